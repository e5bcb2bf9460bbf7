"""Rate of the bearing measurement (ukfb_update_bearing_dev, POSE_POINT) beside the sensor-frame landmark fix
(ukfb_update_sensor_dev, POSE_POINT) on the same engine and the update-only launch (ukfb_update_dev with POS3) on a twin of the
same capacity, interleaved A/B/C/A/B/C so that all see the same clocks.  Two batches of Pose filters (the batches of
tests/test_gpu_bearing.py, from synth.pose_initial): the ordinary one, landmarks 15 ... 80 m away, and the wide one, Sigma x 4
and landmarks 0.6 ... 2.0 m from the body origin, on which the mean iteration on the sphere really iterates.  Reported: median
ms per call over the repetitions, their spread, filter-updates/s, the ratio to the sensor POINT update and to the update-only
launch, and the mean trips per filter of each batch (steps of the mean iteration above mean_tol, by the NumPy reference on the
first filters of the batch; the kernel's loop makes one more pass, which confirms).

The bearing and the sensor call run with commit = 0: every step still runs (include/ukf_batch.h), only the stores of the state
are left out, and the batch -- with it the trips of the mean iteration -- stays what it was from call to call.

    python tools/bearing_rate.py [repetitions=7] [calls per repetition=20] [pose filters=1048576] [reference filters=8192] \\
        > profiles/bearing_rate.txt
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import slam_pose_estimation_amd as spe
import bearing_reference as br
import sensor_meas_reference as sr

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
POSE_FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
REF_FILTERS = int(sys.argv[4]) if len(sys.argv) > 4 else 8192
BATCHES = {"ordinary": (1.0, 15.0, 80.0), "wide": (4.0, 0.6, 2.0)}


def initial(engines, n, scale, chunk=262144):
    """initialises the engines chunk by chunk; -> (mu [n, S], cov of the first REF_FILTERS filters)"""
    mus, head = [], None
    for lo in range(0, n, chunk):
        mu, cov = spe.synth.pose_initial(min(chunk, n - lo), first=lo)
        for e in engines:
            e.initialize(mu, scale * cov, first=lo)
        mus.append(mu)
        if lo == 0:
            head = scale * cov[:REF_FILTERS]
    return np.concatenate(mus), head


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(batch, n, prec):
    scale, lo, hi = BATCHES[batch]
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    e = spe.BatchPoseUKF(n, precision=prec, stream="private")
    twin = spe.BatchPoseUKF(n, precision=prec, stream="private")
    for x in (e, twin):
        x.set_process_noise(sy.pose_default_process_noise())
    mu, cov_head = initial((e, twin), n, scale)
    mount, point, z, Q = br.make_inputs(br.on.POSE, mu, lo, hi, e.dtype)
    _, z3, Q3 = sy.pose_cycle_inputs(n, 0, mu[:, :3])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)
    zb, Qb, md, pd = dev(z[br.POSE_POINT]), dev(Q.reshape(n, 9)), dev(mount), dev(point)
    zs = dev(sr.h(sr.POSE_POINT, mu, mount, point))
    Qs = dev(np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).reshape(n, 9))
    z3d, Q3d = dev(z3), dev(Q3.reshape(n, 9))
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    calls = {
        "bearing POINT": (e, lambda: e.update_bearing_dev(spe.BEARING_POSE_POINT, zb, Qb, mount_dev=md, point_dev=pd, commit=False, status=st)),
        "sensor POINT": (e, lambda: e.update_sensor_dev(spe.SENSOR_POSE_POINT, zs, Qs, mount_dev=md, point_dev=pd, commit=False, status=st)),
        "update POS3": (twin, lambda: twin.update_dev(spe.MEAS_POS3, z3d, Q3d)),
    }
    bad = {}
    for name, (eng, fn) in calls.items():
        fn()
        eng.sync()
        bad[name] = int((st != 0).sum()) if eng is e else int(twin.status_summary() != 0)
    ms = {name: [] for name in calls}
    for _ in range(REPS):
        for name, (eng, fn) in calls.items():   # interleaved
            ms[name].append(timed(eng, fn))
    label = f"{batch} pose {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:36s} {name:14s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filter-updates/s  = x{med[name] / med['sensor POINT']:.2f} sensor POINT"
              f"  = x{med[name] / med['update POS3']:.2f} update POS3 launches", flush=True)
    print(f"{label:36s} filters with a non-zero status in the first call: {bad}", flush=True)
    k = min(REF_FILTERS, n)
    stored = lambda a: np.asarray(a, dtype=np.float64).astype(e.dtype).astype(np.float64)
    ref = br.update_bearing(br.on.POSE, stored(mu[:k]), stored(cov_head[:k]), br.POSE_POINT, z[br.POSE_POINT][:k], Q[:k], mount[:k], point[:k])
    trips = ref["trips"][ref["status"] == 0]
    print(f"{label:36s} mean trips per filter (reference, first {k} filters): {trips.mean():.4f}; filters by trips "
          f"{dict(enumerate(np.bincount(trips).tolist()))}; largest sigma-point angle from z-bar {np.nanmax(ref['spread']):.3f} rad", flush=True)
    e.close()
    twin.close()


if __name__ == "__main__":
    print(f"# interleaved, medians of {REPS} repetitions of {CALLS} calls each, HIP-event timing on each engine's stream", flush=True)
    for prec in (spe.F64, spe.F32):
        for batch in ("ordinary", "wide"):
            run(batch, POSE_FILTERS, prec)
