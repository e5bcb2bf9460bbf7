"""Rate of the sensor-frame association (ukfb_associate_sensor_dev, POSE_POINT) beside what the same association costs
without it: K calls of ukfb_update_sensor_dev(commit = 0), one per candidate, plus -- for a nearest-neighbour commit -- one
committing call; and the update-only launch (ukfb_update_dev with POS3) on a twin of the same capacity as the yardstick of the
other rate files.  K = 1, 4, 16 candidates, shared-h mode (K detections of one landmark) and per-hypothesis mode (candidate k
pairs its detection with landmark k), commit = 0 and commit = 1, interleaved so that all see the same clocks.

Pose filters from synth.pose_initial, landmarks 15 ... 80 m away (the batch of tools/bearing_rate.py's "ordinary" run).  The
read-only calls run on one engine, whose state never changes; every committing call runs on a second engine, whose state
moves from call to call (the arithmetic of a call does not depend on it).  Outputs asked for: maha, loglik, best, n_gated and
status by the association, maha, loglik and status by each sensor call -- what an association needs; z-bar, S and nu are
left NULL on both sides.  Reported: median ms per association over the repetitions, their spread, filter-associations/s, the
ratio to the K-call alternative of the same commit mode and to update-only launches.

    python tools/associate_rate.py [repetitions=5] [calls per repetition=10] [pose filters=1048576] > profiles/associate_rate.txt
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import slam_pose_estimation_amd as spe
import bearing_reference as br
import sensor_meas_reference as sr

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
POSE_FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
KS = (1, 4, 16)


def initial(engines, n, chunk=262144):
    mus = []
    for lo in range(0, n, chunk):
        mu, cov = spe.synth.pose_initial(min(chunk, n - lo), first=lo)
        for e in engines:
            e.initialize(mu, cov, first=lo)
        mus.append(mu)
    return np.concatenate(mus)


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    ro = spe.BatchPoseUKF(n, precision=prec, stream="private")     # read-only calls
    rw = spe.BatchPoseUKF(n, precision=prec, stream="private")     # committing calls
    twin = spe.BatchPoseUKF(n, precision=prec, stream="private")   # the update-only launch
    for x in (ro, rw, twin):
        x.set_process_noise(sy.pose_default_process_noise())
    mu = initial((ro, rw, twin), n)
    mount, point, _, _ = br.make_inputs(br.on.POSE, mu, 15.0, 80.0, ro.dtype)
    rng = np.random.default_rng(31)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)
    Kmax = max(KS)
    md, pd = dev(mount), dev(point)
    Qd = dev(np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).reshape(n, 9))
    # shared-h mode: K detections around the one landmark's; per-hypothesis mode: landmark k a few metres from the first, its
    # own detection with it
    z_sh = torch.empty((Kmax, n, 3), dtype=tdt, device="cuda")
    z_hy = torch.empty((Kmax, n, 3), dtype=tdt, device="cuda")
    p_hy = torch.empty((Kmax, n, 3), dtype=tdt, device="cuda")
    zc = sr.h(sr.POSE_POINT, mu, mount, point)
    for k in range(Kmax):
        z_sh[k] = dev(zc + 0.05 * (1 + k) * rng.standard_normal((n, 3)))
        pk = point + (2.0 * rng.standard_normal((n, 3)) if k else 0.0)
        p_hy[k] = dev(pk)
        z_hy[k] = dev(sr.h(sr.POSE_POINT, mu, mount, pk) + 0.05 * rng.standard_normal((n, 3)))
    _, z3, Q3 = sy.pose_cycle_inputs(n, 0, mu[:, :3])
    z3d, Q3d = dev(z3), dev(Q3.reshape(n, 9))
    maha = torch.empty((Kmax, n), dtype=tdt, device="cuda")
    ll = torch.empty((Kmax, n), dtype=tdt, device="cuda")
    best = torch.empty((n,), dtype=torch.int32, device="cuda")
    ng = torch.empty((n,), dtype=torch.int32, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    P = spe.SENSOR_POSE_POINT

    def associate(e, K, hyp, commit):
        e.associate_sensor_dev(P, K, z_hy if hyp else z_sh, Qd, mount_dev=md, point_dev=p_hy if hyp else pd, point_per_candidate=hyp,
                               commit=commit, maha=maha, loglik=ll, best=best, n_gated=ng, status=st)

    def k_calls(e, K, hyp, commit):
        for k in range(K):
            e.update_sensor_dev(P, (z_hy if hyp else z_sh)[k], Qd, mount_dev=md, point_dev=p_hy[k] if hyp else pd, commit=False,
                                maha=maha[k], loglik=ll[k], status=st)
        if commit:   # the nearest neighbour's update (which candidate it is does not change the cost)
            e.update_sensor_dev(P, (z_hy if hyp else z_sh)[0], Qd, mount_dev=md, point_dev=p_hy[0] if hyp else pd, commit=True, status=st)

    label = f"pose {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    for K in KS:
        for hyp in (False, True):
            mode = "per-hypothesis" if hyp else "shared-h"
            calls = {}
            for commit in (False, True):
                e = rw if commit else ro
                calls[f"associate commit={int(commit)}"] = (e, lambda e=e, c=commit: associate(e, K, hyp, c))
                calls[f"{K} sensor calls{' + 1 commit' if commit else ''}"] = (e, lambda e=e, c=commit: k_calls(e, K, hyp, c))
            calls["update POS3"] = (twin, lambda: twin.update_dev(spe.MEAS_POS3, z3d, Q3d))
            bad = {}
            for name, (eng, fn) in calls.items():
                fn()
                eng.sync()
                bad[name] = int((st != 0).sum()) if eng is not twin else int(twin.status_summary() != 0)
            ms = {name: [] for name in calls}
            for _ in range(REPS):
                for name, (eng, fn) in calls.items():   # interleaved
                    ms[name].append(timed(eng, fn))
            med = {name: float(np.median(v)) for name, v in ms.items()}
            names = list(calls)
            for name, v in ms.items():
                alt = names[1] if name in names[:2] else (names[3] if name in names[2:4] else name)
                print(f"{label:28s} K={K:<2d} {mode:14s} {name:26s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
                      f"  {n / med[name] / 1e3:8.1f} M filter-associations/s  = x{med[name] / med[alt]:.3f} the K-call alternative"
                      f"  = x{med[name] / med['update POS3']:.2f} update POS3 launches", flush=True)
            print(f"{label:28s} K={K:<2d} {mode:14s} filters with a non-zero status in the first call: {bad}", flush=True)
    ro.close(); rw.close(); twin.close()


if __name__ == "__main__":
    print(f"# interleaved, medians of {REPS} repetitions of {CALLS} calls each, HIP-event timing on each engine's stream", flush=True)
    for prec in (spe.F64, spe.F32):
        run(POSE_FILTERS, prec)
