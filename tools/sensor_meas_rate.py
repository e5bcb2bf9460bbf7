"""Rate of the sensor-frame measurement (ukfb_update_sensor_dev, commit = 1) for POSE_POSITION, POSE_RANGE, POSE_VELOCITY and
ORIENT_VELOCITY, beside the update-only launch of the same engine over the same capacity (ukfb_update_dev with POS3;
OrientationState: its body-velocity update), interleaved A/B/A/B so that all see the same clocks.  Reported: median ms per
call over the repetitions, their spread, filter-updates/s and the ratio to the update-only launch.  Mounts r ~ U(-1, 1)^3,
qs = exp(U(-1, 1)^3), beacons 15 ... 80 m away, per filter; the sample is h(mu) of the initial estimate: a timing run -- the
instruction count of an update depends on its data only through the trips of the mean iteration; the covariance shrinks from
call to call and stays positive definite.

    python tools/sensor_meas_rate.py [repetitions=7] [calls per repetition=20] [pose filters=1048576] [orient filters=4194304] \\
        > profiles/sensor_meas_rate.txt

(the tool prints; profiles/sensor_meas_rate.txt is its redirected output, as with tools/state_meas_rate.py)
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import slam_pose_estimation_amd as spe
import sensor_meas_reference as sr

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
POSE_FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
ORIENT_FILTERS = int(sys.argv[4]) if len(sys.argv) > 4 else 4194304


def initial(e, make, n, chunk=262144):
    """initialises the engine chunk by chunk (the covariances of four million filters need not exist at once); -> mu [n, S]"""
    mus = []
    for lo in range(0, n, chunk):
        mu, cov = make(min(chunk, n - lo), first=lo)
        e.initialize(mu, cov, first=lo)
        mus.append(mu)
    return np.concatenate(mus)


def build(kind, n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    rng = np.random.default_rng(5)
    mount = np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)), sr.on.so3_exp(rng.uniform(-1.0, 1.0, (n, 3)))], axis=1)
    d = rng.standard_normal((n, 3))
    away = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(15.0, 80.0, (n, 1))
    if kind == "pose":
        e = spe.BatchPoseUKF(n, precision=prec, stream="private")
        e.set_process_noise(sy.pose_default_process_noise())
        mu = initial(e, sy.pose_initial, n)
        _, z3, Q3 = sy.pose_cycle_inputs(n, 0, mu[:, :3])
        point, gyro = mu[:, 0:3] + away, None
        ids = (spe.SENSOR_POSE_POSITION, spe.SENSOR_POSE_RANGE, spe.SENSOR_POSE_VELOCITY)
    else:
        e = spe.BatchOrientationUKF(n, sy.ORIENT_TAU, sy.ORIENT_TAU, sy.ORIENT_LATITUDE, precision=prec, stream="private")
        e.set_process_noise(sy.orient_process_noise())
        mu = initial(e, sy.orient_initial, n)
        gyro, _, z3, Q3 = sy.orient_cycle_inputs(n, 0, mu[:, :4])
        point = away
        ids = (spe.SENSOR_ORIENT_VELOCITY,)
    if gyro is not None:
        e.set_orient_inputs(gyro=gyro)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)
    zs = {}
    for mid in ids:
        z = np.zeros((n, 3))
        z[:, :sr.meas_dim(mid)] = sr.h(mid, mu, mount, point, gyro)
        zs[mid] = dev(z)
    return e, ids, zs, dev(mount), dev(point), dev(z3), dev(Q3.reshape(n, 9))


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(kind, n, prec):
    e, ids, zs, mount, point, z3d, Q3d = build(kind, n, prec)
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    calls = {sr.NAMES[mid]: (lambda mid=mid: e.update_sensor_dev(mid, zs[mid], Q3d, mount_dev=mount, point_dev=point, status=st))
             for mid in ids}
    base = "update POS3" if kind == "pose" else "update BODYVEL3"
    calls[base] = lambda: e.update_dev(spe.MEAS_POS3 if kind == "pose" else spe.MEAS_ORIENT_BODYVEL3, z3d, Q3d)
    bad = {}
    for name, fn in calls.items():
        fn()
        e.sync()
        bad[name] = int((st != 0).sum()) if name != base else int(e.status_summary() != 0)
    ms = {name: [] for name in calls}
    for _ in range(REPS):
        for name, fn in calls.items():   # interleaved
            ms[name].append(timed(e, fn))
    label = f"{kind} {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:30s} {name:16s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filter-updates/s  = x{med[name] / med[base]:.2f} {base} launches", flush=True)
    print(f"{label:30s} filters with a non-zero status in the first call: {bad}; engine status summary {e.status_summary()}", flush=True)
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, medians of {REPS} repetitions of {CALLS} calls each, HIP-event timing on the engine's stream", flush=True)
    run("pose", POSE_FILTERS, spe.F64)
    run("pose", POSE_FILTERS, spe.F32)
    run("orient", ORIENT_FILTERS, spe.F32)
