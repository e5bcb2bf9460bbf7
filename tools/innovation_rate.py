"""Rate of the read-only innovation statistics (ukfb_innovation_dev, every output requested) in filter-evaluations/s for
1, 4 and 16 candidates per filter, and beside it the update-only launch (ukfb_update_dev) on the same engine, interleaved
A/B/A/B so that both see the same clocks.  Reported: median ms per launch, the spread (min ... max) over the repetitions, the
ratio to the update launch and the cost of a further candidate (slope between 4 and 16 candidates).

    python tools/innovation_rate.py [repetitions=7] [launches per repetition=20]
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import slam_pose_estimation_amd as spe

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
LAUNCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 20
KMAX = 16
CHUNK = 262144


def build(kind, n, prec):
    """engine with the bench workload's state after one prediction; inputs resident on the device"""
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    if kind == "pose":
        e = spe.BatchPoseUKF(n, precision=prec, stream="private")
        e.set_process_noise(sy.pose_default_process_noise())
    else:
        e = spe.BatchOrientationUKF(n, sy.ORIENT_TAU, sy.ORIENT_TAU, sy.ORIENT_LATITUDE, precision=prec, stream="private")
        e.set_process_noise(sy.orient_process_noise())
    z = torch.empty((KMAX, n, 3), dtype=tdt, device="cuda")
    Q = torch.empty((n, 9), dtype=tdt, device="cuda")
    rng = np.random.default_rng(5)
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        if kind == "pose":
            mu, cov = sy.pose_initial(hi - lo, first=lo)
            acc, z0, Qh = sy.pose_cycle_inputs(hi - lo, 0, mu[:, :3], first=lo)
            e.initialize(mu, cov, first=lo)
            e.set_acceleration(acc, 0.01 * np.eye(3), first=lo)
        else:
            mu, cov = sy.orient_initial(hi - lo, first=lo)
            gyro, acc, z0, Qh = sy.orient_cycle_inputs(hi - lo, 0, mu[:, :4], first=lo)
            e.initialize(mu, cov, first=lo)
            e.set_orient_inputs(gyro, acc, first=lo)
        for k in range(KMAX):   # candidate 0: the bench's sample; the others: clutter around it
            z[k, lo:hi] = torch.from_numpy(z0 + (0.05 * k) * rng.uniform(-1, 1, z0.shape)).to("cuda", tdt)
        Q[lo:hi] = torch.from_numpy(Qh.reshape(-1, 9)).to("cuda", tdt)
    e.predict(0.01)
    e.sync()
    out = dict(z_pred=torch.empty((n, 4), dtype=tdt, device="cuda"), S=torch.empty((n, 9), dtype=tdt, device="cuda"),
               innov=torch.empty((KMAX, n, 3), dtype=tdt, device="cuda"), maha=torch.empty((KMAX, n), dtype=tdt, device="cuda"),
               loglik=torch.empty((KMAX, n), dtype=tdt, device="cuda"), best=torch.empty(n, dtype=torch.int32, device="cuda"),
               status=torch.empty(n, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return e, z, Q, out


def timed(e, fn):
    e.timer_begin()
    for _ in range(LAUNCHES):
        fn()
    return e.timer_end() / LAUNCHES


def run(kind, n, prec, model):
    e, z, Q, out = build(kind, n, prec)
    mu0, cov0, _ = e.state(0, min(n, 1024))
    calls = {"update": lambda: e.update_dev(model, z[0], Q)}
    for k in (1, 4, 16):
        calls[f"innovation K={k}"] = (lambda k=k: e.innovation_dev(model, k, z, Q, **out))
    ms = {name: [] for name in calls}
    for name, fn in calls.items():   # warm-up (the update converges on its sample: later launches see the same work)
        for _ in range(3):
            fn()
    e.sync()
    for _ in range(REPS):
        for name, fn in calls.items():   # interleaved
            ms[name].append(timed(e, fn))
    label = f"{kind} {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:34s} {name:18s} {med[name]:8.4f} ms  (min {min(v):.4f} max {max(v):.4f}, spread {100 * (max(v) - min(v)) / med[name]:.1f} %)"
              f"  {n / med[name] / 1e3:9.1f} M filter-evaluations/s  x{med[name] / med['update']:.3f} of the update launch")
    slope = (med["innovation K=16"] - med["innovation K=4"]) / 12.0
    b = 8 if prec == spe.F64 else 4
    print(f"{label:34s} per further candidate: {slope * 1e3:.2f} us = {n * 8 * b / (slope * 1e-3) / 1e9 if slope > 0 else float('nan'):.0f} GB/s of its 8 scalars per filter")
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, {REPS} repetitions of {LAUNCHES} launches each, HIP-event timing on the engine's stream")
    run("pose", 1048576, spe.F64, spe.MEAS_POS3)
    run("pose", 1048576, spe.F32, spe.MEAS_POS3)
    run("pose", 1048576, spe.F64, spe.MEAS_ORIENT_SO3)
    run("orient", 4194304, spe.F32, spe.MEAS_ORIENT_BODYVEL3)
