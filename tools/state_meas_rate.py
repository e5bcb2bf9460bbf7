"""Rate of the joint state-block measurement (ukfb_update_state_dev, commit = 1) for the full mask and, Pose, the 6-DOF mask
{position, orientation}, beside the update-only POS3 launch (ukfb_update_dev; OrientationState: its body-velocity update) of the
same engine over the same capacity, interleaved A/B/A/B so that all see the same clocks.  Reported: median ms per call, the
spread over the repetitions, filter-updates/s and the ratio to the update-only launch.  The measurement is the engine's own
initial estimate (z = mu, Qz = Sigma): a timing run -- the instruction count of an update depends on its data only through the
trips of the mean iteration; the covariance shrinks from call to call and stays positive definite.

    python tools/state_meas_rate.py [repetitions=5] [calls per repetition=4] [filters=262144] > profiles/state_meas_rate.txt

(the tool prints; profiles/state_meas_rate.txt is its redirected output, as with tools/smoother_rate.py)
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import slam_pose_estimation_amd as spe

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 4
FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 262144


def build(kind, n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    if kind == "pose":
        e = spe.BatchPoseUKF(n, precision=prec, stream="private")
        e.set_process_noise(sy.pose_default_process_noise())
        mu, cov = sy.pose_initial(n)
        _, z3, Q3 = sy.pose_cycle_inputs(n, 0, mu[:, :3])
        e.initialize(mu, cov)
    else:
        e = spe.BatchOrientationUKF(n, sy.ORIENT_TAU, sy.ORIENT_TAU, sy.ORIENT_LATITUDE, precision=prec, stream="private")
        e.set_process_noise(sy.orient_process_noise())
        mu, cov = sy.orient_initial(n)
        _, _, z3, Q3 = sy.orient_cycle_inputs(n, 0, mu[:, :4])
        e.initialize(mu, cov)
    r, c = np.tril_indices(e.D)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)
    return e, dev(mu), dev(cov[:, r, c]), dev(z3), dev(Q3.reshape(n, 9)), tdt


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(kind, n, prec):
    e, zd, qd, z3d, Q3d, tdt = build(kind, n, prec)
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    masks = {"full mask": spe.BLOCK_POSE_ALL if kind == "pose" else spe.BLOCK_ORIENT_ALL}
    if kind == "pose":
        masks["6-DOF mask"] = spe.BLOCK_POSE_POSITION | spe.BLOCK_POSE_ORIENTATION
    calls = {name: (lambda m=m: e.update_state_dev(m, zd, qd, status=st)) for name, m in masks.items()}
    base = "update POS3" if kind == "pose" else "update BODYVEL3"
    calls[base] = lambda: e.update_dev(spe.MEAS_POS3 if kind == "pose" else spe.MEAS_ORIENT_BODYVEL3, z3d, Q3d)
    bad = {}
    for name, fn in calls.items():
        fn()
        e.sync()
        bad[name] = int((st != 0).sum()) if name in masks else int(e.status_summary() != 0)
    ms = {name: [] for name in calls}
    for _ in range(REPS):
        for name, fn in calls.items():   # interleaved
            ms[name].append(timed(e, fn))
    label = f"{kind} {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:30s} {name:16s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filter-updates/s  = x{med[name] / med[base]:.2f} {base} launches")
    print(f"{label:30s} filters with a non-zero status in the first call: {bad}; engine status summary {e.status_summary()}")
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, {REPS} repetitions of {CALLS} calls each, HIP-event timing on the engine's stream")
    run("pose", FILTERS, spe.F64)
    run("pose", FILTERS, spe.F32)
    run("orient", FILTERS, spe.F64)
    run("orient", FILTERS, spe.F32)
