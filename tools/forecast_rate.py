"""Rate of the forecast (ukfb_forecast_dev) for horizons of 1, 8 and 32 steps, beside the predict-only launch (ukfb_predict) of
the same engine over the same capacity, interleaved A/B/A/B so that all see the same clocks.  Reported: median ms per call, the
spread over the repetitions, filter-steps/s (capacity x steps per second) and the ratio of that rate to ukfb_predict's of the
same build (one predict launch = one filter-step per filter).  For a horizon above 1 the state crosses HBM once, where `steps`
predict launches read and write it `steps` times: a ratio below 1 there would be a finding to explain.  The forecast starts from
the engine's state with the latched inputs and writes to a ring of 32 slots (a timing run: the instruction count of a step
depends on its data only through the trips of the mean iteration).

    python tools/forecast_rate.py [repetitions=5] [calls per repetition=4] [filters=262144] > profiles/forecast_rate.txt

(the tool prints; profiles/forecast_rate.txt is its redirected output, as with tools/smoother_rate.py)
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import slam_pose_estimation_amd as spe

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 4
FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 262144
SLOTS = 32


def build(kind, n, prec):
    sy = spe.synth
    if kind == "pose":
        e = spe.BatchPoseUKF(n, precision=prec, stream="private")
        e.set_process_noise(sy.pose_default_process_noise())
        mu, cov = sy.pose_initial(n)
        acc, _, _ = sy.pose_cycle_inputs(n, 0, mu[:, :3])
        e.initialize(mu, cov)
        e.set_acceleration(acc, 0.01 * np.eye(3))
    else:
        e = spe.BatchOrientationUKF(n, sy.ORIENT_TAU, sy.ORIENT_TAU, sy.ORIENT_LATITUDE, precision=prec, stream="private")
        e.set_process_noise(sy.orient_process_noise())
        mu, cov = sy.orient_initial(n)
        gyro, acc, _, _ = sy.orient_cycle_inputs(n, 0, mu[:, :4])
        e.initialize(mu, cov)
        e.set_orient_inputs(gyro, acc)
    e.sync()
    return e


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(kind, n, prec):
    e = build(kind, n, prec)
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    mo = torch.empty((SLOTS, n, e.S), dtype=tdt, device="cuda")
    co = torch.empty((SLOTS, n, e.PK), dtype=tdt, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    calls = {}
    for steps in (1, 8, 32):
        calls[f"forecast {steps:2d} steps"] = (steps, lambda steps=steps: e.forecast_dev(SLOTS, 3, mo, co, st, dt=np.full(steps, 0.01)))
    bad = 0
    for _, fn in calls.values():
        fn()
        e.sync()
        bad = max(bad, int((st != 0).sum()))
    # the predict launch last in every round: it moves the engine's state, from which the next forecast starts
    ms = {name: [] for name in calls}
    ms["predict"] = []
    for _ in range(REPS):
        for name, (_, fn) in calls.items():   # interleaved
            ms[name].append(timed(e, fn))
        ms["predict"].append(timed(e, lambda: e.predict(0.01)))
    label = f"{kind} {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        steps = calls[name][0] if name in calls else 1
        print(f"{label:30s} {name:17s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n * steps / med[name] / 1e3:9.1f} M filter-steps/s  rate = x{steps * med['predict'] / med[name]:.2f} ukfb_predict")
    print(f"{label:30s} filters with a non-zero forecast status: {bad}; engine status summary {e.status_summary()}")
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, {REPS} repetitions of {CALLS} calls each, HIP-event timing on the engine's stream")
    run("pose", FILTERS, spe.F64)
    run("pose", FILTERS, spe.F32)
    run("orient", FILTERS, spe.F32)
