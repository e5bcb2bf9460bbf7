"""Rate of the delayed-measurement update (ukfb_update_delayed_dev, commit = 0 so that every repetition sees the same state) for
uniform lags 1, 4 and 16 and for lags mixed 0 ... 16 over the filters, beside three other workloads of the same engine over the
same capacity, interleaved A/B/C/D so that all see the same clocks:

  * a smoother window of the same length (ukfb_smooth_dev over lag + 1 steps),
  * the update-only launch (ukfb_update_dev),
  * the replay alternative: scatter the ring's record of the sample's step into the engine (ukfb_scatter_filters_dev), then
    `lag` fused cycles in one launch (ukfb_cycle_multi_dev) -- which needs the measurements of those cycles stored, the same
    lag for every filter, and one model per cycle.

Reported: median ms per call over the repetitions, the spread, filter-updates/s (capacity per second) and the call's cost in
update-only launches.  The history is the engine's initial state pushed into every slot of a ring of 32 (a timing run: the
instruction count of a step depends on its data only through the trips of the mean iteration).

    python tools/delayed_rate.py [repetitions=5] [calls per repetition=2] [filters=262144] > profiles/delayed_rate.txt
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import slam_pose_estimation_amd as spe

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 262144
SLOTS = 32
LAGS = (1, 4, 16)
DT = 0.01


def build(kind, n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    if kind == "pose":
        e = spe.BatchPoseUKF(n, precision=prec, stream="private")
        e.set_process_noise(sy.pose_default_process_noise())
        mu, cov = sy.pose_initial(n)
        acc, z, Q = sy.pose_cycle_inputs(n, 0, mu[:, :3])
        e.initialize(mu, cov)
        e.set_acceleration(acc, 0.01 * np.eye(3))
        model = spe.MEAS_POS3
    else:
        e = spe.BatchOrientationUKF(n, sy.ORIENT_TAU, sy.ORIENT_TAU, sy.ORIENT_LATITUDE, precision=prec, stream="private")
        e.set_process_noise(sy.orient_process_noise())
        mu, cov = sy.orient_initial(n)
        gyro, acc, z, Q = sy.orient_cycle_inputs(n, 0, mu[:, :4])
        e.initialize(mu, cov)
        e.set_orient_inputs(gyro, acc)
        model = spe.MEAS_ORIENT_BODYVEL3
    mh = torch.empty((SLOTS, n, e.S), dtype=tdt, device="cuda")
    ch = torch.empty((SLOTS, n, e.PK), dtype=tdt, device="cuda")
    zr = torch.from_numpy(z).to("cuda", tdt).repeat(SLOTS, 1, 1).contiguous()
    Qr = torch.from_numpy(Q.reshape(n, 9)).to("cuda", tdt).repeat(SLOTS, 1, 1).contiguous()
    torch.cuda.synchronize()
    for s in range(SLOTS):
        e.history_push_dev(SLOTS, s, mh, ch)
    e.sync()
    return e, mh, ch, zr, Qr, model, tdt


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(kind, n, prec):
    e, mh, ch, zr, Qr, model, tdt = build(kind, n, prec)
    mo, co = torch.empty_like(mh), torch.empty_like(ch)
    mu_out = torch.empty((n, e.S), dtype=tdt, device="cuda")
    cov_out = torch.empty((n, e.PK), dtype=tdt, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    mixed = (torch.arange(n, dtype=torch.int32, device="cuda") % 17).contiguous()
    first = 3
    torch.cuda.synchronize()

    def delayed(lag, steps):
        e.update_delayed_dev(np.full(steps - 1, DT), SLOTS, first, mh, ch, lag, model, zr[0], Qr[0], commit=False, mu_out=mu_out,
                             cov_out=cov_out, status=st)

    def replay(lag):
        e.scatter_filters_dev(idx, mh[first], ch[first])   # step 0 of the window is the sample's step
        e.cycle_multi_dev(lag, DT, model, zr, Qr, SLOTS, first)

    calls = {}
    for lag in LAGS:
        calls[f"delayed lag {lag:2d}"] = lambda lag=lag: delayed(lag, lag + 1)
        calls[f"smooth {lag + 1:2d} steps"] = lambda lag=lag: e.smooth_dev(np.full(lag, DT), SLOTS, first, mh, ch, mo, co, st)
        calls[f"replay lag {lag:2d}"] = lambda lag=lag: replay(lag)
    calls["delayed lags 0..16"] = lambda: delayed(mixed, 17)
    calls["update only"] = lambda: e.update_dev(model, zr[0], Qr[0])
    bad = {}
    for name, fn in calls.items():
        if name.startswith("delayed"):
            fn()
            e.sync()
            bad[name] = int((st != 0).sum())
    ms = {name: [] for name in calls}
    for _ in range(REPS):
        for name, fn in calls.items():   # interleaved
            ms[name].append(timed(e, fn))
    label = f"{kind} {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:30s} {name:20s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filter-updates/s  = x{med[name] / med['update only']:.2f} update-only launches")
    for lag in LAGS:
        d, s, r = med[f"delayed lag {lag:2d}"], med[f"smooth {lag + 1:2d} steps"], med[f"replay lag {lag:2d}"]
        print(f"{label:30s} lag {lag:2d}: delayed / smoother window = x{d / s:.2f}, delayed - smoother = x{(d - s) / med['update only']:.2f} "
              f"update-only launches, delayed / replay = x{d / r:.2f}")
    print(f"{label:30s} filters with a non-zero status of the delayed call: {bad}")
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, {REPS} repetitions of {CALLS} calls each, HIP-event timing on the engine's stream")
    run("pose", FILTERS, spe.F64)
    run("pose", FILTERS, spe.F32)
    run("orient", FILTERS, spe.F32)
