"""Rate of the relative-measurement update (ukfb_update_relative_dev, model UKFB_RELATIVE_POSE, commit = 0 so that every
repetition sees the same state) for uniform lags 1, 4 and 16, beside the delayed-measurement update at the same lags
(ukfb_update_delayed_dev) and the update-only launch (ukfb_update_dev) of the same engine over the same capacity, interleaved so
that all see the same clocks.

EXPECTED, stated before the first run: the delayed call plus roughly one more update's worth.  Both calls run
the same chain (lag backward steps); the relative call then forms Sigma_e (two 12 x 12 row products and a second 12-step
factorisation), evaluates four measurement points per lane instead of two, reduces 21 + 6 row sums instead of 6 + 3, and
factorises a 6 x 6 S in registers instead of a 3 x 3 one, but has no retrodiction (the delayed call's two triangular solves per
row).  The difference (relative - delayed) should therefore not depend on the lag and lie near x1 update-only launches.

Reported: median ms per call over the repetitions, the spread, filter-updates/s (capacity per second), the call's cost in
update-only launches, and per lag the difference to the delayed call in update-only launches.  The history is the engine's
initial state pushed into every slot of a ring of 32 (a timing run: the instruction count of a step depends on its data only
through the trips of the mean iteration); with it Sigma_e is far from singular and no pivot is clamped.

    python tools/relative_rate.py [repetitions=5] [calls per repetition=2] [filters=262144] > profiles/relative_rate.txt
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


def build(n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    e = spe.BatchPoseUKF(n, precision=prec, stream="private")
    e.set_process_noise(sy.pose_default_process_noise())
    mu, cov = sy.pose_initial(n)
    acc, z, Q = sy.pose_cycle_inputs(n, 0, mu[:, :3])
    e.initialize(mu, cov)
    e.set_acceleration(acc, 0.01 * np.eye(3))
    mh = torch.empty((SLOTS, n, e.S), dtype=tdt, device="cuda")
    ch = torch.empty((SLOTS, n, e.PK), dtype=tdt, device="cuda")
    zd = torch.from_numpy(z).to("cuda", tdt).contiguous()
    Qd = torch.from_numpy(Q.reshape(n, 9)).to("cuda", tdt).contiguous()
    # the increment between two equal records: no motion, the identity rotation, 3 cm and 0.02 rad
    zr = torch.zeros((n, 7), dtype=tdt, device="cuda")
    zr[:, 6] = 1.0
    Qr = torch.from_numpy(np.diag([0.03 ** 2] * 3 + [0.02 ** 2] * 3).reshape(36)).to("cuda", tdt).contiguous()
    torch.cuda.synchronize()
    for s in range(SLOTS):
        e.history_push_dev(SLOTS, s, mh, ch)
    e.sync()
    return e, mh, ch, zd, Qd, zr, Qr, tdt


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(n, prec):
    e, mh, ch, zd, Qd, zr, Qr, tdt = build(n, prec)
    mu_out = torch.empty((n, e.S), dtype=tdt, device="cuda")
    cov_out = torch.empty((n, e.PK), dtype=tdt, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    first = 3
    torch.cuda.synchronize()

    def relative(lag):
        e.update_relative_dev(np.full(lag, DT), SLOTS, first, mh, ch, lag, spe.RELATIVE_POSE, zr, Qr, q_is_uniform=True, commit=False,
                              mu_out=mu_out, cov_out=cov_out, status=st)

    def delayed(lag):
        e.update_delayed_dev(np.full(lag, DT), SLOTS, first, mh, ch, lag, spe.MEAS_POS3, zd, Qd, commit=False, mu_out=mu_out,
                             cov_out=cov_out, status=st)

    calls = {}
    for lag in LAGS:
        calls[f"relative lag {lag:2d}"] = lambda lag=lag: relative(lag)
        calls[f"delayed lag {lag:2d}"] = lambda lag=lag: delayed(lag)
    calls["update only"] = lambda: e.update_dev(spe.MEAS_POS3, zd, Qd)
    bad = {}
    for name, fn in calls.items():
        if not name.startswith("update"):
            fn()
            e.sync()
            bad[name] = int((st != 0).sum())
    ms = {name: [] for name in calls}
    for _ in range(REPS):
        for name, fn in calls.items():   # interleaved
            ms[name].append(timed(e, fn))
    label = f"pose {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:30s} {name:20s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filter-updates/s  = x{med[name] / med['update only']:.2f} update-only launches")
    for lag in LAGS:
        r, d = med[f"relative lag {lag:2d}"], med[f"delayed lag {lag:2d}"]
        print(f"{label:30s} lag {lag:2d}: relative / delayed = x{r / d:.2f}, relative - delayed = x{(r - d) / med['update only']:.2f} "
              f"update-only launches (expected: near x1, the same at every lag)")
    print(f"{label:30s} filters with a non-zero status: {bad}")
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, {REPS} repetitions of {CALLS} calls each, HIP-event timing on the engine's stream")
    run(FILTERS, spe.F64)
    run(FILTERS, spe.F32)
