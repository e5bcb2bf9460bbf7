"""Rate of the late sensor-frame samples (ukfb_update_delayed_sensor_dev, models UKFB_SENSOR_POSE_POSITION and
UKFB_SENSOR_POSE_POINT, commit = 0 so that every repetition sees the same state) for uniform lags 0, 1, 4 and 16, beside the
delayed-measurement update at the same lags (ukfb_update_delayed_dev, model 0) and the sensor-frame update of the present state
(ukfb_update_sensor_dev, commit = 0) on the same engine over the same capacity, interleaved so that all see the same clocks.

EXPECTED, stated before the first run: little more than the delayed call at lag >= 4, and near the sensor-frame
update plus the retrodiction at lag 0.  The chain is shared with the delayed call, statement for statement (lag backward steps,
each a redone prediction and two factorisations).  The measurement half adds, once per call, up to three fp64 quaternion
rotations per sigma point (POSITION: one, POINT: two or three) and the staging of 25 scalars; and, once per backward step, the
lane-owned look at those 25 scalars by which the chain learns the row's reach (two loads per lane and one row vote).  Against
a chain step of several thousand instructions both are small: delayed_sensor / delayed should be x1.00 ... x1.05 at lags 4 and
16 and the difference (delayed_sensor - delayed) should not grow with the lag by more than a few per cent of a step.  At lag 0
there is no chain: the call is the sensor-frame update's work plus the delayed call's retrodiction (N = Sigma_n M^T, two
triangular solves per row) and its second record load, so it should sit between x1.0 and x1.5 of the sensor-frame update and
within a few per cent of the delayed call at lag 0.

Reported: median ms per call over the repetitions, the spread, filter-updates/s (capacity per second), per lag the ratio and the
difference to the delayed call, and at lag 0 the ratio to the sensor-frame update.  The history is the engine's initial state
pushed into every slot of a ring of 17 (a timing run: the instruction count of a step depends on its data only through the
trips of the mean iteration).

    python tools/delayed_sensor_rate.py [repetitions=5] [calls per repetition=2] [filters=1048576] > profiles/delayed_sensor_rate.txt
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import slam_pose_estimation_amd as spe
from oracle import ukf_numpy as on

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
SLOTS = 17
LAGS = (0, 1, 4, 16)
DT = 0.01
MODELS = {"POSITION": spe.SENSOR_POSE_POSITION, "POINT": spe.SENSOR_POSE_POINT}


def build(n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda", tdt).contiguous()   # noqa: E731
    e = spe.BatchPoseUKF(n, precision=prec, stream="private")
    e.set_process_noise(sy.pose_default_process_noise())
    mu, cov = sy.pose_initial(n)
    acc, z0, Q = sy.pose_cycle_inputs(n, 0, mu[:, :3])
    e.initialize(mu, cov)
    e.set_acceleration(acc, 0.01 * np.eye(3))
    mh = torch.empty((SLOTS, n, e.S), dtype=tdt, device="cuda")
    ch = torch.empty((SLOTS, n, e.PK), dtype=tdt, device="cuda")
    # a lever arm of 1 m, a sensor turned against the body, a landmark 5 m away; the samples 3 cm off what the state predicts
    rng = np.random.default_rng(7)
    d = rng.standard_normal((n, 3))
    r = d / np.linalg.norm(d, axis=1, keepdims=True)
    qs = on.so3_exp(rng.uniform(-1.0, 1.0, (n, 3)))
    d = rng.standard_normal((n, 3))
    b = mu[:, 0:3] + 5.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    p, q = mu[:, 0:3], mu[:, 3:7]
    z = {"POSITION": p + on.quat_rotate(q, r) + 0.03,
         "POINT": on.quat_rotate(on.quat_inverse(qs), on.quat_rotate(on.quat_inverse(q), b - p) - r) + 0.03}
    dev = dict(z0=up(z0), Q=up(Q.reshape(n, 9)), mount=up(np.concatenate([r, qs], axis=1)), point=up(b), z={k: up(v) for k, v in z.items()})
    torch.cuda.synchronize()
    for s in range(SLOTS):
        e.history_push_dev(SLOTS, s, mh, ch)
    e.sync()
    return e, mh, ch, dev, tdt


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(n, prec):
    e, mh, ch, d, tdt = build(n, prec)
    mu_out = torch.empty((n, e.S), dtype=tdt, device="cuda")
    cov_out = torch.empty((n, e.PK), dtype=tdt, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    first = 3
    torch.cuda.synchronize()

    def delayed_sensor(name, lag):
        e.update_delayed_sensor_dev(np.full(lag, DT), SLOTS, first, mh, ch, lag, MODELS[name], d["z"][name], d["Q"], mount_dev=d["mount"],
                                    point_dev=d["point"], commit=False, mu_out=mu_out, cov_out=cov_out, status=st)

    def delayed(lag):
        e.update_delayed_dev(np.full(lag, DT), SLOTS, first, mh, ch, lag, spe.MEAS_POS3, d["z0"], d["Q"], commit=False, mu_out=mu_out,
                             cov_out=cov_out, status=st)

    def sensor(name):
        e.update_sensor_dev(MODELS[name], d["z"][name], d["Q"], mount_dev=d["mount"], point_dev=d["point"], commit=False, status=st)

    calls = {}
    for lag in LAGS:
        for name in MODELS:
            calls[f"delayed_sensor {name:8s} lag {lag:2d}"] = lambda name=name, lag=lag: delayed_sensor(name, lag)
        calls[f"delayed model 0         lag {lag:2d}"] = lambda lag=lag: delayed(lag)
    for name in MODELS:
        calls[f"sensor {name:8s} (present)"] = lambda name=name: sensor(name)
    bad = {}
    for name, fn in calls.items():   # warm-up, and the statuses
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
        print(f"{label:30s} {name:32s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})  {n / med[name] / 1e3:9.1f} M filter-updates/s")
    step = (med[f"delayed model 0         lag {16:2d}"] - med[f"delayed model 0         lag {4:2d}"]) / 12.0
    print(f"{label:30s} one backward step of the delayed call: {step:.4f} ms")
    for lag in LAGS:
        dl = med[f"delayed model 0         lag {lag:2d}"]
        for name in MODELS:
            ds = med[f"delayed_sensor {name:8s} lag {lag:2d}"]
            line = f"{label:30s} lag {lag:2d} {name:8s}: delayed_sensor / delayed = x{ds / dl:.3f}, delayed_sensor - delayed = {ds - dl:+.4f} ms = {(ds - dl) / step:+.2f} steps"
            if lag == 0:
                line += f"; / sensor-frame update = x{ds / med[f'sensor {name:8s} (present)']:.3f} (expected x1.0 ... x1.5)"
            else:
                line += " (expected x1.00 ... x1.05)" if lag >= 4 else ""
            print(line)
    print(f"{label:30s} filters with a non-zero status: {[k for k, v in bad.items() if v]} (of {len(bad)} calls)")
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, {REPS} repetitions of {CALLS} calls each after one warm-up call of each kind, HIP-event timing on the engine's stream")
    run(FILTERS, spe.F64)
    run(FILTERS, spe.F32)
