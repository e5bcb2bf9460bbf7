"""Rate of the user-defined process models beside the calls that compute the same thing with a built-in model, interleaved so that
all see the same clocks:

    export             ukfb_sigma_points_dev (X only): it STORES the record the prediction loads
    predict_sampled    ukfb_predict_sampled_dev, commit = 1, on propagated points of the initial export (the call does not read
                       the state: the same points give the same prediction every time)
    predict_sampled c=0  the same with commit = 0 and the outputs mu / cov_packed / status
    torch f            the torch expression of the chain alone (the built-in constant-velocity Pose model on the exported X,
                       eager mode)
    chain              export, XX = f(X) as a torch expression, ukfb_predict_sampled_dev with commit = 1 and the R the built-in
                       predict forms (unrotated here: a timing run)
    forecast 1 step    ukfb_forecast_dev, one step into a ring (read-only: the built-in model without the commit)
    predict            ukfb_predict, the predict-only launch: the like-for-like line for the chain

Reported: median ms per call over the repetitions, their spread, filter-predictions/s, the ratio to the export and the ratio to
ukfb_predict.  The engine runs on torch's current stream, so that the torch expression of the chain is ordered with the two
calls and is inside the HIP-event timing.  The predict launch comes last in every round: it moves the engine's state.  There is
no threshold: the output is the record.

    python tools/predict_sampled_rate.py [repetitions=7] [calls per repetition=10] [pose filters=1048576] > profiles/predict_sampled_rate.txt
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import slam_pose_estimation_amd as spe
import predict_sampled_reference as pr

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
DT = 0.01


def run(n, prec, chunk=262144):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    e = spe.BatchPoseUKF(n, precision=prec, stream="torch")
    e.set_process_noise(sy.pose_default_process_noise())
    for lo in range(0, n, chunk):
        mu, cov = sy.pose_initial(min(chunk, n - lo), first=lo)
        e.initialize(mu, cov, first=lo)
    X = torch.empty((n, 2 * e.D + 1, e.S), dtype=tdt, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    mo = torch.empty((1, n, e.S), dtype=tdt, device="cuda")
    co = torch.empty((1, n, e.PK), dtype=tdt, device="cuda")
    R = torch.from_numpy(DT * sy.pose_default_process_noise()).to("cuda", tdt).contiguous()
    e.sigma_points_dev(X, None, st)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    f = lambda: pr.pose_builtin(X, None, DT).contiguous()   # noqa: E731
    XX = f()

    def chain():
        e.sigma_points_dev(X, None, None)
        e.predict_sampled_dev(f(), R, r_is_uniform=True, status=st)

    calls = {"export": lambda: e.sigma_points_dev(X, None, st),
             "predict_sampled": lambda: e.predict_sampled_dev(XX, R, r_is_uniform=True, status=st),
             "predict_sampled c=0": lambda: e.predict_sampled_dev(XX, R, r_is_uniform=True, commit=False, mu=mo[0], cov_packed=co[0], status=st),
             "torch f": f,
             "chain": chain,
             "forecast 1 step": lambda: e.forecast_dev(1, 0, mo, co, st, dt=np.full(1, DT)),
             "predict": lambda: e.predict(DT)}
    base = "predict"
    bad = {}
    for name, fn in calls.items():
        if name == base:
            continue
        fn()
        e.sync()
        bad[name] = int((st != 0).sum())

    def timed(fn):
        e.timer_begin()
        for _ in range(CALLS):
            fn()
        return e.timer_end() / CALLS
    ms = {name: [] for name in calls}
    for _ in range(REPS):
        for name, fn in calls.items():   # interleaved
            ms[name].append(timed(fn))
    label = f"pose {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:28s} {name:20s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filter-predictions/s  = x{med[name] / med['export']:.2f} export = x{med[name] / med[base]:.2f} {base}", flush=True)
    rec = X.element_size() * (2 * e.D + 1) * e.S
    print(f"{label:28s} sigma-point record {rec} B per filter: the export writes it at {n * rec / med['export'] / 1e6:.0f} GB/s, "
          f"predict_sampled reads it at {n * rec / med['predict_sampled'] / 1e6:.0f} GB/s (commit = 0: {n * rec / med['predict_sampled c=0'] / 1e6:.0f} GB/s)", flush=True)
    print(f"{label:28s} filters with a non-zero status in the first call: {bad}; engine status summary after the timing: {e.status_summary()}", flush=True)
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, medians of {REPS} repetitions of {CALLS} calls each, HIP-event timing on the engine's (torch's) stream", flush=True)
    run(FILTERS, spe.F64)
    run(FILTERS, spe.F32)
