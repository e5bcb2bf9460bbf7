"""Rate of the covariance conditioning (ukfb_condition_dev) at 1 048 576 Pose filters, beside the update-only launch and a
device-to-device copy of the state's bytes, interleaved so that all see the same clocks.  Three batches, each in an engine of its
own:

    healthy      every filter as synth.pose_initial makes it: the Jacobi sweeps run, nothing is repaired
    1 % deficient  every 100th filter has lambda_min = -1e-3 (tests/condition_reference.with_eigenvalues): one wavefront in 25
                 runs the correction
    deficient    every filter has lambda_min = -1e-3

and per batch

    condition c=1   commit = 1, out = status only.  A committed repair makes the filter healthy, so the deficient batches restore
                    their covariances in front of every call (a device-to-device copy of the packed covariances on the same
                    stream, INSIDE the timed region: `restore` is that copy alone, to be subtracted)
    condition c=0   commit = 0 with the outputs eig_min, eig_max and status (the monitoring call)

then, once,

    restore         the copy of the packed covariances alone
    state copy      hipMemcpyAsync device to device of the bytes of the state (mean + packed covariance)
    update          ukfb_update_dev (MEAS_POS3) on a fourth, healthy engine: the update-only launch

Reported: median ms per call over the repetitions, their spread, filters/s, and the ratios to the update and to the state copy.
eps = 1e-10 (fp64) / 1e-4 (fp32), the floor 1e-3 of the smallest variance.  The populations are tiled from 65 536 synthesised
filters (a timing run).  There is no threshold: the output is the record.

    python tools/condition_rate.py [repetitions=7] [calls per repetition=5] [pose filters=1048576] > profiles/condition_rate.txt
"""
import torch  # noqa: F401
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import slam_pose_estimation_amd as spe
import condition_reference as cr

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
UNIQUE = 65536
HIP = C.CDLL("libamdhip64.so")
ST_REPAIRED = 1 << 11
BATCHES = (("healthy", 0), ("1 % deficient", 100), ("deficient", 1))


def build(n, prec, every, mu, cov, bad):
    """an engine of n filters tiled from (mu, cov); filter i is deficient (bad[i % m]) iff every > 0 and i % every == 0"""
    m = mu.shape[0]
    e = spe.BatchPoseUKF(n, precision=prec, stream="torch")
    for lo in range(0, n, m):   # chunked: the full covariances of a million filters are 1.2 GB of doubles
        k = min(m, n - lo)
        c = cov[:k]
        if every:
            pick = (lo + np.arange(k)) % every == 0
            c = np.where(pick[:, None, None], bad[:k], c)
        e.initialize(mu[:k], c, first=lo)
    e.sync()
    return e


def run(n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    ts = 8 if prec == spe.F64 else 4
    eps = 1e-10 if prec == spe.F64 else 1e-4
    m = min(n, UNIQUE)
    mu, cov = sy.pose_initial(m)
    bad = cr.with_eigenvalues(cov, [-1e-3])
    v = 1e-3 * np.einsum("bii->bi", cov).min(axis=0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    label = f"pose {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    engines, calls, first = {}, {}, {}
    for name, every in BATCHES:
        e = build(n, prec, every, mu, cov, bad)
        vd = torch.from_numpy(v).to("cuda", tdt)
        st = torch.empty((n,), dtype=torch.int32, device="cuda")
        lo, hi = torch.empty((n,), dtype=tdt, device="cuda"), torch.empty((n,), dtype=tdt, device="cuda")
        cov_bytes = n * e.PK * ts
        cov_ptr = e.device_views()[1]
        keep = torch.empty((cov_bytes + 7) // 8, dtype=torch.int64, device="cuda")
        assert HIP.hipMemcpyAsync(C.c_void_p(keep.data_ptr()), C.c_void_p(cov_ptr), C.c_size_t(cov_bytes), 3, stream) == 0
        torch.cuda.synchronize()

        def restore(cov_ptr=cov_ptr, keep=keep, cov_bytes=cov_bytes):
            assert HIP.hipMemcpyAsync(C.c_void_p(cov_ptr), C.c_void_p(keep.data_ptr()), C.c_size_t(cov_bytes), 3, stream) == 0

        def commit(e=e, vd=vd, st=st, every=every, restore=restore):
            if every:
                restore()
            e.condition_dev(vd, eps, status=st)

        def dry(e=e, vd=vd, st=st, lo=lo, hi=hi):
            e.condition_dev(vd, eps, commit=False, eig_min=lo, eig_max=hi, status=st)
        dry()
        e.sync()
        first[name] = (int((st == ST_REPAIRED).sum()), int(((st != 0) & (st != ST_REPAIRED)).sum()))
        engines[name] = (e, vd, st, lo, hi, keep)
        calls[f"{name}: condition c=1"] = commit
        calls[f"{name}: condition c=0"] = dry
        if name == "deficient":
            calls["restore"] = restore
    # the yardsticks
    eh = build(n, prec, 0, mu, cov, bad)
    state_bytes = n * (eh.S + eh.PK) * ts
    src = torch.zeros((state_bytes + 7) // 8, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)

    def state_copy():
        assert HIP.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(state_bytes), 3, stream) == 0
    reps = (n + m - 1) // m
    _, z, Q = sy.pose_cycle_inputs(m, 0, mu[:, :3])
    tile = lambda x: np.tile(x, (reps,) + (1,) * (x.ndim - 1))[:n]   # noqa: E731
    zd = torch.from_numpy(tile(z)).to("cuda", tdt).contiguous()
    Qd = torch.from_numpy(tile(Q).reshape(n, 9)).to("cuda", tdt).contiguous()
    calls["state copy"] = state_copy
    calls["update"] = lambda: eh.update_dev(spe.MEAS_POS3, zd, Qd)
    any_e = eh

    def timed(fn):
        any_e.timer_begin()   # (every engine runs on torch's current stream: one engine's events time them all)
        for _ in range(CALLS):
            fn()
        return any_e.timer_end() / CALLS
    for fn in calls.values():   # warm-up
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(REPS):
        for name, fn in calls.items():   # interleaved
            ms[name].append(timed(fn))
    med = {name: float(np.median(t)) for name, t in ms.items()}
    for name, t in ms.items():
        print(f"{label:28s} {name:32s} {med[name]:9.4f} ms  (min {min(t):.4f} max {max(t):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filters/s  = x{med[name] / med['update']:.2f} update = x{med[name] / med['state copy']:.2f} state copy", flush=True)
    print(f"{label:28s} state {state_bytes / n:.0f} B per filter: the copy moves it at {2 * state_bytes / med['state copy'] / 1e6:.0f} GB/s (read + write); "
          f"restore = the packed covariances, {n * eh.PK * ts / n:.0f} B per filter", flush=True)
    print(f"{label:28s} (REPAIRED, other non-zero) statuses of the first read-only call: {first}; eps = {eps:g}; "
          f"healthy engine's status summary after the updates: {eh.status_summary()}", flush=True)
    for e, *_ in engines.values():
        e.close()
    eh.close()


if __name__ == "__main__":
    print(f"# interleaved, medians of {REPS} repetitions of {CALLS} calls each, HIP-event timing on the engines' (torch's) stream", flush=True)
    run(FILTERS, spe.F64)
    run(FILTERS, spe.F32)
