"""Rate of the filter-lifecycle calls (ukfb_gather_filters_dev, ukfb_scatter_filters_dev, ukfb_compact_dev) on Pose engines,
each beside a device-to-device hipMemcpyAsync of the SAME number of bytes on the same stream -- the yardstick, not the code under
test -- interleaved so that all see the same clocks.

  gather / scatter   random distinct indices, a quarter of the filters; a record is mean, packed covariance, last measurement
                     time, flag and both latches (no noise: the engine's is batch-uniform); the gather also with mean and
                     covariance alone, which tells the cost of the four small arrays
  compact            10 % and 50 % of the filters dead at random; the whole call (count, scan, rank, move); its bytes are those of
                     the records it moves, status word included; the engine is fragmented again before every timed call
  fused cycle        ukfb_cycle_dev on the 50 %-dead engine before and after the compaction

Reported: median ms per call with the spread, records/s, GB/s counting every byte once read and once written (for the copy too),
and the ratio of the call's rate to the copy's.  A mover below half the copy's rate is a finding to explain.

    python tools/lifecycle_rate.py [repetitions=7] [filters=1048576] > profiles/lifecycle_rate.txt
"""
import torch  # noqa: F401
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import slam_pose_estimation_amd as spe

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
FILTERS = int(sys.argv[2]) if len(sys.argv) > 2 else 1048576
UNIQUE = 65536   # filters synthesised; the population is tiled from them (a timing run)
HIP = C.CDLL("libamdhip64.so")


def build(n, prec):
    sy = spe.synth
    m = min(n, UNIQUE)
    reps = (n + m - 1) // m
    e = spe.BatchPoseUKF(n, precision=prec, stream="torch")
    mu, cov = sy.pose_initial(m)
    acc, z, Q = sy.pose_cycle_inputs(m, 0, mu[:, :3])
    tile = lambda x: np.tile(x, (reps,) + (1,) * (x.ndim - 1))[:n]
    for lo in range(0, n, m):   # chunked: the full covariances of a million filters are 1.2 GB of doubles
        k = min(m, n - lo)
        e.initialize(mu[:k], cov[:k], first=lo)
    e.set_acceleration(tile(acc), 0.01 * np.eye(3))
    e.set_last_measurement_time(1_000_000 + np.arange(n, dtype=np.int64))
    e.sync()
    return e, tile(z), tile(Q)


def timed(e, fn):
    e.timer_begin()
    fn()
    return e.timer_end()


def copy_fn(nbytes, tdt):
    src = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        assert HIP.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(nbytes), 3, stream) == 0
    return fn


def run(n, prec):
    e, z, Q = build(n, prec)
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    ts = 8 if prec == spe.F64 else 4
    rec_bytes = (e.S + e.PK + 6) * ts + 8 + 1
    rng = np.random.default_rng(5)
    label = f"pose {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"

    def records(m):
        return dict(mu=torch.empty((m, e.S), dtype=tdt, device="cuda"), cov_packed=torch.empty((m, e.PK), dtype=tdt, device="cuda"),
                    last_ts_us=torch.empty((m,), dtype=torch.int64, device="cuda"), initialised=torch.empty((m,), dtype=torch.uint8, device="cuda"),
                    in_a=torch.empty((m, 3), dtype=tdt, device="cuda"), in_b=torch.empty((m, 3), dtype=tdt, device="cuda"))

    # everything, to fragment the engine again before a timed compact
    everything = records(n)
    e.gather_filters_dev(None, **everything)
    q = n // 4
    index = torch.from_numpy(rng.choice(n, size=q, replace=False).astype(np.int32)).to("cuda")
    part = records(q)
    status = torch.empty((q,), dtype=torch.int32, device="cuda")
    e.gather_filters_dev(index, **part)
    flags = {}
    for pct in (10, 50):
        flags[pct] = torch.from_numpy((rng.random(n) >= pct / 100.0).astype(np.uint8)).to("cuda")
    live = torch.zeros((1,), dtype=torch.int64, device="cuda")
    new_index = torch.empty((n,), dtype=torch.int32, device="cuda")
    old_index = torch.empty((n,), dtype=torch.int32, device="cuda")

    def fragment(pct):
        e.scatter_filters_dev(None, **{**everything, "initialised": flags[pct]})

    moved = {}
    for pct in (10, 50):   # how many records a compact moves: the yardstick's bytes
        fragment(pct)
        e.compact_dev(1, new_index, old_index, live)
        e.sync()
        ni = new_index.cpu().numpy()
        moved[pct] = int(((ni >= 0) & (ni != np.arange(n))).sum())
    calls = {
        "gather 25 %": (q, rec_bytes, None, lambda: e.gather_filters_dev(index, **part)),
        "gather 25 % mu+cov": (q, (e.S + e.PK) * ts, None, lambda: e.gather_filters_dev(index, mu=part["mu"], cov_packed=part["cov_packed"])),
        "scatter 25 %": (q, rec_bytes, None, lambda: e.scatter_filters_dev(index, status=status, **part)),
        "compact 10 % dead": (moved[10], rec_bytes + 4, lambda: fragment(10), lambda: e.compact_dev(1, new_index, old_index, live)),
        "compact 50 % dead": (moved[50], rec_bytes + 4, lambda: fragment(50), lambda: e.compact_dev(1, new_index, old_index, live)),
    }
    copies = {name: copy_fn(c[0] * c[1], tdt) for name, c in calls.items()}
    ms = {name: [] for name in calls}
    ms_copy = {name: [] for name in calls}
    for _ in range(REPS + 1):   # the first round warms up
        for name, (_, _, prepare, fn) in calls.items():   # interleaved
            if prepare:
                prepare()
            ms[name].append(timed(e, fn))
            ms_copy[name].append(timed(e, copies[name]))
    for name, (m, rb, _, _) in calls.items():
        v, c = ms[name][1:], ms_copy[name][1:]
        med, medc = float(np.median(v)), float(np.median(c))
        print(f"{label:28s} {name:19s} {med:8.4f} ms (min {min(v):.4f} max {max(v):.4f})  {m / med / 1e3:8.1f} M records/s "
              f"{2 * m * rb / med / 1e6:7.1f} GB/s | copy of {m * rb / 1e6:7.1f} MB {medc:8.4f} ms {2 * m * rb / medc / 1e6:7.1f} GB/s | "
              f"rate = x{medc / med:.2f} copy")
    # the fused cycle on the 50 %-dead engine, before and after the compaction
    zt = torch.from_numpy(z).to("cuda", tdt)
    Qt = torch.from_numpy(Q).to("cuda", tdt)
    cyc = {}
    for state in ("fragmented", "compacted"):
        cyc[state] = []
        for _ in range(REPS + 1):
            fragment(50)
            if state == "compacted":
                e.compact_dev(1, None, None, live)
            cyc[state].append(timed(e, lambda: e.cycle_dev(0.01, spe.MEAS_POS3, zt, Qt)))
    n_live = int(flags[50].sum().item())
    for state, v in cyc.items():
        med = float(np.median(v[1:]))
        print(f"{label:28s} fused cycle, 50 % dead, {state:10s} {med:8.4f} ms (min {min(v[1:]):.4f} max {max(v[1:]):.4f})  "
              f"{n_live / med / 1e3:8.1f} M live filters/s  kernel={e.last_launch_info()['kernel']}")
    print(f"{label:28s} live after compaction: {int(live.item())} of {n}")
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, {REPS} repetitions after one warm-up round, one call per timing, HIP-event timing on the engine's stream")
    run(FILTERS, spe.F64)
    run(FILTERS, spe.F32)
