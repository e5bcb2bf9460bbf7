"""Rate of the user-defined measurement models beside the built-in sensor-frame update that computes the same thing
(ukfb_update_sensor_dev with POSE_POINT, the only way to make that update without them), interleaved so that all see the same
clocks:

    export            ukfb_sigma_points_dev (X only)
    sampled m=1/3/6   ukfb_update_sampled_dev, commit = 0, on samples of the initial export (m = 1: the range to the point, m = 3:
                      POSE_POINT's formula, m = 6: p + R(q) r stacked on R(q) v).  commit = 0 because the samples belong to ONE
                      state: every step of the update still runs, only the store of the new state is left out
    sensor POINT c=0  ukfb_update_sensor_dev(POSE_POINT), commit = 0: the like-for-like line for the three above
    torch h m=3       the torch expression of the chain alone (POSE_POINT's formula on the exported X, eager mode)
    chain m=3         export, Z = h(X) as a torch expression (POSE_POINT's formula), ukfb_update_sampled_dev with commit = 1
    sensor POINT      ukfb_update_sensor_dev(POSE_POINT), commit = 1: the like-for-like line for the chain

Reported: median ms per call over the repetitions, their spread, filter-updates/s and the ratio to the committing sensor update.
The engine runs on torch's current stream, so that the torch expression of the chain is ordered with the two calls and is inside
the HIP-event timing.  There is no threshold: the output is the record.

    python tools/sampled_rate.py [repetitions=7] [calls per repetition=10] [pose filters=1048576] > profiles/sampled_rate.txt
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import slam_pose_estimation_amd as spe
import sampled_reference as sm
import sensor_meas_reference as sr

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576


def h_point(X, r, qs, b):
    return sm.rot_t(qs, sm.rot_t(X[..., 3:7], b - X[..., 0:3]) - r)


def run(n, prec, chunk=262144):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    e = spe.BatchPoseUKF(n, precision=prec, stream="torch")
    e.set_process_noise(sy.pose_default_process_noise())
    mus = []
    for lo in range(0, n, chunk):
        mu, cov = sy.pose_initial(min(chunk, n - lo), first=lo)
        e.initialize(mu, cov, first=lo)
        mus.append(mu)
    mu = np.concatenate(mus)
    rng = np.random.default_rng(5)
    mount = np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)), sr.on.so3_exp(rng.uniform(-1.0, 1.0, (n, 3)))], axis=1)
    d = rng.standard_normal((n, 3))
    point = mu[:, 0:3] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(15.0, 80.0, (n, 1))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
    mount_d, point_d = dev(mount), dev(point)
    r, qs, b = mount_d[:, None, 0:3], mount_d[:, None, 3:7], point_d[:, None, :]
    z3 = dev(sr.h(sr.POSE_POINT, mu, mount, point))
    Q3 = dev(np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)))
    X = torch.empty((n, 2 * e.D + 1, e.S), dtype=tdt, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    maha = torch.empty((n,), dtype=tdt, device="cuda")
    e.sigma_points_dev(X, None, st)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    Z = {1: sm._norm((X[..., 0:3] - b) + sm.rot(X[..., 3:7], r)).contiguous(), 3: h_point(X, r, qs, b).contiguous(),
         6: torch.cat([X[..., 0:3] + sm.rot(X[..., 3:7], r), sm.rot(X[..., 3:7], X[..., 7:10])], dim=-1).contiguous()}
    z = {m: Z[m][:, 0].contiguous() for m in Z}   # the sample is h(mu): a timing run
    Q = {m: dev(0.05 ** 2 * np.eye(m)) for m in Z}

    def chain():
        e.sigma_points_dev(X, None, None)
        e.update_sampled_dev(3, h_point(X, r, qs, b).contiguous(), z3, Q3, status=st)

    calls = {"export": lambda: e.sigma_points_dev(X, None, st)}
    for m in (1, 3, 6):
        calls[f"sampled m={m} c=0"] = lambda m=m: e.update_sampled_dev(m, Z[m], z[m], Q[m], q_is_uniform=True, commit=False, maha=maha, status=st)
    calls["sensor POINT c=0"] = lambda: e.update_sensor_dev(spe.SENSOR_POSE_POINT, z3, Q3, mount_dev=mount_d, point_dev=point_d, commit=False, maha=maha, status=st)
    calls["torch h m=3"] = lambda: h_point(X, r, qs, b).contiguous()
    calls["chain m=3"] = chain
    base = "sensor POINT"
    calls[base] = lambda: e.update_sensor_dev(spe.SENSOR_POSE_POINT, z3, Q3, mount_dev=mount_d, point_dev=point_d, status=st)
    bad = {}
    for name, fn in calls.items():
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
        print(f"{label:28s} {name:18s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filter-updates/s  = x{med[name] / med[base]:.2f} {base} launches", flush=True)
    after = {}
    for name in ("chain m=3", base):   # (a timing run: the same sample is committed some hundred times)
        calls[name]()
        e.sync()
        after[name] = int((st != 0).sum())
    rec = X.element_size() * (2 * e.D + 1) * e.S
    print(f"{label:28s} sigma-point record {rec} B per filter: the export writes it, the torch expression reads it: "
          f"{n * rec / med['export'] / 1e6:.0f} GB/s written by the export", flush=True)
    print(f"{label:28s} filters with a non-zero status in the first call: {bad}; in a call after the timing: {after}", flush=True)
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, medians of {REPS} repetitions of {CALLS} calls each, HIP-event timing on the engine's (torch's) stream", flush=True)
    run(FILTERS, spe.F64)
    run(FILTERS, spe.F32)
