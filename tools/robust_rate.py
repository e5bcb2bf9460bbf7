"""Rate of the robust sensor-frame update (ukfb_update_robust_dev, POSE_POINT) beside the sensor-frame landmark fix
(ukfb_update_sensor_dev, POSE_POINT) on the same engine and the update-only launch (ukfb_update_dev with POS3) on a twin of the
same capacity, interleaved so that all see the same clocks.  One batch of Pose filters (synth.pose_initial, landmarks 15 ... 80 m
away), four sets of samples, each at a constructed Mahalanobis radius rho of the filter's own S (z = z-bar + Ls u rho, z-bar
and S from a read-only sensor call on the device): every sample an inlier (rho = 0.5), 10 % outliers at rho = 8, every sample
an outlier at rho = 8 in MATCH, and the same in HUBER.  c^2 = 7.8147, tol 1e-13 (fp64) / 2e-6 (fp32), max_iter 16, no clamp.
Reported: median ms per call over the repetitions, their spread, filter-updates/s, the ratio to the sensor POINT update and to
the update-only launch, and the mean Newton trips per filter (the kernel's own `iterations` output).

Every robust and sensor call runs with commit = 0: every step still runs, only the stores of the state are left out, and the
batch -- with it the trips -- stays what it was from call to call.

    python tools/robust_rate.py [repetitions=5] [calls per repetition=10] [pose filters=1048576] > profiles/robust_rate.txt
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import slam_pose_estimation_amd as spe
import sensor_meas_reference as sr

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
POSE_FILTERS = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
CHI2 = 7.8147

EXPECTED = """# EXPECTED (written before the first run): a trip of the lambda loop is one 3 x 3 factorisation, two triangular solves and a
# quadratic form on scalars the row already holds -- some 80 fp operations per lane, no LDS, no reduction -- beside a call of
# about 2 ms that is bound by its state traffic and its two 12 x 12 factorisations.  So: an all-inlier batch within a few
# percent of the sensor call (it adds one evaluation at lambda = 1 and three stores per filter), and every trip well under 1 %
# of it.  No threshold to pass: the sensor call on the same engine in the same run is the yardstick."""


def initial(engines, n, chunk=262144):
    mus = []
    for lo in range(0, n, chunk):
        mu, cov = spe.synth.pose_initial(min(chunk, n - lo), first=lo)
        for e in engines:
            e.initialize(mu, cov, first=lo)
        mus.append(mu)
    return np.concatenate(mus)


def timed(e, fn):
    e.timer_begin()
    for _ in range(CALLS):
        fn()
    return e.timer_end() / CALLS


def run(n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    e = spe.BatchPoseUKF(n, precision=prec, stream="private")
    twin = spe.BatchPoseUKF(n, precision=prec, stream="private")
    for x in (e, twin):
        x.set_process_noise(sy.pose_default_process_noise())
    mu = initial((e, twin), n)
    rng = np.random.default_rng(5)
    mount = np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)), sr.on.so3_exp(rng.uniform(-1.0, 1.0, (n, 3)))], axis=1)
    d = rng.standard_normal((n, 3))
    point = mu[:, 0:3] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(15.0, 80.0, (n, 1))
    _, z3, Q3 = sy.pose_cycle_inputs(n, 0, mu[:, :3])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)
    md, pd = dev(mount), dev(point)
    Qs = dev(np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).reshape(n, 9))
    z3d, Q3d = dev(z3), dev(Q3.reshape(n, 9))
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    its = torch.empty((n,), dtype=torch.int32, device="cuda")
    lam = torch.empty((n,), dtype=tdt, device="cuda")
    # z-bar and S of every filter, from the device; then the samples at their radii
    zbar, S = torch.empty((n, 3), dtype=tdt, device="cuda"), torch.empty((n, 9), dtype=tdt, device="cuda")
    e.update_sensor_dev(spe.SENSOR_POSE_POINT, torch.zeros_like(zbar), Qs, mount_dev=md, point_dev=pd, commit=False, z_pred=zbar, S=S, status=st)
    e.sync()
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    Ls = torch.linalg.cholesky(S.double().reshape(n, 3, 3))
    u = torch.from_numpy(rng.standard_normal((n, 3))).to("cuda")
    u = u / u.norm(dim=1, keepdim=True)
    step = torch.einsum("nij,nj->ni", Ls, u)
    tenth = torch.from_numpy(np.arange(n) % 10 == 0).to("cuda")
    at = lambda rho: (zbar.double() + step * rho[:, None]).to(tdt)   # noqa: E731
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    z_in, z_mix, z_out = at(0.5 * ones), at(torch.where(tenth, 8.0 * ones, 0.5 * ones)), at(8.0 * ones)
    tol = 1e-13 if prec == spe.F64 else 2e-6
    match = spe.RobustRule(spe.ROBUST_MATCH, 3.8415, CHI2, 1e30, tol, 16)
    huber = spe.RobustRule(spe.ROBUST_HUBER, 3.8415, CHI2, 1e30, tol, 16)
    robust = lambda z, rule: (lambda: e.update_robust_dev(spe.SENSOR_POSE_POINT, z, Qs, rule, mount_dev=md, point_dev=pd, commit=False,   # noqa: E731
                                                          scale=lam, iterations=its, status=st))
    calls = {
        "robust all inliers": (e, robust(z_in, match)),
        "robust 10% rho=8": (e, robust(z_mix, match)),
        "robust all rho=8 MATCH": (e, robust(z_out, match)),
        "robust all rho=8 HUBER": (e, robust(z_out, huber)),
        "sensor POINT": (e, lambda: e.update_sensor_dev(spe.SENSOR_POSE_POINT, z_in, Qs, mount_dev=md, point_dev=pd, commit=False, status=st)),
        "update POS3": (twin, lambda: twin.update_dev(spe.MEAS_POS3, z3d, Q3d)),
    }
    label = f"pose {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    for name, (eng, fn) in calls.items():
        fn()
        eng.sync()
        torch.cuda.synchronize()
        if name.startswith("robust"):
            print(f"{label:28s} {name:24s} mean trips per filter {its.double().mean().item():.4f} (max {int(its.max())}); "
                  f"inflated {int((lam > 1).sum())}; mean lambda of those {lam[lam > 1].double().mean().item() if (lam > 1).any() else 1.0:.3f}; "
                  f"non-zero status {int((st != 0).sum())}", flush=True)
    ms = {name: [] for name in calls}
    for _ in range(REPS):
        for name, (eng, fn) in calls.items():   # interleaved
            ms[name].append(timed(eng, fn))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:28s} {name:24s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
              f"  {n / med[name] / 1e3:9.1f} M filter-updates/s  = x{med[name] / med['sensor POINT']:.3f} sensor POINT"
              f"  = x{med[name] / med['update POS3']:.2f} update POS3 launches", flush=True)
    e.close()
    twin.close()


if __name__ == "__main__":
    print(EXPECTED, flush=True)
    print(f"# interleaved, medians of {REPS} repetitions of {CALLS} calls each, HIP-event timing on each engine's stream", flush=True)
    for prec in (spe.F64, spe.F32):
        run(POSE_FILTERS, prec)
