"""Rate of the probabilistic data association update (ukfb_update_pda_dev, POSE_POINT) beside the calls it is built on and
replaces: ukfb_associate_sensor_dev (shared-h, the same K), one ukfb_update_sensor_dev, and the update-only launch
(ukfb_update_dev with POS3) on a twin of the same capacity as the yardstick of the other rate files.  K = 1, 4, 16 candidates,
commit = 0 and commit = 1, with and without the beta output (without it the kernel skips its second pass over the candidates),
interleaved so that all see the same clocks.

Pose filters from synth.pose_initial, landmarks 15 ... 80 m away, K detections around the one landmark's (the batch of
tools/associate_rate.py, shared-h mode), the gate off: every candidate is inside and enters the sums.  The read-only calls run
on one engine, whose state never changes; every committing call runs on a second engine, whose state moves from call to call
(the arithmetic of a call does not depend on it).  Outputs asked for: maha, loglik, beta, beta0, innov_comb, best, n_gated and
status by the PDA call; maha, loglik, best, n_gated and status by the association; maha, loglik and status by the sensor call.

EXPECTED, written before the first run, from the per-candidate increments measured for the shared-h association (DESIGN.md
4.26: 0.11 ms fp64 / 0.054 ms fp32 per candidate on 1 048 576 filters over a base of 2.09 ms / 0.97 ms; the loop is bound by
its serial chain load -> solve -> store, not by bytes):
  * first pass: the association's candidate, plus one exponential and 26 fma of running sums: 1.3 increments;
  * second pass (beta wanted): load z, the solve, one exponential, one store: 1.0 increment;
  * after the loop: one logarithm, one exponential, one division, ~60 fma: 0.03 ms fp64 / 0.015 ms fp32.
  PDA(K) with beta    = 2.12 + 0.25 K ms fp64:  K = 1: 2.37   K = 4: 3.12   K = 16: 6.12
                      = 0.98 + 0.124 K ms fp32: K = 1: 1.11   K = 4: 1.48   K = 16: 2.97
  PDA(K) without beta = 2.12 + 0.143 K ms fp64: K = 1: 2.26   K = 4: 2.69   K = 16: 4.41
                      = 0.98 + 0.070 K ms fp32: K = 1: 1.05   K = 4: 1.26   K = 16: 2.10
  commit = 1 adds the state's stores: + 0.05 ms fp64 / + 0.02 ms fp32, as for the association.
Each line reports measured / expected beside the ratios.  Each precision runs in a child process under its own time limit; a
child that fails or overruns ends the run.

    python tools/pda_rate.py [repetitions=5] [calls per repetition=10] [pose filters=1048576] > profiles/pda_rate.txt
"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (1, 4, 16)
STEP_LIMIT_S = 240
EXPECT = {"fp64": {True: (2.12, 0.25), False: (2.12, 0.143), "commit": 0.05}, "fp32": {True: (0.98, 0.124), False: (0.98, 0.070), "commit": 0.02}}


def expected(pname, K, beta, commit):
    base, per = EXPECT[pname][beta]
    return base + per * K + (EXPECT[pname]["commit"] if commit else 0.0)


def run(n, pname, reps, ncalls):
    import numpy as np
    import torch
    import slam_pose_estimation_amd as spe
    import bearing_reference as br
    import sensor_meas_reference as sr
    sy = spe.synth
    prec = spe.F64 if pname == "fp64" else spe.F32
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    ro = spe.BatchPoseUKF(n, precision=prec, stream="private")     # read-only calls
    rw = spe.BatchPoseUKF(n, precision=prec, stream="private")     # committing calls
    twin = spe.BatchPoseUKF(n, precision=prec, stream="private")   # the update-only launch
    mus = []
    for x in (ro, rw, twin):
        x.set_process_noise(sy.pose_default_process_noise())
    for lo in range(0, n, 262144):
        mu, cov = sy.pose_initial(min(262144, n - lo), first=lo)
        for e in (ro, rw, twin):
            e.initialize(mu, cov, first=lo)
        mus.append(mu)
    mu = np.concatenate(mus)
    mount, point, _, _ = br.make_inputs(br.on.POSE, mu, 15.0, 80.0, ro.dtype)
    rng = np.random.default_rng(31)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
    Kmax = max(KS)
    md, pd = dev(mount), dev(point)
    Qd = dev(np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).reshape(n, 9))
    zs = torch.empty((Kmax, n, 3), dtype=tdt, device="cuda")
    zc = sr.h(sr.POSE_POINT, mu, mount, point)
    for k in range(Kmax):
        zs[k] = dev(zc + 0.05 * (1 + k) * rng.standard_normal((n, 3)))
    _, z3, Q3 = sy.pose_cycle_inputs(n, 0, mu[:, :3])
    z3d, Q3d = dev(z3), dev(Q3.reshape(n, 9))
    new = lambda *shape, t=tdt: torch.empty(shape, dtype=t, device="cuda")   # noqa: E731
    maha, ll, beta, beta0, comb = new(Kmax, n), new(Kmax, n), new(Kmax, n), new(n), new(n, 3)
    best, ng, st = new(n, t=torch.int32), new(n, t=torch.int32), new(n, t=torch.int32)
    torch.cuda.synchronize()
    P = spe.SENSOR_POSE_POINT
    rule = spe.PdaRule(0.9, 0.9989, 0.9989, 2.0, 300.0)

    def timed(e, fn):
        e.timer_begin()
        for _ in range(ncalls):
            fn()
        return e.timer_end() / ncalls

    def pda(e, K, commit, with_beta):
        e.update_pda_dev(P, K, zs, Qd, rule, mount_dev=md, point_dev=pd, commit=commit, maha=maha, loglik=ll,
                         beta=beta if with_beta else None, beta0=beta0, innov_comb=comb, best=best, n_gated=ng, status=st)

    def associate(e, K, commit):
        e.associate_sensor_dev(P, K, zs, Qd, mount_dev=md, point_dev=pd, commit=commit, maha=maha, loglik=ll, best=best, n_gated=ng, status=st)

    label = f"pose {pname} {n} filters"
    for K in KS:
        calls = {}
        for commit in (False, True):
            e = rw if commit else ro
            calls[f"pda commit={int(commit)}"] = (e, lambda e=e, c=commit: pda(e, K, c, True), expected(pname, K, True, commit))
            calls[f"pda commit={int(commit)} no beta"] = (e, lambda e=e, c=commit: pda(e, K, c, False), expected(pname, K, False, commit))
            calls[f"associate commit={int(commit)}"] = (e, lambda e=e, c=commit: associate(e, K, c), None)
        calls["sensor call commit=0"] = (ro, lambda: ro.update_sensor_dev(P, zs[0], Qd, mount_dev=md, point_dev=pd, commit=False, maha=maha[0],
                                                                           loglik=ll[0], status=st), None)
        calls["update POS3"] = (twin, lambda: twin.update_dev(spe.MEAS_POS3, z3d, Q3d), None)
        bad = {}
        for name, (eng, fn, _) in calls.items():
            fn()
            eng.sync()
            bad[name] = int((st != 0).sum()) if eng is not twin else int(twin.status_summary() != 0)
        ms = {name: [] for name in calls}
        for _ in range(reps):
            for name, (eng, fn, _) in calls.items():   # interleaved
                ms[name].append(timed(eng, fn))
        med = {name: float(np.median(v)) for name, v in ms.items()}
        for name, v in ms.items():
            exp = calls[name][2]
            commit = "commit=1" in name
            ref = med[f"associate commit={int(commit)}"] + med["sensor call commit=0"]
            tail = f"  measured / expected {med[name] / exp:.3f} (expected {exp:.3f} ms)" if exp else ""
            tail += f"  = x{med[name] / ref:.3f} the association at this K plus one sensor call" if name.startswith("pda") else ""
            print(f"{label:28s} K={K:<2d} {name:26s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
                  f"  {n / med[name] / 1e3:8.1f} M filter-updates/s  = x{med[name] / med['update POS3']:.2f} update POS3 launches{tail}", flush=True)
        print(f"{label:28s} K={K:<2d} filters with a non-zero status in the first call: {bad}", flush=True)
    ro.close(); rw.close(); twin.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        run(int(sys.argv[3]), sys.argv[2], int(sys.argv[4]), int(sys.argv[5]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ncalls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    filters = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
    print(__doc__[__doc__.index("EXPECTED"):__doc__.index("Each line reports")].rstrip().replace("\n", "\n# ").join(("# ", "")), flush=True)
    print(f"# interleaved, medians of {reps} repetitions of {ncalls} calls each, HIP-event timing on each engine's stream", flush=True)
    for pname in ("fp64", "fp32"):   # a fresh child per precision, each under its own time limit; the first failure ends the run
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", pname, str(filters), str(reps), str(ncalls)],
                                timeout=STEP_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"# {pname}: the child ended with status {rc}; nothing more is run", flush=True)
            sys.exit(rc)
