"""Rate of the joint association marginals of a scene (ukfb_jpda_scenes_dev, include/ukf_batch_jpda.h) beside
ukfb_assign_scenes_dev at the same shapes, and of the update with given weights (ukfb_update_weighted_dev) beside
ukfb_update_pda_dev at the same K and the update-only launch.  1 048 576 Pose filters, uniform scenes of (T, K) = (2, 4), (4, 8)
and (6, 32) over the whole engine; loglik = -d^2 / 2 - c with d^2 uniform in [0, 20) and c in [-1, 7), 30 % of the pairs
forbidden (NaN), the gate off; the update on POSE_POINT with weights uniform in (0, 1 / K); interleaved so that all see the
same clocks.  Outputs asked for: beta, beta0, free, log_z and scene_status by the scene call; assign, owner, objective and
scene_status by the assignment; status alone by the updates (and weight_used / beta on the lines that say so).

EXPECTED, written before the first run.  Nobody has measured any of these rates and no target is set.
The scene kernel: one wavefront solves one scene, four scenes share a workgroup, no LDS; 95 VGPRs allow five wavefronts per
SIMD, 20 per CU, 5 120 scenes at a time on 256 CUs.  A wavefront's time is a chain of latencies:
  staging: T loads of loglik along the detections (one cache line each, ~2 us of memory latency in all) and T exponentials:
           ~5 000 cycles;
  a backward step (one detection): the T exchanges of G are independent (two ds_bpermute each, ~100 cycles of latency once),
           then T dependent fp64 fma: ~110 cycles at T = 2, ~160 at T = 6;
  a forward step: per track one product, one six-stage butterfly sum over the wavefront (two ds_bpermute ~70 cycles and one
           fp64 add per stage: ~470 cycles) and one exchange of F; the T sums are independent but taken as serial: T x 470 + 150;
  beta_i0, ln Z and the stores: ~3 000 cycles.
At 2.4 GHz:
  (2, 4):   5 000 + 4 x 110 + 4 x 1 090 + 3 000 =  12 800 cycles =  5.3 us per scene; 524 288 scenes = 102.4 rounds: 0.55 ms
  (4, 8):   5 000 + 8 x 135 + 8 x 2 030 + 3 000 =  25 300 cycles = 10.5 us per scene; 262 144 scenes =  51.2 rounds: 0.54 ms
  (6, 32):  5 000 + 32 x 160 + 32 x 2 970 + 3 000 = 108 200 cycles = 45.1 us per scene; 174 763 scenes =  34.1 rounds: 1.54 ms
The other limit is the cross-lane unit of a CU, which the 20 wavefronts share: K T x 16 + K T x 2 ds_bpermute per scene (3 456
at (6, 32)) at 2 cycles each (64 lanes x 4 B at 128 B per clock) is 6 900 cycles per scene, x 683 scenes per CU = 1.96 ms at
(6, 32), 0.25 ms at (4, 8), 0.06 ms at (2, 4).  Expected: the larger of the two, 0.55 / 0.54 / 1.96 ms, in either precision (the
solve is fp64 in both).  At T = 2 a wavefront uses 4 of its 64 lanes: packing 2^(6 - T) scenes into one wavefront falls out of
the xor layout and is the thing to measure first; it is not done here.
The update with given weights: the PDA update's launch without its exponentials and without a second pass over z: expected at
the association's cost at the same K, 2.09 + 0.11 K ms fp64 / 0.97 + 0.054 K ms fp32, and with weight_used one
load and one store per candidate more, ~0.02 ms per candidate.
Each line reports measured / expected.  Each precision runs in a child process under its own time limit; a child that fails
or overruns ends the run.

    python tools/jpda_rate.py [repetitions=5] [calls per repetition=10] [pose filters=1048576] > profiles/jpda_rate.txt
"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((2, 4), (4, 8), (6, 32))
STEP_LIMIT_S = 240
EXPECT_SCENE_MS = {(2, 4): 0.55, (4, 8): 0.54, (6, 32): 1.96}
EXPECT_UPDATE_MS = {"fp64": (2.09, 0.11), "fp32": (0.97, 0.054)}
WAVES_PER_CU = 20   # 95 VGPRs: five wavefronts per SIMD; no LDS


def run(n, pname, reps, ncalls):
    import numpy as np
    import torch
    import slam_pose_estimation_amd as spe
    import bearing_reference as br
    import pda_reference as pr
    import sensor_meas_reference as sr
    sy = spe.synth
    prec = spe.F64 if pname == "fp64" else spe.F32
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    mus, covs = [], []
    for lo in range(0, n, 262144):
        mu, cov = sy.pose_initial(min(262144, n - lo), first=lo)
        mus.append(mu)
        covs.append(cov)

    def engine():
        e = spe.BatchPoseUKF(n, precision=prec, stream="private", gate_chi2=pr.GATE)
        e.set_process_noise(sy.pose_default_process_noise())
        lo = 0
        for mu, cov in zip(mus, covs):
            e.initialize(mu, cov, first=lo)
            lo += len(mu)
        return e
    e = engine()
    mu = np.concatenate(mus)
    mount, point, _, _ = br.make_inputs(br.on.POSE, mu, 15.0, 80.0, e.dtype)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
    Kmax = max(K for _, K in SHAPES)
    md, pd = dev(mount), dev(point)
    Qd = dev(np.broadcast_to(0.05 ** 2 * np.eye(3), (n, 3, 3)).reshape(n, 9))
    zc = dev(sr.h(sr.POSE_POINT, mu, mount, point))
    gen = torch.Generator(device="cuda").manual_seed(31)
    zs = torch.empty((Kmax, n, 3), dtype=tdt, device="cuda")
    for k in range(Kmax):
        zs[k] = zc + 0.05 * (1 + k % 4) * torch.randn((n, 3), dtype=tdt, device="cuda", generator=gen)
    d2 = 20.0 * torch.rand((Kmax, n), dtype=tdt, device="cuda", generator=gen)
    loglik = -0.5 * d2 - (8.0 * torch.rand((Kmax, n), dtype=tdt, device="cuda", generator=gen) - 1.0)
    forbidden = torch.rand((Kmax, n), device="cuda", generator=gen) < 0.3
    loglik[forbidden] = float("nan")
    cost = d2.clone()
    cost[forbidden] = float("nan")
    new = lambda *shape, t=tdt: torch.empty(shape, dtype=t, device="cuda")   # noqa: E731
    beta, beta0, wused = new(Kmax, n), new(n), new(Kmax, n)
    st, assign = new(n, t=torch.int32), new(n, t=torch.int32)
    rule = spe.PdaRule(*pr.RULE)
    torch.cuda.synchronize()
    P = spe.SENSOR_POSE_POINT
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def timed(fn):
        e.timer_begin()
        for _ in range(ncalls):
            fn()
        return e.timer_end() / ncalls

    def report(label, ms, tails):
        med = {name: float(np.median(v)) for name, v in ms.items()}
        for name, v in ms.items():
            print(f"{label} {name:34s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})  {n / med[name] / 1e3:8.1f} M filters/s"
                  f"{tails(name, med)}", flush=True)

    label = f"pose {pname} {n} filters"
    # ---- the scene call beside the assignment
    for T, K in SHAPES:
        scenes = -(-n // T)
        free, log_z, sstat = new(scenes * K, t=torch.float64), new(scenes, t=torch.float64), new(scenes, t=torch.int32)
        owner, objective = new(scenes * K, t=torch.int32), new(scenes, t=torch.float64)
        calls = {
            "jpda_scenes": lambda: e.jpda_scenes_dev(K, loglik, rule, scenes, tracks_per_scene=T, model=P, beta=beta, beta0=beta0, free=free,
                                                     log_z=log_z, scene_status=sstat),
            "assign_scenes": lambda: e.assign_scenes_dev(K, cost, scenes, tracks_per_scene=T, miss=20.0, assign=assign, owner=owner,
                                                         objective=objective, scene_status=sstat),
        }
        for fn in calls.values():
            fn()
        e.sync()
        ms = {name: [] for name in calls}
        for _ in range(reps):
            for name, fn in calls.items():   # interleaved
                ms[name].append(timed(fn))
        exp = EXPECT_SCENE_MS[T, K]

        def tails(name, med):
            if name != "jpda_scenes":
                return f"  {scenes / med[name] / 1e3:8.2f} M scenes/s"
            return (f"  {scenes / med[name] / 1e3:8.2f} M scenes/s  measured / expected {med[name] / exp:.3f} (expected {exp:.2f} ms)"
                    f"  = x{med[name] / med['assign_scenes']:.3f} the assignment at this shape")
        report(f"{label:28s} T={T:<2d} K={K:<2d}", ms, tails)
        print(f"{label:28s} T={T:<2d} K={K:<2d} scenes={scenes} wavefronts resident at a time: {min(scenes, cus * WAVES_PER_CU)} "
              f"({cus} CUs x {WAVES_PER_CU}: five per SIMD by 95 VGPRs, no LDS), lanes in use per wavefront: {1 << T} of 64", flush=True)
    e.jpda_scenes_dev(4, loglik, rule, -(-n // 2), tracks_per_scene=2, model=P, beta=beta, beta0=beta0)
    e.sync()
    total = float((torch.nan_to_num(beta[:4]).sum(dim=0) + beta0 - 1.0).abs().max())
    print(f"{label:28s} T=2  K=4  max |sum_k beta_ik + beta_i0 - 1| = {total:.2e}", flush=True)
    e.close()
    # ---- the update with given weights beside the PDA update and the update-only launch: committing calls, each on its own engine
    a0, ak = EXPECT_UPDATE_MS[pname]
    _, z3, Q3 = sy.pose_cycle_inputs(n, 0, mu[:, :3])
    z3d, Q3d = dev(z3), dev(Q3.reshape(n, 9))
    names = ("update_weighted", "update_weighted +weight_used", "update_pda", "update_pda +beta", "update_dev (update only)")
    engines = {name: engine() for name in names}   # the state of each moves from call to call
    for _, K in SHAPES:
        w = torch.rand((K, n), dtype=tdt, device="cuda", generator=gen) / K
        kw = dict(mount_dev=md, point_dev=pd, commit=True, status=st)
        calls = {
            names[0]: lambda: engines[names[0]].update_weighted_dev(P, K, zs, Qd, w, **kw),
            names[1]: lambda: engines[names[1]].update_weighted_dev(P, K, zs, Qd, w, weight_used=wused, **kw),
            names[2]: lambda: engines[names[2]].update_pda_dev(P, K, zs, Qd, rule, **kw),
            names[3]: lambda: engines[names[3]].update_pda_dev(P, K, zs, Qd, rule, beta=beta, **kw),
            names[4]: lambda: engines[names[4]].update_dev(spe.MEAS_POS3, z3d, Q3d),
        }

        def timed_on(name):
            eng = engines[name]
            eng.timer_begin()
            for _ in range(ncalls):
                calls[name]()
            return eng.timer_end() / ncalls
        for name in names:
            calls[name]()
            engines[name].sync()
        ms = {name: [] for name in names}
        for _ in range(reps):
            for name in names:   # interleaved
                ms[name].append(timed_on(name))
        exp = a0 + ak * K

        def tails(name, med):
            if not name.startswith("update_weighted"):
                return ""
            e_ms = exp + (0.02 * K if "weight_used" in name else 0.0)
            return (f"  measured / expected {med[name] / e_ms:.3f} (expected {e_ms:.2f} ms)  = x{med[name] / med['update_pda']:.3f} update_pda"
                    f"  = x{med[name] / med['update_dev (update only)']:.2f} the update-only launch")
        report(f"{label:28s} K={K:<2d}     ", ms, tails)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        run(int(sys.argv[3]), sys.argv[2], int(sys.argv[4]), int(sys.argv[5]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ncalls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    filters = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
    print(__doc__[__doc__.index("EXPECTED"):__doc__.index("Each line reports")].rstrip().replace("\n", "\n# ").join(("# ", "")), flush=True)
    print(f"# interleaved, medians of {reps} repetitions of {ncalls} calls each, HIP-event timing on the engine's stream", flush=True)
    for pname in ("fp64", "fp32"):   # a fresh child per precision, each under its own time limit; the first failure ends the run
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", pname, str(filters), str(reps), str(ncalls)],
                                timeout=STEP_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"# {pname}: the child ended with status {rc}; nothing more is run", flush=True)
            sys.exit(rc)
