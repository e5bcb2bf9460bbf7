"""Rate of the assignment across the filters of a scene (ukfb_assign_scenes_dev, include/ukf_batch_assign.h) beside the calls
around it in a tracker's association step: ukfb_associate_sensor_dev (shared-h, POSE_POINT, commit = 0) at the same K, which
writes the costs, and ukfb_select_candidates_dev, which reads the assignment.  Uniform scenes of (T, K) = (4, 4), (8, 8) and
(32, 32) tracks and detections over the whole engine, costs uniform in [0, 64) with 30 % of the pairs forbidden (NaN), the gate
off, miss = 20 for every track; interleaved so that all see the same clocks.  Outputs asked for: assign, owner, objective and
scene_status by the assignment; maha, best and status by the association.

EXPECTED, written before the first run.  One wavefront solves one scene, four scenes share a workgroup and 33 792 B of LDS, so
a CU holds 16 wavefronts and the 256 CUs 4 096 scenes at a time.  A wavefront's time is a chain of latencies, not of issue
slots: a Dijkstra step is one LDS read (~100 cycles), a handful of fp64 operations, a six-stage butterfly minimum of two
ds_bpermute each (~70 cycles a stage) and two v_readlane: ~600 cycles; a sweep adds ~300 cycles of dual update and walk back;
staging costs ~500 cycles per pair of candidates, the results and the tree sum ~1 500.  With 30 % forbidden pairs a sweep is
expected to take ~1.5 steps at T = 4, ~2 at T = 8 and ~4 at T = 32 (the worst case is T steps).  At 2.4 GHz:
  (4, 4):    4 (1.5 x 600 + 300) + 1 000 + 1 500 =  7 300 cycles =  3.0 us per scene; 262 144 scenes = 64 rounds: 0.19 ms
  (8, 8):    8 (2 x 600 + 300) + 2 000 + 1 500   = 15 500 cycles =  6.5 us per scene; 131 072 scenes = 32 rounds: 0.21 ms
  (32, 32): 32 (4 x 600 + 300) + 8 000 + 1 500   = 95 900 cycles = 40.0 us per scene;  32 768 scenes =  8 rounds: 0.32 ms
in either precision (the solve is fp64 in both; the cost block is 32 MB ... 256 MB in fp64, read once at some TB/s: below
0.1 ms and under the solve of other wavefronts).  The association beside it costs 2.09 + 0.11 K ms fp64 / 0.97 + 0.054 K ms
fp32, so the solve is expected at a tenth of the launch that feeds it.  No ratio is a requirement.
Each line reports measured / expected.  Each precision runs in a child process under its own time limit; a child that fails
or overruns ends the run.

    python tools/assign_rate.py [repetitions=5] [calls per repetition=10] [pose filters=1048576] > profiles/assign_rate.txt
"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((4, 4), (8, 8), (32, 32))
STEP_LIMIT_S = 240
EXPECT_MS = {(4, 4): 0.19, (8, 8): 0.21, (32, 32): 0.32}


def run(n, pname, reps, ncalls):
    import numpy as np
    import torch
    import slam_pose_estimation_amd as spe
    import bearing_reference as br
    import sensor_meas_reference as sr
    sy = spe.synth
    prec = spe.F64 if pname == "fp64" else spe.F32
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    e = spe.BatchPoseUKF(n, precision=prec, stream="private")   # every call here is read-only
    e.set_process_noise(sy.pose_default_process_noise())
    mus = []
    for lo in range(0, n, 262144):
        mu, cov = sy.pose_initial(min(262144, n - lo), first=lo)
        e.initialize(mu, cov, first=lo)
        mus.append(mu)
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
    cost = 64.0 * torch.rand((Kmax, n), dtype=tdt, device="cuda", generator=gen)
    cost[torch.rand((Kmax, n), device="cuda", generator=gen) < 0.3] = float("nan")
    new = lambda *shape, t=tdt: torch.empty(shape, dtype=t, device="cuda")   # noqa: E731
    maha, z_sel = new(Kmax, n), new(n, 3)
    best, st, m_sel, assign = (new(n, t=torch.int32) for _ in range(4))
    torch.cuda.synchronize()
    P = spe.SENSOR_POSE_POINT

    def timed(fn):
        e.timer_begin()
        for _ in range(ncalls):
            fn()
        return e.timer_end() / ncalls

    label = f"pose {pname} {n} filters"
    for T, K in SHAPES:
        scenes = -(-n // T)
        owner, objective, sstat = new(scenes * K, t=torch.int32), new(scenes, t=torch.float64), new(scenes, t=torch.int32)
        calls = {
            "assign": lambda: e.assign_scenes_dev(K, cost, scenes, tracks_per_scene=T, miss=20.0, assign=assign, owner=owner,
                                                  objective=objective, scene_status=sstat),
            "associate commit=0": lambda: e.associate_sensor_dev(P, K, zs, Qd, mount_dev=md, point_dev=pd, commit=False, maha=maha, best=best,
                                                                 status=st),
            "select": lambda: e.select_candidates_dev(K, assign, spe.MEAS_POS3, zs, z_sel, m_sel),
        }
        for fn in calls.values():
            fn()
        e.sync()
        taken = int((assign >= 0).sum())
        bad = int((sstat != 0).sum())
        ms = {name: [] for name in calls}
        for _ in range(reps):
            for name, fn in calls.items():   # interleaved
                ms[name].append(timed(fn))
        med = {name: float(np.median(v)) for name, v in ms.items()}
        for name, v in ms.items():
            tail = ""
            if name == "assign":
                exp = EXPECT_MS[T, K]
                tail = (f"  {scenes / med[name] / 1e3:8.2f} M scenes/s  measured / expected {med[name] / exp:.3f} (expected {exp:.2f} ms)"
                        f"  = x{med[name] / med['associate commit=0']:.3f} the association at this K")
            print(f"{label:28s} T={T:<2d} K={K:<2d} {name:20s} {med[name]:9.4f} ms  (min {min(v):.4f} max {max(v):.4f})"
                  f"  {n / med[name] / 1e3:8.1f} M filters/s{tail}", flush=True)
        print(f"{label:28s} T={T:<2d} K={K:<2d} scenes={scenes} tracks with a detection={taken} scenes refused={bad}", flush=True)
    e.close()


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
