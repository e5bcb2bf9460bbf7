"""Per-call cost of the Python binding (profiles/binding_call_overhead.txt).

  --cpu   the marshalling alone, no GPU: raw calls of ukfb_cycle_dev and ukfb_cycle_multi_dev with a NULL engine (they return
          at the argument check), once with explicit C.c_* boxes on a handle without argtypes and once with bare values on the
          declared library; repetitions interleaved, median and min-max in ns per call.
  --gpu   the launch-bound case, one repetition per process: a Pose fp32 engine of 4 096 filters on a private stream, 2 000
          cycle_dev calls, then sync; wall-clock per call.  Uses only the public binding, so it runs on any revision.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def cpu(calls: int, reps: int):
    import slam_pose_estimation_amd as spe
    typed = spe.load_library()
    if not typed.ukfb_cycle_dev.argtypes:
        raise SystemExit("the loaded library carries no argtypes: nothing to compare")
    boxed = C.CDLL(spe.engine.LIB_PATH)   # the same library, its functions undeclared
    null, z, Q, dt = C.c_void_p(), 0x7f0000001000, 0x7f0000002000, 0.01
    spellings = {
        ("ukfb_cycle_dev", "boxes"): lambda f=boxed.ukfb_cycle_dev: f(null, C.c_double(dt), C.c_int(0), None, C.c_void_p(z), C.c_void_p(Q)),
        ("ukfb_cycle_dev", "argtypes"): lambda f=typed.ukfb_cycle_dev: f(null, dt, 0, None, z, Q),
        ("ukfb_cycle_multi_dev", "boxes"): lambda f=boxed.ukfb_cycle_multi_dev: f(
            null, C.c_int(8), C.c_double(dt), C.c_int(0), C.c_int(8), C.c_int(0), None, None, C.c_void_p(z), C.c_void_p(Q)),
        ("ukfb_cycle_multi_dev", "argtypes"): lambda f=typed.ukfb_cycle_multi_dev: f(null, 8, dt, 0, 8, 0, None, None, z, Q),
    }
    ns = {k: [] for k in spellings}
    for call in spellings.values():
        assert call() != 0   # refused at the argument check: nothing is launched
    for _ in range(reps):
        for key, call in spellings.items():
            t0 = time.perf_counter_ns()
            for _ in range(calls):
                call()
            ns[key].append((time.perf_counter_ns() - t0) / calls)
    for (fn, spelling), v in ns.items():
        print(f"{fn:22s} {spelling:9s} median {statistics.median(v):7.1f} ns/call  min {min(v):7.1f}  max {max(v):7.1f}  "
              f"({reps} x {calls} calls)")


def gpu(calls: int):
    import numpy as np
    import torch
    import slam_pose_estimation_amd as spe
    n = 4096
    mu, cov = spe.synth.pose_initial(n)
    acc, z, Q = spe.synth.pose_cycle_inputs(n, 0, mu[:, :3])
    eng = spe.BatchPoseUKF(n, precision=spe.F32, device=0, stream="private")
    eng.initialize(mu, cov)
    eng.set_acceleration(acc, 0.01 * np.eye(3))
    zd = torch.tensor(z, dtype=torch.float32, device="cuda")
    Qd = torch.tensor(Q.reshape(n, 9), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(200):
        eng.cycle_dev(0.01, spe.MEAS_POS3, zd, Qd)
    eng.sync()
    t0 = time.perf_counter_ns()
    for _ in range(calls):
        eng.cycle_dev(0.01, spe.MEAS_POS3, zd, Qd)
    eng.sync()
    per_call = (time.perf_counter_ns() - t0) / calls
    print(f"cycle_dev pose f32 n={n} private stream: {per_call / 1000:.3f} us/call over {calls} calls, then sync "
          f"(status summary {eng.status_summary():#x})")
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--cpu", action="store_true")
    mode.add_argument("--gpu", action="store_true")
    ap.add_argument("--calls", type=int, default=0, help="default: 200 000 with --cpu, 2 000 with --gpu")
    ap.add_argument("--reps", type=int, default=7, help="--cpu: repetitions of every spelling")
    a = ap.parse_args()
    if a.cpu:
        cpu(a.calls or 200_000, a.reps)
    else:
        gpu(a.calls or 2_000)
