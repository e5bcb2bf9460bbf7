"""Rate of the filter-bank launches (ukfb_bank_mix_dev, ukfb_bank_combine_dev) at M = 2, 4, 8 hypotheses per track, beside the
update-only launch (ukfb_update_dev) of the same engine over the same capacity, interleaved A/B/A/B so that all see the same
clocks.  Reported: median ms per launch, the spread (min ... max) over the repetitions, filters/s and the ratio to the update
launch.  The hypotheses of a track are one synthetic state perturbed by about its own sigma (rotations spread by up to 0.33 rad);
the transition matrix is 0.999 I + 0.001 / M, so that the repeated mixing of a timing run barely moves the hypotheses together
(the instruction count of a launch depends on its data only through the trips of the mean iteration).

    python tools/bank_rate.py [repetitions=7] [launches per repetition=20]
"""
import torch  # noqa: F401
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import slam_pose_estimation_amd as spe

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
LAUNCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 20
CHUNK = 262144
GROUP = 8   # the states are built for tracks of 8 and read as 2, 4 or 8 hypotheses


def quat_mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def quat_exp(v):
    """unit quaternion (x, y, z, w) of the rotation vector v"""
    th = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.concatenate([0.5 * np.sinc(0.5 * th / np.pi) * v, np.cos(0.5 * th)], axis=-1)


def build(kind, n, prec):
    sy = spe.synth
    tdt = torch.float64 if prec == spe.F64 else torch.float32
    if kind == "pose":
        e = spe.BatchPoseUKF(n, precision=prec, stream="private")
        e.set_process_noise(sy.pose_default_process_noise())
        q0, vec = 3, [0, 1, 2, 7, 8, 9, 10, 11, 12]
    else:
        e = spe.BatchOrientationUKF(n, sy.ORIENT_TAU, sy.ORIENT_TAU, sy.ORIENT_LATITUDE, precision=prec, stream="private")
        e.set_process_noise(sy.orient_process_noise())
        q0, vec = 0, list(range(4, 14))
    tan = [i for i in range(e.D) if not (q0 <= i < q0 + 3)]
    z = torch.empty((n, 3), dtype=tdt, device="cuda")
    Q = torch.empty((n, 9), dtype=tdt, device="cuda")
    rng = np.random.default_rng(5)
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        m = hi - lo
        if kind == "pose":
            mu, cov = sy.pose_initial(m, first=lo)
            _, z0, Qh = sy.pose_cycle_inputs(m, 0, mu[:, :3], first=lo)
        else:
            mu, cov = sy.orient_initial(m, first=lo)
            gyro, acc, z0, Qh = sy.orient_cycle_inputs(m, 0, mu[:, :4], first=lo)
        mu = np.repeat(mu[::GROUP], GROUP, axis=0)[:m]        # one state per track of 8 ...
        sig = np.sqrt(np.einsum("nii->ni", cov))
        mu[:, vec] += rng.standard_normal((m, len(vec))) * sig[:, tan]      # ... perturbed by about its own sigma
        rot = rng.uniform(-1, 1, (m, 3)) * 0.33 / np.sqrt(3.0)
        mu[:, q0:q0 + 4] = quat_mul(mu[:, q0:q0 + 4], quat_exp(rot))
        e.initialize(mu, cov, first=lo)
        if kind != "pose":
            e.set_orient_inputs(gyro, acc, first=lo)
        z[lo:hi] = torch.from_numpy(z0).to("cuda", tdt)
        Q[lo:hi] = torch.from_numpy(Qh.reshape(-1, 9)).to("cuda", tdt)
    e.sync()
    torch.cuda.synchronize()
    return e, z, Q, tdt


def timed(e, fn):
    e.timer_begin()
    for _ in range(LAUNCHES):
        fn()
    return e.timer_end() / LAUNCHES


def run(kind, n, prec, model):
    e, z, Q, tdt = build(kind, n, prec)
    calls = {"update": lambda: e.update_dev(model, z, Q)}
    keep = []
    for M in (2, 4, 8):
        w = torch.full((n,), 1.0 / M, dtype=tdt, device="cuda")
        wp = torch.empty((n,), dtype=tdt, device="cuda")
        mu_o = torch.empty((n // M, e.S), dtype=tdt, device="cuda")
        cov_o = torch.empty((n // M, e.PK), dtype=tdt, device="cuda")
        st = torch.empty((n // M,), dtype=torch.int32, device="cuda")
        P = 0.999 * np.eye(M) + 0.001 / M
        keep.append((w, wp, mu_o, cov_o, st))
        calls[f"mix M={M}"] = (lambda M=M, w=w, wp=wp, st=st, P=P: e.bank_mix_dev(M, w, P, wp, st))
        calls[f"combine M={M}"] = (lambda M=M, w=w, mu_o=mu_o, cov_o=cov_o, st=st: e.bank_combine_dev(M, w, mu_o, cov_o, st))
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for name, fn in calls.items():
        for _ in range(3):
            fn()
    e.sync()
    for _ in range(REPS):
        for name, fn in calls.items():   # interleaved
            ms[name].append(timed(e, fn))
    bad = int(sum(int((k[4] != 0).sum()) for k in keep))
    label = f"{kind} {'fp64' if prec == spe.F64 else 'fp32'} {n} filters"
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{label:34s} {name:14s} {med[name]:8.4f} ms  (min {min(v):.4f} max {max(v):.4f}, spread {100 * (max(v) - min(v)) / med[name]:.1f} %)"
              f"  {n / med[name] / 1e3:9.1f} M filters/s  x{med[name] / med['update']:.3f} of the update launch")
    print(f"{label:34s} tracks with a non-zero status in the last launches: {bad}; engine status summary {e.status_summary()}")
    e.close()


if __name__ == "__main__":
    print(f"# interleaved, {REPS} repetitions of {LAUNCHES} launches each, HIP-event timing on the engine's stream")
    run("pose", 1048576, spe.F64, spe.MEAS_POS3)
    run("pose", 1048576, spe.F32, spe.MEAS_POS3)
    run("orient", 4194304, spe.F32, spe.MEAS_ORIENT_BODYVEL3)
