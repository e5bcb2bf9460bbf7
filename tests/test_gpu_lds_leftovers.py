"""No kernel of the engine may depend on LDS it did not write itself.

tests/cpp/lds_poison.hip fills the LDS of every CU with a bit pattern; the engine then runs the launches the BASELINE
configurations use (fused cycle, separate prediction and update, multi-cycle, per-filter models, event rounds = the
indirect kernel) and must give the SAME BITS
after a NaN pattern, an Inf pattern and zeros.  Found in round 3 by tests/fuzz_parity.py as a box-dependent Cholesky failure:
an alignment pad between two LDS regions was read as "leftover times the table's exact-zero row" -- NaN whenever the leftover
of an earlier kernel happened to be NaN or Inf (Layout16::LAF_PAD in ukf_kernel16.hpp).

test_newer_launches_do_not_depend_on_lds_leftovers does the same, the poison in front of every launch, for what came after that
test: the wide-arithmetic instantiations and the bucketed, scheduled, mixed multi-cycle, uniform-Q and timestamp launches.  The
row-layout feature kernels have tests/test_gpu_feature_lds_leftovers.py.

test_the_poison_is_seen_by_the_next_kernel shows that the instrument is not blind.  Measured on an MI355X
(profiles/lds_leftovers.txt): a kernel of the fill's geometry that writes no LDS finds the pattern in 41943040 of the 41943040
dwords of its allocations, share 1.0000, for each of 0x7fc00000, 0x7f800000 and 0xffffffff.  LDS is not cleared between
dispatches and the fill leaves no byte out, so the tests cover the whole LDS of every compute unit their workgroups land on."""
import numpy as np
import pytest

from probe_support import LDS_PATTERNS, lds_leftovers_seen, lds_poison

pytestmark = pytest.mark.gpu


def _run(spe, model, prec, G, n=4099, **cfg):
    import torch
    s = spe.synth
    tdt = torch.float64 if prec == 0 else torch.float32
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1))).to("cuda", tdt)   # noqa: E731
    out = []
    if model == "pose":
        mu, cov = s.pose_initial(n)
        e = spe.BatchPoseUKF(n, precision=prec, lanes_per_filter=G, **cfg)
        e.initialize(mu, cov)
        acc, z, Q = s.pose_cycle_inputs(n, 0, mu[:, :3], random_q=True)
        e.set_acceleration(acc, 0.01 * np.eye(3))
        e.cycle(0.01, spe.MEAS_POS3, z, Q)
        models = s.pose_mixed_models(n, 1)
        zz = s.pose_measurement_for_model(mu, models, z - mu[:, :3])
        e.update(models, zz, Q)                                  # per-filter models incl. the SO(3) sigma-point path
        e.set_acceleration(np.full((n, 3), np.nan), None)        # constant-velocity branch: rotated noise, shaped-noise table
        e.predict(0.02)
        z_t, Q_t = dev(np.stack([z, z])), dev(np.stack([Q.reshape(n, 9)] * 2))
        torch.cuda.synchronize()
        e.cycle_multi_dev(2, 0.01, spe.MEAS_VEL3, z_t.reshape(2, n, 3), Q_t.reshape(2, n, 9), 2, 0)
    else:
        mu, cov = s.orient_initial(n)
        e = spe.BatchOrientationUKF(n, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE, precision=prec, lanes_per_filter=G, **cfg)
        R = s.orient_process_noise()
        e.set_process_noise(R)
        e.initialize(mu, cov)
        gyro, acc, z, Q = s.orient_cycle_inputs(n, 0, mu[:, :4])
        e.set_orient_inputs(gyro, acc)
        e.cycle(0.01, spe.MEAS_ORIENT_BODYVEL3, z, Q)
        R2 = R.copy(); R2[0, 0] *= 3.0; R2[4, 4] *= 2.0            # anisotropic blocks: the rotated-noise path
        e.set_process_noise(R2)
        e.predict(0.02)
        e.update(spe.MEAS_ORIENT_BODYVEL3, z, Q)
        z_t, Q_t = dev(np.stack([z, z])), dev(np.stack([Q.reshape(n, 9)] * 2))
        torch.cuda.synchronize()
        e.cycle_multi_dev(2, 0.01, spe.MEAS_ORIENT_BODYVEL3, z_t.reshape(2, n, 3), Q_t.reshape(2, n, 9), 2, 0)
    m, c, _ = e.state()
    st = e.status()
    # the indirect instantiation (event rounds): two samples for every third filter, a third one for some, any arrival order
    rng = np.random.default_rng(5)
    f_ev = np.concatenate([np.arange(0, n, 3), np.arange(0, n, 3), np.arange(0, n, 7)])
    t_ev = np.concatenate([np.full(len(range(0, n, 3)), 1_010_000), np.full(len(range(0, n, 3)), 1_020_000), np.full(len(range(0, n, 7)), 1_030_000)])
    perm = rng.permutation(f_ev.size)
    f_ev, t_ev = f_ev[perm], t_ev[perm]
    model_ev = spe.MEAS_POS3 if model == "pose" else spe.MEAS_ORIENT_BODYVEL3
    e.process_events(f_ev, t_ev, np.full(f_ev.size, model_ev, dtype=np.int32), z[f_ev], Q[f_ev])
    m2, c2, _ = e.state()
    st2 = e.status()
    e.close()
    return m, c, st, m2, c2, st2


@pytest.mark.parametrize("G", [16, 64])      # the tuned layout and the one-wavefront-per-filter ablation (fp32 in the shipped library)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_results_do_not_depend_on_lds_leftovers(spe, model, prec, G):
    poison = lds_poison()
    ref = None
    for pat in LDS_PATTERNS:
        assert poison(pat) == 0
        got = _run(spe, model, prec, G)
        m, c, st, m2, c2, _ = got
        assert np.isfinite(m).all() and np.isfinite(c).all() and (st == 0).all(), (model, prec, hex(pat))
        assert np.isfinite(m2).all() and np.isfinite(c2).all() and not np.array_equal(m, m2), (model, prec, hex(pat))
        if ref is None:
            ref = got
        else:
            assert all(np.array_equal(x, y) for x, y in zip(got, ref)), (model, prec, hex(pat))


# ------------------------------------------------------------------------------ the launches added after the test above
MODES = {"f64": (0, 0), "f32": (1, 0), "f32w": (1, 1)}   # (precision, wide_arithmetic)
BUCKETED_N = 16387                                        # cycle_dev groups per-filter models from 16384 filters on
ST_INACTIVE = 1 << 8


def _newer_launches(spe, model, mode, poison, pat, n=4099):
    """cycle_dev with per-filter models (at BUCKETED_N too: the grouped indirect launch of ukf_buckets.hip), cycle_schedule_dev,
    cycle_multi_mixed_dev, cycle_uniform_q_dev and predict_timestamps_dev, the LDS poisoned in front of every one of them
    -> [(mean, covariance, status, expected non-zero status rows)] after each launch"""
    import torch
    s = spe.synth
    prec, wide = MODES[mode]
    tdt = torch.float64 if prec == 0 else torch.float32
    cfg = {"wide_arithmetic": 1} if wide else {}
    out = []

    def dev(x, k):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, k))).to("cuda", tdt)

    def engine(n):
        if model == "pose":
            mu, cov = s.pose_initial(n)
            e = spe.BatchPoseUKF(n, precision=prec, lanes_per_filter=16, **cfg)
            e.initialize(mu, cov)
            acc, z, Q = s.pose_cycle_inputs(n, 0, mu[:, :3], random_q=True)
            e.set_acceleration(acc, 0.01 * np.eye(3))
            mods = [s.pose_mixed_models(n, k) for k in range(2)]
            zs = [s.pose_measurement_for_model(mu, m, z - mu[:, :3]) for m in mods]
            full = spe.MEAS_POS3
        else:
            mu, cov = s.orient_initial(n)
            e = spe.BatchOrientationUKF(n, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE, precision=prec, lanes_per_filter=16, **cfg)
            e.set_process_noise(s.orient_process_noise())
            e.initialize(mu, cov)
            gyro, acc, z, Q = s.orient_cycle_inputs(n, 0, mu[:, :4])
            e.set_orient_inputs(gyro, acc)
            full = spe.MEAS_ORIENT_BODYVEL3
            mods = [np.where(np.arange(n) % 5 == 1 + k, -1, full).astype(np.int32) for k in range(2)]
            zs = [z, z]
        return e, z, Q, mods, zs, full

    def launch(e, call, expect_nonzero):
        torch.cuda.synchronize()
        assert poison(pat) == 0
        call()
        e.sync()
        m, c, _ = e.state()
        out.append((m, c, e.status(), expect_nonzero))

    # the grouped launch needs BUCKETED_N filters; the same call at n takes the ordinary per-filter launch
    for nn in (BUCKETED_N, n):
        e, z, Q, mods, zs, full = engine(nn)
        m_d = torch.from_numpy(mods[0]).to("cuda")
        z_d, Q_d = dev(zs[0], 3), dev(Q, 9)
        launch(e, lambda: e.cycle_dev(0.01, full, z_d, Q_d, meas_model_dev=m_d), mods[0] < 0)
        if nn == BUCKETED_N:
            assert e.last_model_groups().size >= nn   # the launch did group its filters
            e.close()
    vel = spe.MEAS_VEL3 if model == "pose" else full
    z3 = torch.stack([dev(z, 3), dev(0.1 * z, 3), dev(0.1 * z, 3)])
    Q3 = torch.stack([Q_d, Q_d, Q_d])
    none = np.zeros(n, bool)
    launch(e, lambda: e.cycle_schedule_dev([0.01, 0.02, 0.01], [full, -1, vel], z3, Q3, 3, 0), none)
    m_r = torch.from_numpy(np.stack(mods)).to("cuda").contiguous()
    z_r = torch.stack([dev(zs[0], 3), dev(zs[1], 3)])
    launch(e, lambda: e.cycle_multi_mixed_dev(2, 0.01, m_r, z_r, Q3[:2].contiguous(), 2, 0), (mods[0] < 0) | (mods[1] < 0))
    q9 = dev(0.05 ** 2 * np.eye(3), 9).reshape(9)
    launch(e, lambda: e.cycle_uniform_q_dev(0.01, full, z_d, q9), none)
    # stamps: most filters 10 ms after their last sample, every 9th at it (too small a step), every 11th before it
    last = np.full(n, 1_000_000, dtype=np.int64)
    ts = last + 10_000
    ts[::9] = last[::9]
    ts[5::11] = last[5::11] - 3_000
    e.set_last_measurement_time(last)
    ts_d = torch.from_numpy(ts).to("cuda")
    launch(e, lambda: e.predict_timestamps_dev(ts_d), ts <= last)
    e.close()
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_newer_launches_do_not_depend_on_lds_leftovers(spe, model, mode):
    """the wide-arithmetic instantiations through the launches of the test above, and for every precision the bucketed, scheduled,
    mixed multi-cycle, uniform-Q and timestamp launches: finite, status 0 except the filters without a sample and the gated
    ones, and the same bits after every pattern"""
    poison = lds_poison()
    ref = wide_ref = None
    for pat in LDS_PATTERNS:
        if mode == "f32w":
            assert poison(pat) == 0
            got = _run(spe, model, 1, 16, wide_arithmetic=1)
            m, c, st, m2, c2, _ = got
            assert np.isfinite(m).all() and np.isfinite(c).all() and (st == 0).all(), (model, hex(pat))
            assert np.isfinite(m2).all() and np.isfinite(c2).all() and not np.array_equal(m, m2), (model, hex(pat))
            if wide_ref is None:
                wide_ref = got
            assert all(np.array_equal(x, y) for x, y in zip(got, wide_ref)), (model, hex(pat))
        got = _newer_launches(spe, model, mode, poison, pat)
        for k, (m, c, st, nonzero) in enumerate(got):
            assert np.isfinite(m).all() and np.isfinite(c).all(), (model, mode, hex(pat), k)
            assert np.array_equal(st != 0, nonzero), (model, mode, hex(pat), k, np.unique(st))
        assert (got[0][2][got[0][3]] == ST_INACTIVE).all() and got[0][3].sum() > 1000
        if ref is None:
            ref = got
        for k, (a, b) in enumerate(zip(got, ref)):
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])), (model, mode, hex(pat), k)


def test_the_poison_is_seen_by_the_next_kernel():
    """the canary of the instrument: after poison(pattern) a kernel of the fill's geometry that writes no LDS finds the pattern
    in its own allocation.  Were LDS cleared between dispatches, or the fill blind, matched would be 0 and every leftover test
    would pass vacuously.  The share is printed, not asserted (profiles/lds_leftovers.txt)."""
    poison, seen = lds_poison(), lds_leftovers_seen()
    for pat in LDS_PATTERNS[:3]:
        assert pat != 0 and poison(pat) == 0
        matched, read = seen(pat)
        print(f"LEFTOVERS pattern={pat:#010x} share={matched}/{read} = {matched / max(read, 1):.4f}")
        assert read == 1024 * 160 * 1024 // 4 and matched > 0, (hex(pat), matched, read)
