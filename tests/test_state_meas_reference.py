"""Pins tests/state_meas_reference.py, the NumPy statement of the joint state-block measurement (include/ukf_batch.h): one
block is the oracle's own single-block update on the same numbers, fusing an estimate with itself halves the covariance,
covariance intersection of an estimate with itself returns it, and the status rules."""
import numpy as np
import pytest

import state_meas_reference as smr
from oracle import ukf_numpy as on

N = 62


def initial(spe, model):
    mu, cov = spe.synth.pose_initial(N) if model == "pose" else spe.synth.orient_initial(N)
    return (on.POSE if model == "pose" else on.ORIENT), mu, cov


def embed(man, block, z, Q3, B):
    """a [B, 3] / [B, 4] sample of one block and its 3 x 3 covariance in the state's own layout, NaN elsewhere"""
    kind, s0, t0, n = man.fields[block]
    zf, Qf = np.full((B, man.S), np.nan), np.full((B, man.D, man.D), np.nan)
    zf[:, s0:s0 + z.shape[1]] = z
    Qf[:, t0:t0 + 3, t0:t0 + 3] = Q3
    return zf, Qf


def test_sub_manifold_indices():
    m, si, ti = smr.sub_manifold(on.POSE, 0b0011)
    assert (m.S, m.D) == (7, 6) and list(si) == list(range(7)) and list(ti) == list(range(6))
    m, si, ti = smr.sub_manifold(on.POSE, 0b1010)
    assert (m.S, m.D) == (7, 6) and list(si) == [3, 4, 5, 6, 10, 11, 12] and list(ti) == [3, 4, 5, 9, 10, 11]
    assert m.fields == [("so3", 0, 0, 3), ("vec", 4, 3, 3)]
    m, si, ti = smr.sub_manifold(on.ORIENT, 0b10001)
    assert (m.S, m.D) == (5, 4) and list(si) == [0, 1, 2, 3, 13] and list(ti) == [0, 1, 2, 12]
    m, si, ti = smr.sub_manifold(on.ORIENT, 31)
    assert (m.S, m.D) == (14, 13) and list(si) == list(range(14)) and list(ti) == list(range(13))


@pytest.mark.parametrize("block,model_id", [(0, on.MEAS_POS3), (2, on.MEAS_VEL3), (3, on.MEAS_ANGVEL3)])
def test_one_vector_block_is_the_oracles_update(spe, block, model_id):
    man, mu, cov = initial(spe, "pose")
    rng = np.random.default_rng(3)
    s0 = man.fields[block][1]
    z3 = mu[:, s0:s0 + 3] + 0.05 * rng.standard_normal((N, 3))
    A = rng.standard_normal((N, 3, 3))
    Q3 = 0.01 * (A @ np.swapaxes(A, 1, 2) + np.eye(3))
    zf, Qf = embed(man, block, z3, Q3, N)
    m_r, C_r, s_r = on.pose_update(mu, cov, model_id, z3, Q3)
    m, C, d2, ll, st = smr.update_state(man, mu, cov, 1 << block, zf, Qf)
    assert np.array_equal(m, m_r) and np.array_equal(C, C_r) and np.array_equal(st, s_r) and (st == 0).all()
    assert np.isfinite(d2).all() and (d2 >= 0).all() and np.isfinite(ll).all()


def test_the_orientation_block_is_the_oracles_update(spe):
    man, mu, cov = initial(spe, "pose")
    rng = np.random.default_rng(4)
    zq = on.so3_boxplus(mu[:, 3:7], 0.05 * rng.standard_normal((N, 3)))
    A = rng.standard_normal((N, 3, 3))
    Q3 = 0.01 * (A @ np.swapaxes(A, 1, 2) + np.eye(3))
    zf, Qf = embed(man, 1, zq, Q3, N)
    m_r, C_r, s_r = on.ukf_update(on.POSE, on.SO3, mu, cov, zq, lambda X: X[..., 3:7], Q3)
    m, C, _, _, st = smr.update_state(man, mu, cov, 2, zf, Qf)
    assert np.array_equal(m, m_r) and np.array_equal(C, C_r) and np.array_equal(st, s_r) and (st == 0).all()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_fusing_an_estimate_with_itself(spe, model):
    """z = mu, Qz = Sigma, every block: the Kalman update leaves the mean and halves the covariance; covariance intersection
    (a = b = 2) returns Sigma.  Measured on these inputs: |C - Sigma / 2| / max|Sigma| <= 2.2e-14, |m (-) mu| <= 5e-19."""
    man, mu, cov = initial(spe, model)
    full = (1 << len(man.fields)) - 1
    scale = np.abs(cov).max(axis=(1, 2))[:, None, None]
    m, C, d2, ll, st = smr.update_state(man, mu, cov, full, mu, cov)
    assert (st == 0).all()
    assert np.abs(man.boxminus(m, mu)).max() <= 1e-12 and (np.abs(C - 0.5 * cov) / scale).max() <= 1e-12
    assert np.abs(d2).max() <= 1e-12
    m, C, _, _, st = smr.update_state(man, mu, cov, full, mu, cov, a=2.0, b=2.0)
    assert (st == 0).all()
    assert np.abs(man.boxminus(m, mu)).max() <= 1e-12 and (np.abs(C - cov) / scale).max() <= 1e-12


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_status_rules(spe, model):
    man, mu, cov = initial(spe, model)
    nb = len(man.fields)
    masks = np.full(N, 0b101, dtype=np.int64)
    z, Qz = mu.copy(), cov.copy()
    init = np.ones(N, bool)
    masks[3], masks[4], masks[5] = 0, -7, 1 << nb          # no measurement, negative, a block the model does not have
    _, s1, t1 = smr.sub_manifold(man, 0b101)
    unsel = [s for s in range(man.S) if s not in s1][0]
    z[7, s1[0]] = np.nan                                   # selected entry of z
    Qz[8, t1[-1], t1[0]] = Qz[8, t1[0], t1[-1]] = np.inf   # selected entry of Qz
    z[9, unsel] = np.nan                                   # unselected: must update normally
    Qz[9, 3, :] = Qz[9, :, 3] = np.nan                     # (tangent dimension 3 is outside blocks 0 and 2 in both models)
    Qz[10] = -np.eye(man.D)                                # S not positive definite
    init[11] = False
    m, C, d2, ll, st = smr.update_state(man, mu, cov, masks, z, Qz, initialised=init)
    clean = smr.update_state(man, mu, cov, 0b101, mu, cov)
    expect = np.zeros(N, dtype=np.uint32)
    expect[[3, 4, 5]] = on.ST_INACTIVE
    expect[[7, 8]] = on.ST_ERR_NONFINITE_MEAS
    expect[10] = on.ST_ERR_CHOLESKY
    expect[11] = on.ST_UNINITIALISED
    assert np.array_equal(st, expect)
    kept = expect != 0
    assert np.array_equal(m[kept], mu[kept]) and np.array_equal(C[kept], cov[kept])
    assert np.isnan(d2[kept]).all() and np.isnan(ll[kept]).all()
    assert np.array_equal(m[~kept], clean[0][~kept]) and np.array_equal(C[~kept], clean[1][~kept])
    assert np.array_equal(d2[~kept], clean[2][~kept]) and st[9] == 0 and not np.array_equal(C[9], cov[9])
    # the gate: the reference's own d^2 decides, a rejected filter keeps its state and still reports d^2
    zg = man.boxplus(mu, 0.02 * np.random.default_rng(5).standard_normal((N, man.D)))
    free = smr.update_state(man, mu, cov, 0b101, zg, cov)
    gate = float(np.median(free[2]))
    m, C, d2, ll, st = smr.update_state(man, mu, cov, 0b101, zg, cov, gate_chi2=gate)
    rej = free[2] > gate
    assert rej.any() and (~rej).any() and np.array_equal(st, np.where(rej, on.ST_REJECTED_GATE, 0).astype(np.uint32))
    assert np.array_equal(m[rej], mu[rej]) and np.array_equal(C[rej], cov[rej]) and np.array_equal(d2, free[2])
    assert np.array_equal(m[~rej], free[0][~rej]) and np.array_equal(C[~rej], free[1][~rej])
