"""Filter banks on the device (ukfb_bank_weights_dev / ukfb_bank_combine_dev / ukfb_bank_mix_dev and the host-array forms,
include/ukf_batch.h): an engine read as capacity / M tracks of M hypotheses, track-major.

The reference is tests/bank_reference.py (pinned by tests/test_bank_reference.py), computed on the state DOWNLOADED from the
engine and on the weights as the device arrays hold them, so that fp32 storage rounding of the inputs is out of the comparison.
Parity bound: |x - ref| <= tol (1 + |ref|), tol = the README's parity gates 1e-9 (fp64) / 1e-4 (fp32); fp32 engines with
wide_arithmetic compute in fp64 and store fp32: 1e-9 + 2^-23.  The maxima measured on an MI355X are in profiles/bank_parity.txt.

Every parity comparison also makes the SCALED one (tests/feature_scaled_parity.py): the combined moments and every mixed hypothesis whitened by the
reference's own sigmas and held block by block -- fp64 1e-9; wide_arithmetic 2 u v + 1e-9 against the float64 reference on the
inputs as stored (the kernel narrows each stored output once); plain fp32 max(M_feat d_32, 20 u v), d_32 the distance of the
all-float32 evaluation of the same call (tests/feature_f32.py) from its float64 evaluation on the same batch.  It prints one
SCALED line: the largest fraction of a bound and the block it belongs to.  The weights are dimensionless
and stay on the bound above.  The IMM run is a chain of 120 launches, not one call: its fp64 run is held to 1e-9 in the
whitened metric at its first and last cycle, its fp32 runs stay on the run-length rule below.

The end-to-end IMM run compares a 20-cycle chain (mix, predict, innovation, update, weights, combine) against the same chain in
NumPy float64, started from the state as downloaded.  All 20 cycles run and are printed in every precision.  fp64 and fp32 engines
are held to their gates for all 20 (measured worst: 3.7e-15 and 1.9e-6).  An fp32 engine with wide_arithmetic stores fp32 after every
one of the six launches of a cycle, and its gate 1e-9 + 2^-23 is ONE such rounding: the run it is held to the gate for is shortened
to the longest at which the reference's own fp32-storage instantiation (float64 arithmetic, every launch's results rounded to fp32)
holds that gate against the reference proper -- a length that comes from the number format, computed by the test, never from the
engine.  The gate is not widened; the remaining cycles still have to run with status 0 and show the manoeuvre.
"""
import numpy as np
import pytest
import torch

import bank_reference as br
import feature_f32 as ff
import feature_scaled_parity as fsp
from engine_support import dev, new_engine, same_snapshot, scaled, snapshot, stored, tdt, unpack

pytestmark = pytest.mark.gpu

T_TRACKS = 1022   # not a multiple of four: the last workgroup holds two tracks
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]
LN2PI = float(np.log(2.0 * np.pi))


# ---------------------------------------------------------------------------------------------------------------- helpers
def snap(e):
    """the engine's snapshot with the process noise of these filters"""
    return snapshot(e, (0, 1, e.capacity // 2, e.capacity - 1))


def bank_engine(spe, onp, model, T, M, prec, wide, seed=7):
    """an engine of T tracks x M hypotheses built as in the prototype, its state as downloaded, and weights as stored"""
    man, mu, cov, w = br.make_tracks(spe, onp, model, T, M, seed=seed)
    e = new_engine(spe, model, T * M, prec, wide)
    e.initialize(mu.reshape(T * M, man.S), cov.reshape(T * M, man.D, man.D))
    latch_inputs(spe, e, model)
    return e, man, stored(w, e.dtype)


def latch_inputs(spe, e, model):
    """distinct last measurement times, latched inputs and a per-filter process noise on every third filter: what a read-only
    call must leave alone"""
    n, sy = e.capacity, spe.synth
    e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
    if model == "pose":
        acc = sy.uniform(sy.SEED_BASE + 31, np.arange(n), np.arange(3), -0.5, 0.5).reshape(n, 3)
        e.set_acceleration(acc, 0.01 * np.eye(3))
    else:
        gyro = sy.uniform(sy.SEED_BASE + 32, np.arange(n), np.arange(3), -0.05, 0.05).reshape(n, 3)
        acc = sy.uniform(sy.SEED_BASE + 33, np.arange(n), np.arange(3), -0.3, 0.3).reshape(n, 3) + np.array([0.0, 0.0, 9.81])
        e.set_orient_inputs(gyro, acc)


def downloaded(e, man, T, M):
    mu, cov, init = e.state()
    return mu.reshape(T, M, man.S), cov.reshape(T, M, man.D, man.D), init.reshape(T, M)


def combine_dev(e, M, w, want_cov=True):
    """-> mu [T, S], cov [T, D, D] or None, status [T] (float64 / int64), and the raw tensors"""
    T = e.capacity // M
    t = tdt(e)
    w_t = dev(e, w.reshape(-1))
    mu_t = torch.full((T, e.S), 7.0, dtype=t, device="cuda")
    cov_t = torch.full((T, e.PK), 7.0, dtype=t, device="cuda") if want_cov else None
    st_t = torch.full((T,), 0x7FFF, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.bank_combine_dev(M, w_t, mu_t, cov_t, st_t)
    e.sync()
    cov = unpack(cov_t.cpu().numpy().astype(np.float64), e.D) if want_cov else None
    return mu_t.cpu().numpy().astype(np.float64), cov, st_t.cpu().numpy().astype(np.int64), (mu_t, cov_t)


def mix_dev(e, M, w, P):
    T = e.capacity // M
    w_t = dev(e, w.reshape(-1))
    wp_t = torch.full((T * M,), 7.0, dtype=tdt(e), device="cuda")
    st_t = torch.full((T,), 0x7FFF, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.bank_mix_dev(M, w_t, P, wp_t, st_t)
    e.sync()
    return wp_t.cpu().numpy().astype(np.float64).reshape(T, M), st_t.cpu().numpy().astype(np.int64)


def scaled_combine(name, model, pname, m_g, C_g, m_r, C_r, mu, cov, w, **kw):
    """the scaled check (tests/feature_scaled_parity.py) of combined moments against the reference's, block by block"""
    fsp.judge_state(name, model, pname, m_g, C_g, m_r, C_r, f32=lambda: tuple(ff.mixture(model, mu, cov, w, p, **kw) for p in ("f32", "f64")))


def scaled_mix(name, model, pname, mu_g, cov_g, mu_r, cov_r, mu, cov, w, Pk, **kw):
    """the same for every mixed hypothesis"""
    fsp.judge_state(name, model, pname, mu_g, cov_g, mu_r, cov_r, f32=lambda: tuple(ff.mix(model, mu, cov, w, Pk, p, **kw) for p in ("f32", "f64")))


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("M", [2, 3, 4, 8])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_combine_and_mix_against_the_reference(spe, onp, model, pname, prec, wide, tol, M):
    T = T_TRACKS
    e, man, w = bank_engine(spe, onp, model, T, M, prec, wide)
    w = w / w.sum(axis=1, keepdims=True)
    w = stored(w, e.dtype)
    mu, cov, init = downloaded(e, man, T, M)
    assert init.all()
    ro = br.rot_offset(man)
    spread = np.linalg.norm(man.boxminus(mu[:, 1], mu[:, 0])[:, ro:ro + 3], axis=1)
    assert spread.max() >= 0.2, "the tracks must spread their rotations, or the transport is not exercised"
    # ---- combine (read-only)
    before = snap(e)
    m_g, C_g, st, _ = combine_dev(e, M, w)
    assert same_snapshot(before, snap(e)), "combine changed the engine"
    m_r, C_r, conv = br.mixture(man, mu, cov, w)
    assert conv.all() and (st == 0).all()
    em, ec = scaled(m_g, m_r), scaled(C_g, C_r)
    _, C_0, _ = br.mixture(man, mu, cov, w, transport=False)
    soft = scaled(C_0, C_r)
    print(f"bank parity {model} {pname} M={M} combine: mean {em:.3e} cov {ec:.3e} (no-transport reference: {soft:.3e})")
    assert soft > 1e-9, "the no-transport variant must be outside the fp64 gate, or this test cannot tell them apart"
    assert em <= tol and ec <= tol
    scaled_combine(f"bank/{model}/{pname}/M={M}/combine", model, pname, m_g, C_g, m_r, C_r, mu, cov, w)
    # mean only
    m_only, _, st2, _ = combine_dev(e, M, w, want_cov=False)
    assert np.array_equal(m_only, m_g) and (st2 == 0).all()
    # host form: the same bits
    m_h, C_h, st_h = e.bank_combine(M, w.reshape(-1))
    assert np.array_equal(m_h, m_g) and np.array_equal(C_h, C_g) and (st_h == 0).all()
    # ---- mix
    P = br.transition(M)
    Pk = stored(P, e.dtype) if (prec == 1 and not wide) else P    # fp32 kernels take the matrix in fp32
    mu_r, cov_r, c_r, conv = br.mix(man, mu, cov, w, Pk)
    wp, st = mix_dev(e, M, w, P)
    assert conv.all() and (st == 0).all()
    mu_g, cov_g, _ = downloaded(e, man, T, M)
    em, ec, ew = scaled(mu_g, mu_r), scaled(cov_g, cov_r), scaled(wp, c_r)
    print(f"bank parity {model} {pname} M={M} mix:     mean {em:.3e} cov {ec:.3e} w_pred {ew:.3e}")
    assert em <= tol and ec <= tol and ew <= tol
    scaled_mix(f"bank/{model}/{pname}/M={M}/mix", model, pname, mu_g, cov_g, mu_r, cov_r, mu, cov, w, Pk)
    # the mixed covariances factorise: a prediction has status 0 everywhere
    if model == "orient":
        n = T * M
        e.set_orient_inputs(np.zeros((n, 3)), np.tile([0.0, 0.0, 9.81], (n, 1)))
    e.predict(0.01)
    assert e.status_summary() == 0
    e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_combine_is_read_only(spe, onp, model, pname, prec, wide, tol):
    """mean, covariance, status, last measurement time and latched inputs bit-identical: downloads before and after, and -- for
    the latches that have no getter -- the next prediction is the one an untouched twin makes"""
    T, M = 514, 4
    e, man, w = bank_engine(spe, onp, model, T, M, prec, wide)
    twin, _, _ = bank_engine(spe, onp, model, T, M, prec, wide)
    w = stored(w / w.sum(axis=1, keepdims=True), e.dtype)
    e.predict(0.01); twin.predict(0.01)          # a status array and a state that a launch has written
    before = snap(e)
    assert len(np.unique(before[4])) == T * M and same_snapshot(before, snap(twin))
    _, _, st, _ = combine_dev(e, M, w)
    m_h, C_h, st_h = e.bank_combine(M, w.reshape(-1))
    assert (st == 0).all() and (st_h == 0).all()
    assert same_snapshot(before, snap(e)), "combine changed the engine"
    e.predict(0.01); twin.predict(0.01)
    assert same_snapshot(snap(e), snap(twin)), "the prediction after combine is not the untouched twin's"
    e.close(); twin.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_mean_iteration_cap_sets_noconv(spe, onp, model, pname, prec, wide, tol, cap=1):
    """mean_max_iter = 1 on spread tracks: the iteration leaves at the cap with |d| > mean_tol, the track gets
    WARN_MEAN_NOCONV, and mean and covariance are those of the reference stopped at the same cap"""
    T, M = 254, 4
    e, man, w = bank_engine(spe, onp, model, T, M, prec, wide)
    e.configure(mean_max_iter=cap)
    w = stored(w / w.sum(axis=1, keepdims=True), e.dtype)
    mu, cov, _ = downloaded(e, man, T, M)
    m_r, C_r, conv = br.mixture(man, mu, cov, w, max_it=cap)
    assert not conv.any(), "the tracks must not converge within the cap, or the flag is not reached"
    m_g, C_g, st, _ = combine_dev(e, M, w)
    assert np.array_equal(st, np.full(T, spe.ST_WARN_MEAN_NOCONV))
    assert scaled(m_g, m_r) <= tol and scaled(C_g, C_r) <= tol
    scaled_combine(f"bank/{model}/{pname}/cap={cap}/combine", model, pname, m_g, C_g, m_r, C_r, mu, cov, w, max_it=cap)
    P = br.transition(M)
    Pk = stored(P, e.dtype) if (prec == 1 and not wide) else P
    mu_r, cov_r, c_r, conv = br.mix(man, mu, cov, w, Pk, max_it=cap)
    assert not conv.any()
    wp, st = mix_dev(e, M, w, P)
    mu_g, cov_g, _ = downloaded(e, man, T, M)
    assert np.array_equal(st, np.full(T, spe.ST_WARN_MEAN_NOCONV))
    assert scaled(mu_g, mu_r) <= tol and scaled(cov_g, cov_r) <= tol and scaled(wp, c_r) <= tol
    scaled_mix(f"bank/{model}/{pname}/cap={cap}/mix", model, pname, mu_g, cov_g, mu_r, cov_r, mu, cov, w, Pk, max_it=cap)
    e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_host_mix_equals_device_mix(spe, onp, model, pname, prec, wide, tol):
    T, M = 257, 3
    P = br.transition(M)
    out = []
    for host in (False, True):
        e, man, w = bank_engine(spe, onp, model, T, M, prec, wide)
        w = stored(w / w.sum(axis=1, keepdims=True), e.dtype)
        if host:
            wp, st = e.bank_mix(M, w.reshape(-1), P)
            wp = wp.reshape(T, M)
        else:
            wp, st = mix_dev(e, M, w, P)
        out.append((wp, np.asarray(st, dtype=np.int64)) + e.state()[:2])
        e.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))


# ---------------------------------------------------------------------------------------------------------------- opposed hypotheses
def opposed_tracks(spe, onp, model, T, M, even, lattice, seed=23):
    """T tracks in which hypothesis t % M + 1 is hypothesis t % M turned by pi: q and q * (axis, 0), everything else equal.
    Weights: the turned one 2^-10, 2^-20, 2^-30, 2^-40 across the tracks, a third one 0.25 a step of make_tracks away, the rest
    on the first; or (even) 0.5 / 0.5 and 0 for the third.
    lattice: q = (+-1/2, +-1/2, +-1/2, +-1/2) and a signed coordinate axis, so that conj(q) (q (axis, 0)) = (axis, +0) without
    a rounding in any precision and any order of the products, and the logarithm is +pi axis for the engine and the reference
    alike.  About a random axis the scalar part is rounding noise of either sign, the logarithm +-pi axis, and the mixture
    mean -- which has two equally good values there -- a coin toss between two correct programs: such tracks (lattice = False)
    can be held to finite results and status, not to parity."""
    man, mu, cov, _ = br.make_tracks(spe, onp, model, T, M, seed=seed)
    so = [s_ for kind, s_, _, _ in man.fields if kind == "so3"][0]
    rng = np.random.default_rng(seed + M)
    w = np.zeros((T, M))
    for t in range(T):
        a, b = t % M, (t + 1) % M
        step = [man.boxminus(mu[t, c], mu[t, a]) for c in range(M)]
        if lattice:
            mu[t, a, so:so + 4] = 0.5 * rng.choice([-1.0, 1.0], 4)
            turn = np.zeros(4)
            turn[rng.integers(3)] = rng.choice([-1.0, 1.0])
        else:
            ax = rng.normal(size=3)
            turn = np.concatenate([ax / np.linalg.norm(ax), [0.0]])
        for c in range(M):
            mu[t, c] = man.boxplus(mu[t, a], step[c]) if c not in (a, b) else mu[t, a]
        mu[t, b, so:so + 4] = onp.quat_mul(mu[t, a, so:so + 4], turn)
        w[t, b] = 0.5 if even else 2.0 ** (-10 * (1 + t % 4))
        if M > 2:
            w[t, (t + 2) % M] = 0.0 if even else 0.25
        w[t, a] = 1.0 - w[t].sum()
    return man, mu, cov, w, so


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_hypothesis_opposite_the_heaviest_one(spe, onp, model, pname, prec, wide, tol, M):
    """A hypothesis exactly pi away from the heaviest one, the edge of the logarithm's range, where the transport Jr^-1 used to
    be 0/0: seven tracks (a ragged last wavefront).  Its weight is tiny, so a converged mixture hardly feels it -- but a NaN in
    its transport would poison the track whatever its weight.  Then the same tracks at 0.5 / 0.5 with mean_max_iter = 1: the
    moments published under WARN_MEAN_NOCONV are those of the reference stopped at the same cap.
    (The sharp test of Jr^-1 towards pi is tests/test_gpu_jacobian_primitives.py.)"""
    T = 7
    P = br.transition(M)
    for even in (False, True):
        kw = dict(max_it=1) if even else {}
        man, mu0, cov0, w0, so = opposed_tracks(spe, onp, model, T, M, even, lattice=True)
        e = new_engine(spe, model, T * M, prec, wide)
        e.initialize(mu0.reshape(T * M, man.S), cov0.reshape(T * M, man.D, man.D))
        latch_inputs(spe, e, model)
        if even:
            e.configure(mean_max_iter=1)
        w = stored(w0, e.dtype)
        mu, cov, init = downloaded(e, man, T, M)
        tr = np.arange(T)
        for j in (tr % M, (tr + 1) % M):
            assert np.array_equal(mu[tr, j, so:so + 4], mu0[tr, j, so:so + 4]), "the lattice quaternions are stored to the bit"
        assert init.all()
        turned = man.boxminus(mu[tr, (tr + 1) % M], mu[tr, tr % M])[:, br.rot_offset(man):br.rot_offset(man) + 3]
        assert np.array_equal(np.linalg.norm(turned, axis=1), np.full(T, np.pi)), "exactly pi away"
        want = np.full(T, spe.ST_WARN_MEAN_NOCONV if even else 0)
        # ---- combine
        m_r, C_r, conv = br.mixture(man, mu, cov, w, **kw)
        assert (conv == (not even)).all()
        m_g, C_g, st, _ = combine_dev(e, M, w)
        assert np.isfinite(m_g).all() and np.isfinite(C_g).all() and np.array_equal(st, want)
        em, ec = scaled(m_g, m_r), scaled(C_g, C_r)
        print(f"bank parity {model} {pname} M={M} opposed {'0.5/0.5 cap=1' if even else 'tiny weight'} combine: mean {em:.3e} cov {ec:.3e}")
        assert em <= tol and ec <= tol
        name = f"bank/{model}/{pname}/M={M}/opposed{'-cap=1' if even else ''}"
        scaled_combine(name + "/combine", model, pname, m_g, C_g, m_r, C_r, mu, cov, w, **kw)
        # ---- mix
        Pk = stored(P, e.dtype) if (prec == 1 and not wide) else P
        mu_r, cov_r, c_r, conv = br.mix(man, mu, cov, w, Pk, **kw)
        assert (conv == (not even)).all()
        wp, st = mix_dev(e, M, w, P)
        mu_g, cov_g, _ = downloaded(e, man, T, M)
        assert np.isfinite(mu_g).all() and np.isfinite(cov_g).all() and np.array_equal(st, want)
        em, ec, ew = scaled(mu_g, mu_r), scaled(cov_g, cov_r), scaled(wp, c_r)
        print(f"bank parity {model} {pname} M={M} opposed {'0.5/0.5 cap=1' if even else 'tiny weight'} mix:     mean {em:.3e} cov {ec:.3e}")
        assert em <= tol and ec <= tol and ew <= tol
        scaled_mix(name + "/mix", model, pname, mu_g, cov_g, mu_r, cov_r, mu, cov, w, Pk, **kw)
        e.close()
    # about a random axis: no poisoning, whichever sign the logarithm takes
    man, mu0, cov0, w0, so = opposed_tracks(spe, onp, model, T, M, even=False, lattice=False)
    e = new_engine(spe, model, T * M, prec, wide)
    e.initialize(mu0.reshape(T * M, man.S), cov0.reshape(T * M, man.D, man.D))
    w = stored(w0, e.dtype)
    m_g, C_g, st, _ = combine_dev(e, M, w)
    assert np.isfinite(m_g).all() and np.isfinite(C_g).all() and (st == 0).all()
    wp, st = mix_dev(e, M, w, P)
    mu_g, cov_g, _ = downloaded(e, man, T, M)
    assert np.isfinite(mu_g).all() and np.isfinite(cov_g).all() and np.isfinite(wp).all() and (st == 0).all()
    e.close()


# ---------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_one_hot_weights_and_identity_transition_keep_the_bits(spe, onp, model, pname, prec, wide, tol):
    T, M = 510, 4
    e, man, w = bank_engine(spe, onp, model, T, M, prec, wide)
    mu, cov, _ = downloaded(e, man, T, M)
    pick = np.arange(T) % M
    oh = np.zeros((T, M)); oh[np.arange(T), pick] = 1.0
    m_g, C_g, st, _ = combine_dev(e, M, oh)
    assert (st == 0).all()
    assert np.array_equal(m_g, mu[np.arange(T), pick]) and np.array_equal(C_g, cov[np.arange(T), pick])
    # Pi = I: w_{j|i} is the one-hot on i, every hypothesis is written back with its own bits
    w = stored(w / w.sum(axis=1, keepdims=True), e.dtype)
    before = snap(e)
    wp, st = mix_dev(e, M, w, np.eye(M))
    assert (st == 0).all() and same_snapshot(before, snap(e))
    assert scaled(wp, w) <= tol
    e.close()


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_zero_weight_hypothesis_never_reaches_the_result(spe, onp, model, pname, prec, wide, tol):
    """hypothesis 1 of every track has weight exactly 0 and holds 1e300 / NaN / -1e300 in turn: the results are those of the
    track whose hypothesis 1 holds an ordinary state, bit for bit, and those of the reference without it"""
    T, M = 258, 3
    man, mu, cov, w = br.make_tracks(spe, onp, model, T, M)
    w[:, 1] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    P = br.transition(M)
    res = []
    for poisoned in (False, True):
        mu_p, cov_p = mu.copy(), cov.copy()
        if poisoned:
            bad = np.array([1e300, np.nan, -1e300])[np.arange(T) % 3]
            mu_p[:, 1] = bad[:, None]
            cov_p[:, 1] = bad[:, None, None]
        e = new_engine(spe, model, T * M, prec, wide)
        e.initialize(mu_p.reshape(T * M, -1), cov_p.reshape(T * M, man.D, man.D))
        ws = stored(w, e.dtype)
        m_g, C_g, st, _ = combine_dev(e, M, ws)
        assert (st == 0).all()
        wp, st = mix_dev(e, M, ws, P)
        assert (st == 0).all()
        mu_g, cov_g, _ = downloaded(e, man, T, M)
        res.append((m_g, C_g, wp, mu_g[:, [0, 2]], cov_g[:, [0, 2]]))
        if not poisoned:
            keep = [0, 2]
            mu_d, cov_d = stored(mu, e.dtype), stored(cov, e.dtype)
            m_r, C_r, _ = br.mixture(man, mu_d[:, keep], cov_d[:, keep], ws[:, keep])
            assert scaled(m_g, m_r) <= tol and scaled(C_g, C_r) <= tol
            scaled_combine(f"bank/{model}/{pname}/zero-weight/combine", model, pname, m_g, C_g, m_r, C_r, mu_d[:, keep], cov_d[:, keep],
                           ws[:, keep])
        e.close()
    assert all(np.isfinite(x).all() for x in res[1])
    assert all(np.array_equal(a, b) for a, b in zip(*res))


# ---------------------------------------------------------------------------------------------------------------- failures
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_per_track_failures_stay_on_their_track(spe, onp, model, pname, prec, wide, tol):
    T, M = 64, 4
    man, mu, cov, w = br.make_tracks(spe, onp, model, T, M)
    P = br.transition(M)
    UNINIT, NEG, NAN, SUM = 5, 18, 35, 50     # tracks 4 ... 7, 16 ... 19, 32 ... 35, 48 ... 51 share a wavefront with one each
    runs = []
    for broken in (False, True):
        e = new_engine(spe, model, T * M, prec, wide)
        flat_mu, flat_cov = mu.reshape(T * M, -1), cov.reshape(T * M, man.D, man.D)
        if broken:   # hypothesis 2 of track UNINIT is never initialised
            k = UNINIT * M + 2
            e.initialize(flat_mu[:k], flat_cov[:k])
            e.initialize(flat_mu[k + 1:], flat_cov[k + 1:], first=k + 1)
        else:
            e.initialize(flat_mu, flat_cov)
        ws = stored(w, e.dtype)
        if broken:
            ws[NEG, 1] = -ws[NEG, 1]
            ws[NAN, 3] = np.nan
            ws[SUM, 0] += 64 * M * np.finfo(e.dtype).eps
        m_g, C_g, st_c, _ = combine_dev(e, M, ws)
        before = downloaded(e, man, T, M)
        wp, st_m = mix_dev(e, M, ws, P)
        after = downloaded(e, man, T, M)
        runs.append((m_g, C_g, st_c, wp, st_m, before, after, ws))
        e.close()
    clean, brk = runs
    bad = np.array([UNINIT, NEG, NAN, SUM])
    good = np.setdiff1d(np.arange(T), bad)
    expect = np.zeros(T, dtype=np.int64)
    expect[UNINIT] = spe.ST_UNINITIALISED
    expect[[NEG, NAN, SUM]] = spe.ST_ERR_WEIGHTS
    assert (clean[2] == 0).all() and (clean[4] == 0).all()
    assert np.array_equal(brk[2], expect) and np.array_equal(brk[4], expect)
    # combine: NaN on the failing tracks, the neighbours as in the clean run
    assert np.isnan(brk[0][bad]).all() and np.isnan(brk[1][bad]).all()
    assert np.array_equal(brk[0][good], clean[0][good]) and np.array_equal(brk[1][good], clean[1][good])
    # mix: the failing tracks keep every bit and w_pred = w, the neighbours as in the clean run
    for x_before, x_after in zip(brk[5], brk[6]):
        assert np.array_equal(x_before[bad], x_after[bad], equal_nan=True)
    assert np.array_equal(brk[3][bad], brk[7][bad], equal_nan=True)
    assert np.array_equal(brk[3][good], clean[3][good])
    for x_brk, x_clean in zip(brk[6], clean[6]):
        assert np.array_equal(x_brk[good], x_clean[good])


def test_argument_errors(spe, onp):
    e, man, w = bank_engine(spe, onp, "pose", 6, 2, 0, 0)
    w_t = dev(e, w.reshape(-1)); out = torch.zeros(12 * 13, dtype=torch.float64, device="cuda")
    for M in (1, 9, 5):   # out of range, out of range, capacity 12 % 5 != 0
        with pytest.raises(spe.UkfbError):
            e.bank_combine_dev(M, w_t, out)
    for P in ([[0.5, 0.6], [0.5, 0.5]], [[1.5, -0.5], [0.5, 0.5]], [[np.nan, 1.0], [0.5, 0.5]]):
        with pytest.raises(spe.UkfbError):
            e.bank_mix_dev(2, w_t, np.array(P), out)
    e.close()


# ---------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_weights_against_the_reference(spe, onp, pname, prec, wide, tol):
    T, M = 1001, 4
    e, man, w = bank_engine(spe, onp, "pose", T, M, prec, wide)
    rng = np.random.default_rng(5)
    lw = stored(np.log(w / w.sum(axis=1, keepdims=True)), e.dtype)
    ll = rng.uniform(-30.0, 5.0, (T, M))
    ll[::7] -= 690.0                       # log-likelihoods down to -720
    ll[3::11, 2] = np.nan                  # a dead hypothesis
    ll[5::50] = np.nan                     # every hypothesis of the track dead
    ll = stored(ll, e.dtype)
    t = tdt(e)

    def run(lw_in, ll_in, want_w=True):
        lo = torch.full((T * M,), 7.0, dtype=t, device="cuda")
        wo = torch.full((T * M,), 7.0, dtype=t, device="cuda") if want_w else None
        st = torch.full((T,), 0x7FFF, dtype=torch.int32, device="cuda")
        a = None if lw_in is None else dev(e, lw_in.reshape(-1))
        b = None if ll_in is None else dev(e, ll_in.reshape(-1))
        torch.cuda.synchronize()
        e.bank_weights_dev(M, a, b, lo, wo, st)
        e.sync()
        return (lo.cpu().numpy().astype(np.float64).reshape(T, M),
                wo.cpu().numpy().astype(np.float64).reshape(T, M) if want_w else None, st.cpu().numpy().astype(np.int64), wo)

    for lw_in, ll_in in ((lw, ll), (None, ll), (lw, None)):
        lo, wo, st, wo_t = run(lw_in, ll_in)
        lo_r, wo_r, dead = br.weights(lw_in, ll_in)
        assert np.array_equal(st, np.where(dead, spe.ST_ERR_WEIGHTS, 0))
        assert np.array_equal(np.isneginf(lo), np.isneginf(lo_r)) and np.array_equal(wo == 0, wo_r == 0)
        fin = np.isfinite(lo_r)
        el, ew = scaled(lo[fin], lo_r[fin]), scaled(wo, wo_r)
        print(f"bank parity weights {pname} prior={'yes' if lw_in is not None else 'no'} loglik={'yes' if ll_in is not None else 'no'}: "
              f"logw {el:.3e} w {ew:.3e} max|sum w - 1| {np.abs(wo.sum(axis=1) - 1).max():.3e}")
        assert el <= tol and ew <= tol
        # by construction a distribution within the bound combine / mix enforce: fed straight in
        st_t = torch.full((T,), 0x7FFF, dtype=torch.int32, device="cuda")
        mu_t = torch.empty((T, e.S), dtype=t, device="cuda")
        e.bank_combine_dev(M, wo_t, mu_t, None, st_t)
        e.sync()
        assert (st_t.cpu().numpy() == 0).all()
    assert np.array_equal(run(lw, ll, want_w=False)[0], run(lw, ll)[0])
    e.close()


# ---------------------------------------------------------------------------------------------------------------- IMM run
def imm_inputs(spe, onp, T, cycles, dt):
    mu0, cov0 = spe.synth.pose_initial(T)
    vel = onp.quat_rotate(mu0[:, 3:7], mu0[:, 7:10])
    jump = np.array([1.0, -1.0, 0.0])
    z = np.array([mu0[:, :3] + (c + 1) * dt * vel + (jump if c >= 10 else 0.0) for c in range(cycles)])
    Q = np.tile(0.05 ** 2 * np.eye(3), (2 * T, 1, 1))
    R = spe.synth.pose_default_process_noise()
    return np.repeat(mu0, 2, axis=0), np.repeat(cov0, 2, axis=0), np.repeat(z, 2, axis=1), Q, np.array([R, 100.0 * R] * T)


def imm_reference(onp, mu, cov, z, Q, R, P, cycles, dt, store=np.float64):
    """the IMM chain in NumPy float64 arithmetic; `store`: the number format in which the engine's arrays hold every launch's
    results (float64: the reference proper; float32: its instantiation with fp32 storage, the rounding an fp32 engine cannot avoid)"""
    r = lambda x: np.asarray(x, dtype=store).astype(np.float64)
    T = mu.shape[0] // 2
    w = np.full((T, 2), 0.5)
    out = []
    for c in range(cycles):
        m3, c3, wp, _ = br.mix(onp.POSE, mu.reshape(T, 2, 13), cov.reshape(T, 2, 12, 12), w, P)
        mu, cov, wp = r(m3.reshape(2 * T, 13)), r(c3.reshape(2 * T, 12, 12)), r(wp)
        mu, cov, st = onp.pose_predict(mu, cov, R, None, np.eye(3), dt)
        assert (st == 0).all()
        mu, cov = r(mu), r(cov)
        S = cov[:, :3, :3] + Q
        nu = z[c] - mu[:, :3]
        d2 = np.einsum("bi,bij,bj->b", nu, np.linalg.inv(S), nu)
        ll = r(-0.5 * (d2 + np.log(np.linalg.det(S)) + 3 * LN2PI))
        mu, cov, st = onp.pose_update(mu, cov, 0, z[c], Q)
        assert (st == 0).all()
        mu, cov = r(mu), r(cov)
        with np.errstate(divide="ignore"):
            _, w, _ = br.weights(r(np.log(wp)), ll.reshape(T, 2))
        w = r(w)
        m, C, _ = br.mixture(onp.POSE, mu.reshape(T, 2, 13), cov.reshape(T, 2, 12, 12), w)
        out.append((r(m), r(C), w))
    return out


@pytest.mark.parametrize("pname,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_imm_run_end_to_end(spe, onp, pname, prec, wide, tol):
    """2 048 tracks x (quiet, manoeuvring) PoseWithVelocity hypotheses, 20 IMM cycles with a position fix that jumps at cycle 10"""
    T, M, cycles, dt = 2048, 2, 20, 0.1
    P = np.array([[0.95, 0.05], [0.05, 0.95]])
    mu, cov, z, Q, R = imm_inputs(spe, onp, T, cycles, dt)
    e = new_engine(spe, "pose", T * M, prec, wide)
    e.initialize(mu, cov)
    e.set_process_noise(R)
    # the reference starts from the state, noise and samples as the engine's arrays hold them
    mu_s, cov_s, _ = e.state()
    z_s, Q_s, R_s = stored(z, e.dtype), stored(Q, e.dtype), stored(R, e.dtype)
    ref = imm_reference(onp, mu_s, cov_s, z_s, Q_s, R_s, P, cycles, dt)
    # How many cycles the storage format itself holds the gate: the same chain, float64 arithmetic, every launch's results
    # rounded to the engine's storage format, against the reference proper.  The engine is held to the gate for these cycles.
    ref_st = imm_reference(onp, mu_s, cov_s, z_s, Q_s, R_s, P, cycles, dt, store=e.dtype)
    fmt = [max(scaled(a[0], b[0]), scaled(a[1], b[1]), scaled(a[2], b[2])) for a, b in zip(ref_st, ref)]
    held = next((c for c, v in enumerate(fmt) if v > tol), cycles)
    print(f"bank parity imm {pname}: the reference with {np.dtype(e.dtype).name} storage holds {tol:.3e} for {held} of {cycles} cycles "
          f"(its own error per cycle: {' '.join(f'{v:.2e}' for v in fmt)})")
    assert held >= 1
    t = tdt(e)
    w = torch.full((T * M,), 0.5, dtype=t, device="cuda")
    wp, logw, ll = torch.empty_like(w), torch.empty_like(w), torch.empty((1, T * M), dtype=t, device="cuda")
    mu_o = torch.empty((T, 13), dtype=t, device="cuda"); cov_o = torch.empty((T, 78), dtype=t, device="cuda")
    st = torch.zeros((T,), dtype=torch.int32, device="cuda")
    Q_t = dev(e, Q_s.reshape(-1, 9))
    worst = [0.0, 0.0, 0.0]
    p_man, p_man_ref, late = [], [], []
    for c in range(cycles):
        z_t = dev(e, z_s[c][None])
        torch.cuda.synchronize()
        wp, _ = e.bank_mix_dev(M, w, P)          # the allocating form of the binding
        e.predict(dt)
        e.innovation_dev(spe.MEAS_POS3, 1, z_t, Q_t, loglik=ll)
        e.update_dev(spe.MEAS_POS3, z_t, Q_t)
        e.sync()
        lwp = torch.log(wp)
        torch.cuda.synchronize()
        e.bank_weights_dev(M, lwp, ll, logw, w)
        e.bank_combine_dev(M, w, mu_o, cov_o, st)
        e.sync()
        assert e.status_summary() == 0 and (st.cpu().numpy() == 0).all()
        m_r, C_r, w_r = ref[c]
        errs = (scaled(mu_o.cpu().numpy().astype(np.float64), m_r),
                scaled(unpack(cov_o.cpu().numpy().astype(np.float64), 12), C_r),
                scaled(w.cpu().numpy().astype(np.float64).reshape(T, 2), w_r))
        worst = [max(a, b) for a, b in zip(worst, errs)]
        print(f"bank parity imm {pname} cycle {c:2d}: mean {errs[0]:.3e} cov {errs[1]:.3e} weights {errs[2]:.3e}")
        if pname == "f64" and c in (0, cycles - 1):   # a chain of launches: the fp64 bound needs no count of roundings
            fsp.judge_state(f"bank/pose/f64/imm/cycle={c}", "pose", "f64", mu_o.cpu().numpy(), unpack(cov_o.cpu().numpy().astype(np.float64), 12),
                            m_r, C_r)
        if c < held and max(errs) > tol:
            late.append((c, errs))
        p_man.append(float(w.cpu().numpy().astype(np.float64).reshape(T, 2)[:, 1].mean()))
        p_man_ref.append(float(w_r[:, 1].mean()))
    print(f"bank parity imm {pname} worst: mean {worst[0]:.3e} cov {worst[1]:.3e} weights {worst[2]:.3e}; "
          f"P(manoeuvre) cycle 9 / 12: engine {p_man[9]:.4f} / {p_man[12]:.4f}, reference {p_man_ref[9]:.4f} / {p_man_ref[12]:.4f}")
    assert late == [], f"cycles outside the gate {tol:.3e}: {late}"
    assert p_man[12] > p_man[9] and p_man_ref[12] > p_man_ref[9]
    e.close()
