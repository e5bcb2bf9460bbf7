"""Pins tests/bank_reference.py, the NumPy statement of the filter-bank definitions (include/ukf_batch.h, "filter banks"), on the
CPU: the yardstick of tests/test_gpu_bank.py must itself be right."""
import numpy as np
import pytest

import bank_reference as br


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_closed_form_transport_against_central_differences(spe, onp, model):
    man, mu, cov, w = br.make_tracks(spe, onp, model, 64, 4)
    mean, _, conv = br.mixture(man, mu, cov, w)
    assert conv.all()
    D, ro, h = man.D, br.rot_offset(man), 1e-5
    worst = 0.0
    for j in range(4):
        delta = man.boxminus(mu[:, j], mean)
        J = np.broadcast_to(np.eye(D), (64, D, D)).copy()
        J[:, ro:ro + 3, ro:ro + 3] = br.jr_inv(delta[:, ro:ro + 3])
        for k in range(D):
            e = np.zeros(D); e[k] = h
            col = (man.boxminus(man.boxplus(mu[:, j], e), mean) - man.boxminus(man.boxplus(mu[:, j], -e), mean)) / (2 * h)
            worst = max(worst, np.abs(col - J[:, :, k]).max())
    print("closed form vs central differences:", worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_vector_blocks_are_textbook_moment_matching(spe, onp, model):
    man, mu, cov, w = br.make_tracks(spe, onp, model, 64, 4)
    mean, C, _ = br.mixture(man, mu, cov, w)
    for kind, so, to, n in man.fields:
        if kind == "so3":
            continue
        m = np.einsum("tj,tjk->tk", w, mu[:, :, so:so + n])
        d = mu[:, :, so:so + n] - m[:, None, :]
        Cv = np.einsum("tj,tjab->tab", w, cov[:, :, to:to + n, to:to + n] + d[..., :, None] * d[..., None, :])
        assert np.abs(mean[:, so:so + n] - m).max() <= 1e-14
        assert np.abs(C[:, to:to + n, to:to + n] - Cv).max() <= 1e-14


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_one_hot_identical_and_permuted_hypotheses(spe, onp, model):
    man, mu, cov, w = br.make_tracks(spe, onp, model, 32, 4)
    for j in range(4):
        oh = np.zeros_like(w); oh[:, j] = 1.0
        mean, C, _ = br.mixture(man, mu, cov, oh)
        assert np.array_equal(mean, mu[:, j]) and np.abs(C - cov[:, j]).max() <= 1e-16
        # ... whatever the other hypotheses hold
        mu2 = mu.copy(); mu2[:, (j + 1) % 4] = np.nan
        mean2, C2, _ = br.mixture(man, mu2, cov, oh)
        assert np.array_equal(mean2, mean) and np.array_equal(C2, C)
    same_mu = np.repeat(mu[:, :1], 4, axis=1); same_cov = np.repeat(cov[:, :1], 4, axis=1)
    mean, C, _ = br.mixture(man, same_mu, same_cov, w)
    assert np.array_equal(mean, mu[:, 0]) and np.abs(C - cov[:, 0]).max() <= 1e-16
    perm = np.array([2, 0, 3, 1])
    mean, C, _ = br.mixture(man, mu, cov, w)
    mean_p, C_p, _ = br.mixture(man, mu[:, perm], cov[:, perm], w[:, perm])
    assert np.abs(man.boxminus(mean_p, mean)).max() <= 1e-14 and np.abs(C_p - C).max() <= 1e-14


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_mixture_covariance_is_symmetric_positive_definite_and_transport_matters(spe, onp, model):
    man, mu, cov, w = br.make_tracks(spe, onp, model, 512, 4)
    mean, C, conv = br.mixture(man, mu, cov, w)
    assert conv.all()
    assert np.abs(C - np.swapaxes(C, 1, 2)).max() <= 1e-15
    assert np.linalg.eigvalsh(0.5 * (C + np.swapaxes(C, 1, 2))).min() > 0
    _, C0, _ = br.mixture(man, mu, cov, w, transport=False)
    gap = np.abs(C0 - C) / (1 + np.abs(C))
    print("covariance moved by leaving J out:", gap.max())
    assert gap.max() > 1e-7   # far outside the 1e-9 parity gate: a build without the transport cannot pass


def test_mixing_weights_are_distributions():
    rng = np.random.default_rng(3)
    for M in (2, 3, 8):
        P = rng.uniform(0, 1, (M, M)); P /= P.sum(axis=1, keepdims=True)
        w = rng.uniform(0, 1, (100, M)); w /= w.sum(axis=1, keepdims=True)
        c, wji = br.mixing_weights(w, P)
        assert np.abs(c.sum(axis=1) - 1).max() <= 1e-15 and np.abs(wji.sum(axis=2) - 1).max() <= 1e-15
    # a model nobody can enter: c_i = 0, its row is the one-hot on itself (the hypothesis keeps its state)
    P = np.array([[1.0, 0.0], [1.0, 0.0]])
    c, wji = br.mixing_weights(np.array([[0.3, 0.7]]), P)
    assert c[0, 1] == 0.0 and np.array_equal(wji[0, 1], [0.0, 1.0]) and np.array_equal(wji[0, 0], [0.3, 0.7])


def test_log_sum_exp_with_tiny_likelihoods_and_dead_hypotheses():
    ll = np.array([[-700.0, -701.0, -690.0], [-700.0, np.nan, -700.0], [np.nan, np.nan, np.nan], [-1.0, -2.0, -3.0]])
    lw = np.log(np.array([[0.2, 0.3, 0.5]] * 4))
    logw, w, dead = br.weights(lw, ll)
    assert np.array_equal(dead, [False, False, True, False])
    assert np.abs(w.sum(axis=1) - 1).max() <= 4 * np.finfo(float).eps
    ref0 = np.array([0.2 * np.exp(-10.0), 0.3 * np.exp(-11.0), 0.5]); ref0 /= ref0.sum()
    # logw_in + loglik is rounded at |a| ~ 702 (half an ulp = 5.7e-14 each); the difference of two such sums carries both
    assert np.abs(w[0] - ref0).max() <= 1e-15 and np.abs(logw[0] - np.log(ref0)).max() <= 2.5e-13
    assert w[1, 1] == 0.0 and logw[1, 1] == -np.inf and np.abs(w[1, [0, 2]] - np.array([2, 5]) / 7).max() <= 1e-13   # (same rounding of a)
    assert np.abs(w[2] - [0.2, 0.3, 0.5]).max() <= 1e-15          # every hypothesis dead: the prior, normalised
    assert np.abs(br.weights(None, ll[3:])[1] - np.exp(ll[3]) / np.exp(ll[3]).sum()).max() <= 1e-15
    assert np.abs(br.weights(lw[:1] + 5.0, None)[1] - [0.2, 0.3, 0.5]).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ Jr^-1 against 40 digits
def jr_inv_mp(mp, phi):
    """Jr^-1(phi) = I + [phi]x / 2 + (1 - (theta/2) cot(theta/2)) / theta^2 [phi]x^2 at 40 digits from the exact binary phi"""
    p = [mp.mpf(float(x)) for x in phi]
    th = mp.sqrt(sum(x * x for x in p))
    H = mp.matrix([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
    c = mp.mpf(1) / 12
    if th != 0:
        with mp.extradps(10 + max(0, -2 * int(mp.floor(mp.log10(th))))):   # 1 - (theta/2) cot(theta/2) = theta^2 / 12 + ...
            c = (1 - (th / 2) * mp.cot(th / 2)) / th ** 2
    return mp.eye(3) + H / 2 + c * (H * H)


def test_jr_inv_against_mpmath_up_to_pi():
    """The theta list of test_delayed_reference.test_jr_against_mpmath_at_branch_edges (3.5 and 6.0 lie beyond the range of the
    logarithm, but below the pole of Jr^-1 at 2 pi), extended by the switch to the series and towards and at fl(pi); the Jr
    test's bound, a few roundings per coefficient times [phi]x and [phi]x^2.  (1/t^2 - (1 + cos t) / (2 t sin t), the form this
    replaced, misses it from pi - 1e-3 on and is 75 % wrong at fl(pi).)"""
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng(4)
    pi = float(np.pi)
    thetas = [0.0, 1e-300, 1e-12, 1e-6, 1e-3, np.nextafter(1e-2, 0), 1e-2, 0.3, np.nextafter(0.5, 0), 0.5, np.nextafter(0.5, 1), 0.5 + 1e-9,
              1.0, 2.5, pi - 1e-1, pi - 1e-3, pi - 1e-6, pi - 1e-9, np.nextafter(np.nextafter(pi, 0), 0), np.nextafter(pi, 0), pi,
              np.nextafter(pi, 4), np.nextafter(np.nextafter(pi, 4), 4), 3.5, 6.0]
    worst = 0.0
    with mp.workdps(40):
        for th in thetas:
            dirs = [d / np.linalg.norm(d) for d in rng.normal(size=(4, 3))] + [np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.0])]
            for d in dirs:
                phi = th * d
                got, ref = br.jr_inv(phi), jr_inv_mp(mp, phi)
                err = float(max(abs(mp.mpf(float(got[i, j])) - ref[i, j]) for i in range(3) for j in range(3)))
                worst = max(worst, err / (2.0 ** -52 * (1.0 + th * th)))
                assert np.isfinite(got).all() and err <= 8 * 2.0 ** -52 * (1.0 + th * th), (th, err)
    print(f"BANK Jr^-1 against mpmath at 40 digits: largest error {worst:.2f} eps (1 + theta^2)")
    # batched, as the references call it
    P = np.array([[pi, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1e-3, 0.0]])
    assert np.array_equal(br.jr_inv(P), np.stack([br.jr_inv(p) for p in P]))
