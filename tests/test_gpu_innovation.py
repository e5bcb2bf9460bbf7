"""Innovation statistics without an update (ukfb_innovation_dev / ukfb_select_candidates_dev / ukfb_innovation,
include/ukf_batch.h): predicted measurement, S, innovation, squared Mahalanobis distance and log-likelihood of up to 32 candidate
samples per filter, and the nearest candidate inside the gate.

The reference is computed here with the NumPy oracle on the state DOWNLOADED from the engine (for fp32 engines that takes the storage
rounding of the state out of the comparison):
    X, ok = sigma_points(man, mu, sigma);  Z = h(X);  mz, conv = mean_sigma_points(manz, Z)
    S = cov_sigma_points(manz, mz, Z) + Q;  nu_k = manz.boxminus(z_k, mz);  d2_k = nu_k^T S^-1 nu_k
Parity bound: |x - ref| <= tol (1 + |ref|), tol = the README's parity gates 1e-9 (fp64) / 1e-4 (fp32); fp32 engines with
wide_arithmetic compute in fp64 and store fp32: 1e-9 + 2^-23 (one fp32 rounding of the stored value).  The per-model maxima that
were measured on an MI355X are in profiles/innovation_parity.txt.

Every parity comparison also makes the SCALED one (tests/feature_scaled_parity.py): z-bar, S and nu whitened by
s^z_i = sqrt(S_ref[i, i]) -- |dS|_ij / (s^z_i s^z_j), |d nu_i| / s^z_i, |(z-bar (-) z-bar_ref)_i| / s^z_i with SO(3)'s own (-) for
model 3 -- and held per output: fp64 1e-9; wide_arithmetic 2 u v + 1e-9 (v = 1 for S, |nu_i| / s^z_i, max(1, |z-bar_i|) / s^z_i, 2 / s^z_i for
a rotation coordinate); plain fp32 max(M_feat d_32, 20 u v), d_32 the distance of the all-float32 evaluation of the same call
(tests/feature_f32.py) from its float64 evaluation on the same batch.  It prints one SCALED line.  d^2 and the log-likelihood are
dimensionless (or offset by logdet) and stay on the bound above.
"""
import numpy as np
import pytest
import torch

import feature_f32 as ff
import feature_scaled_parity as fsp
from engine_support import scaled, stored, tdt
from innovation_reference import K, POSE_MODELS, clutter, reference, reference_scores

pytestmark = pytest.mark.gpu

N = 4096
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]


# ---------------------------------------------------------------------------------------------------------------- helpers
def make_engine(spe, kind, n, prec, wide, **cfg):
    """an engine after one predict of the bench workload"""
    sy = spe.synth
    if wide:
        cfg["wide_arithmetic"] = 1
    if kind == "pose":
        mu, cov = sy.pose_initial(n)
        acc, _, Q = sy.pose_cycle_inputs(n, 0, mu[:, :3], random_q=True)
        e = spe.BatchPoseUKF(n, precision=prec, **cfg)
        e.initialize(mu, cov)
        e.set_process_noise(sy.pose_default_process_noise())
        e.set_acceleration(acc, 0.01 * np.eye(3))
    else:
        mu, cov = sy.orient_initial(n)
        gyro, acc, _, Q = sy.orient_cycle_inputs(n, 0, mu[:, :4])
        G = sy.uniform(sy.SEED_BASE + 9, np.arange(n), np.arange(9), -1.0, 1.0).reshape(n, 3, 3)
        Q = 0.05 ** 2 * (np.eye(3)[None] + 0.3 * (G @ np.swapaxes(G, 1, 2)) / 3.0)
        Q = 0.5 * (Q + np.swapaxes(Q, 1, 2))
        e = spe.BatchOrientationUKF(n, sy.ORIENT_TAU, sy.ORIENT_TAU, sy.ORIENT_LATITUDE, precision=prec, **cfg)
        e.initialize(mu, cov)
        e.set_process_noise(sy.orient_process_noise())
        e.set_orient_inputs(gyro, acc)
    e.predict(0.01)
    assert e.status_summary() == 0
    return e, Q


def run_innovation(e, model, z, Q, uniform_q=False, want=("z_pred", "S", "innov", "maha", "loglik", "best", "status")):
    """model: an id or an int32 array of per-filter ids; z [K, n, 3]; Q [n, 3, 3] or [3, 3] (uniform_q)"""
    n, k = e.capacity, z.shape[0]
    t = tdt(e)
    z_t = torch.from_numpy(np.ascontiguousarray(z)).to("cuda", t)
    Q_t = torch.from_numpy(np.ascontiguousarray(Q).reshape(-1)).to("cuda", t)
    shapes = {"z_pred": (n, 4), "S": (n, 9), "innov": (k, n, 3), "maha": (k, n), "loglik": (k, n)}
    bufs = {name: torch.full(shapes[name], 7.0, dtype=t, device="cuda") for name in shapes if name in want}
    if "best" in want:
        bufs["best"] = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    if "status" in want:
        bufs["status"] = torch.full((n,), 0x7FFF, dtype=torch.int32, device="cuda")
    m_t = None if np.isscalar(model) else torch.from_numpy(np.ascontiguousarray(model, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    e.innovation_dev(int(model) if np.isscalar(model) else 0, k, z_t, Q_t, q_is_uniform=uniform_q, meas_model_dev=m_t, **bufs)
    e.sync()
    out = {name: b.cpu().numpy().astype(np.float64 if name not in ("best", "status") else np.int64) for name, b in bufs.items()}
    if "S" in out:
        out["S"] = out["S"].reshape(n, 3, 3)
    out["_z_t"], out["_Q_t"], out["_m_t"], out["_best_t"] = z_t, Q_t, m_t, bufs.get("best")
    return out


def compare(onp, kind, mid, out, sel, mu, cov, Q, z, judged):
    """scaled errors of the five float outputs for the filters `sel` (one model id), and the reference d2; judged = (name,
    precision name): z-bar, S and nu are also held to the scale of S (tests/feature_scaled_parity.py), before this returns"""
    m, manz, mz, S, ok, conv = reference(onp, kind, mid, mu[sel], cov[sel], Q[sel])
    assert ok.all() and conv.all()
    so3 = kind == "pose" and mid == 3
    nu, d2, ll = reference_scores(onp, so3, m, manz, mz, S, z[:, sel])
    zp = out["z_pred"][sel]
    if so3:   # a quaternion and its negative are the same rotation
        sign = np.sign(np.sum(zp * mz, axis=-1, keepdims=True))
        err_z = scaled(zp * sign, mz)
    else:
        err_z = max(scaled(zp[:, :m], mz), float(np.abs(zp[:, m:]).max()))
    Sp = np.zeros((len(S), 3, 3)); Sp[:, :m, :m] = S
    errs = {"z_pred": err_z, "S": scaled(out["S"][sel], Sp), "innov": scaled(out["innov"][:, sel, :m], nu),
            "maha": scaled(out["maha"][:, sel], d2), "loglik": scaled(out["loglik"][:, sel], ll)}
    fsp.judge_meas(judged[0], judged[1], zp if so3 else zp[:, :m], out["S"][sel][:, :m, :m], out["innov"][:, sel, :m], mz, S, nu, so3,
                   f32=lambda: tuple(ff.innovation_stats(kind, mid, mu[sel], cov[sel], Q[sel], z[:, sel], p) for p in ("f32", "f64")))
    return errs, d2


def gate_for(kind, mid):
    m = 3 if kind == "orient" else {0: 3, 1: 2, 2: 1, 3: 3, 4: 3, 5: 2, 6: 1, 7: 2, 8: 3}[mid]
    return 7.81 if m >= 2 else 3.84


def check_best(best, d2, gate):
    """the engine's choice against the reference's argmin inside the gate; returns the number of filters left out (reference
    decisions closer than 1e-3 (1 + .) to a tie or to the gate)"""
    srt = np.sort(d2, axis=0)
    ambiguous = (srt[1] - srt[0] < 1e-3 * (1.0 + srt[0])) | (np.abs(d2 - gate) < 1e-3 * (1.0 + gate)).any(axis=0)
    ref = np.where(srt[0] <= gate, np.argmin(d2, axis=0), -1)
    keep = ~ambiguous
    assert (best[keep] == ref[keep]).all(), np.nonzero(keep & (best != ref))[0][:10]
    return int(ambiguous.sum())


# ------------------------------------------------------------------------------------------- 1 + 3: parity, random clutter
@pytest.mark.parametrize("name,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("kind", ["pose", "orient"])
def test_parity_every_model_and_clutter_association(spe, onp, kind, name, prec, wide, tol):
    """Tests 1 and 3 of the issue: every measurement model with a uniform id, per-filter and uniform Q; `best` against the
    reference's choice with at most 5 % of the filters left out."""
    models = POSE_MODELS if kind == "pose" else [9]
    e, Q = make_engine(spe, kind, N, prec, wide)
    mu, cov, _ = e.state()
    worst = {}
    for mid in models:
        gate = gate_for(kind, mid)
        e.configure(gate_chi2=gate)
        z = clutter(onp, spe, kind, mid, mu)
        for uniform_q in (False, True):
            Qh = np.broadcast_to(Q[0], Q.shape).copy() if uniform_q else Q
            out = run_innovation(e, mid, z, Q[0] if uniform_q else Q, uniform_q=uniform_q)
            assert (out["status"] == 0).all()
            errs, d2 = compare(onp, kind, mid, out, np.arange(N), mu, cov, stored(Qh, e.dtype), stored(z, e.dtype),
                                   (f"innovation/{kind}/{name}/model={mid}/uniform_q={int(uniform_q)}", name))
            left_out = check_best(out["best"], d2, float(np.float32(gate)) if prec == 1 else gate)
            print(f"innovation parity {kind} {name} model={mid} uniform_q={int(uniform_q)} "
                  + " ".join(f"{k}={v:.3e}" for k, v in errs.items()) + f" best_left_out={left_out}")
            assert left_out <= 0.05 * N
            for k, v in errs.items():
                worst[(mid, k)] = max(worst.get((mid, k), 0.0), v)
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, (tol, bad)
    e.close()


@pytest.mark.parametrize("name,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
def test_parity_per_filter_model_ids(spe, onp, name, prec, wide, tol):
    """per-filter ids (synth.pose_mixed_models: the nine Pose models, a quarter of the filters without one)"""
    e, Q = make_engine(spe, "pose", N, prec, wide, gate_chi2=7.81)
    mu, cov, _ = e.state()
    models = spe.synth.pose_mixed_models(N, 0)
    z = np.zeros((K, N, 3))
    for mid in POSE_MODELS:
        sel = models == mid
        z[:, sel] = clutter(onp, spe, "pose", mid, mu)[:, sel]
    out = run_innovation(e, models, z, Q)
    off = models < 0
    assert off.any() and (out["status"][off] == onp.ST_INACTIVE).all() and (out["status"][~off] == 0).all()
    assert (out["best"][off] == -1).all()
    assert np.isnan(out["z_pred"][off]).all() and np.isnan(out["S"][off]).all() and np.isnan(out["innov"][:, off]).all()
    assert np.isnan(out["maha"][:, off]).all() and np.isnan(out["loglik"][:, off]).all()
    worst = {}
    for mid in POSE_MODELS:
        sel = np.nonzero(models == mid)[0]
        errs, _ = compare(onp, "pose", mid, out, sel, mu, cov, stored(Q, e.dtype), stored(z, e.dtype), (f"innovation/pose/{name}/mixed-ids/model={mid}", name))
        print(f"innovation parity pose-mixed {name} model={mid} " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
        for k, v in errs.items():
            worst[(mid, k)] = v
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, (tol, bad)
    e.close()


# --------------------------------------------------------------------------------- 2: constructed candidates, exact decisions
@pytest.mark.parametrize("name,prec,wide,tol", PRECS[:2], ids=["f64", "f32"])
@pytest.mark.parametrize("kind,mid", [("pose", 0), ("pose", 3), ("orient", 9)])
def test_constructed_candidates_select_and_update(spe, oracle, onp, kind, mid, name, prec, wide, tol):
    """z_k = z-bar [+] c_k chol(S) u_k, |u_k| = 1, c = (0.5, 2, 3.5, 5) rotated by i % 4 (every eighth filter: c x 6), gate 6.0:
    `best` equals the reference's choice for EVERY filter; select + update_dev equals the oracle's update with that candidate;
    filters without an accepted candidate are bit-identical and INACTIVE; the existing update's gate rejects exactly the
    filters with maha[k] > 6."""
    n = N
    e, Q = make_engine(spe, kind, n, prec, wide, gate_chi2=6.0)
    mu, cov, _ = e.state()
    Qs = stored(Q, e.dtype)
    m, manz, mz, S, ok, conv = reference(onp, kind, mid, mu, cov, Qs)
    assert ok.all() and conv.all() and m == 3
    L = np.linalg.cholesky(S)
    u = spe.synth.uniform(spe.synth.SEED_BASE + 31, np.arange(n), np.arange(3 * K), -1.0, 1.0).reshape(n, K, 3)
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    c = np.array([0.5, 2.0, 3.5, 5.0])
    so3 = kind == "pose" and mid == 3
    z = np.empty((K, n, 3))
    for k in range(K):
        ck = c[(k + np.arange(n)) % 4] * np.where(np.arange(n) % 8 == 7, 6.0, 1.0)
        d = np.einsum("bij,bj->bi", L, u[:, k]) * ck[:, None]
        zk = manz.boxplus(mz, d)
        z[k] = onp.so3_log(zk) if so3 else zk
    zs = stored(z, e.dtype)
    nu, d2, _ = reference_scores(onp, so3, m, manz, mz, S, zs)
    ref_best = np.where(d2.min(axis=0) <= 6.0, np.argmin(d2, axis=0), -1)
    assert (ref_best[7::8] == -1).all() and (ref_best[np.arange(n) % 8 != 7] >= 0).all()
    out = run_innovation(e, mid, z, Q)
    assert (out["status"] == 0).all()
    assert (out["best"] == ref_best).all(), np.nonzero(out["best"] != ref_best)[0][:10]

    # the tie to the existing gate, on a copy of the engine (same stored state)
    e2 = (spe.BatchPoseUKF(n, precision=prec, gate_chi2=6.0) if kind == "pose" else
          spe.BatchOrientationUKF(n, spe.synth.ORIENT_TAU, spe.synth.ORIENT_TAU, spe.synth.ORIENT_LATITUDE, precision=prec, gate_chi2=6.0))
    for k in (1, 2):
        e2.initialize(mu, cov)
        e2.update_dev(mid, out["_z_t"][k], out["_Q_t"])
        rejected = (e2.status() & onp.ST_REJECTED_GATE) != 0
        assert (rejected == (out["maha"][k] > 6.0)).all()
    e2.close()

    # association on the device: select, then the existing update
    z_sel = torch.full((n, 3), 9.0, dtype=tdt(e), device="cuda")
    m_sel = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.select_candidates_dev(K, out["_best_t"], mid, out["_z_t"], z_sel, m_sel)
    e.update_dev(0, z_sel, out["_Q_t"], meas_model_dev=m_sel)
    e.sync()
    st = e.status()
    none = ref_best < 0
    assert (m_sel.cpu().numpy() == np.where(none, -1, mid)).all()
    assert (st[none] == onp.ST_INACTIVE).all() and (st[~none] == 0).all()
    mu2, cov2, _ = e.state()
    assert np.array_equal(mu2[none], mu[none]) and np.array_equal(cov2[none], cov[none])
    z_ref = zs[np.maximum(ref_best, 0), np.arange(n)]
    if kind == "pose":
        m_o, c_o, st_o = onp.pose_update(mu[~none], cov[~none], mid, z_ref[~none], Qs[~none])
    else:
        m_o, c_o, st_o = onp.orient_update(mu[~none], cov[~none], z_ref[~none], Qs[~none])
    assert (st_o == 0).all()
    em, ec = np.abs(mu2[~none] - m_o).max(), np.abs(cov2[~none] - c_o).max()
    print(f"association {kind} model={mid} {name}: max|dmu|={em:.3e} max|dcov|={ec:.3e}")
    assert em <= tol and ec <= tol
    e.close()


# ----------------------------------------------------------------------------------------------------------- 4: read-only
@pytest.mark.parametrize("name,prec,wide,tol", PRECS, ids=[p[0] for p in PRECS])
@pytest.mark.parametrize("kind,mid", [("pose", 0), ("pose", 3), ("orient", 9)])
def test_read_only(spe, onp, kind, mid, name, prec, wide, tol):
    n = 1024
    e, Q = make_engine(spe, kind, n, prec, wide, gate_chi2=7.81)
    e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000)
    t = tdt(e)
    mu_d, cov_d, st_d = e.device_views()

    def snapshot():
        e.sync()
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        outs = []
        for ptr, nbytes in ((mu_d, n * e.S * np.dtype(e.dtype).itemsize), (cov_d, n * e.PK * np.dtype(e.dtype).itemsize), (st_d, n * 4)):
            buf = (ctypes.c_ubyte * nbytes)()
            assert hip.hipMemcpy(buf, ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0
            outs.append(bytes(buf))
        latch = e.rotation_rate().tobytes() if kind == "orient" else b""
        return outs, e.last_measurement_time().tobytes(), latch

    mu, _, _ = e.state()
    a = snapshot()
    out = run_innovation(e, mid, clutter(onp, spe, kind, mid, mu), Q)
    assert (out["status"] == 0).all()
    b = snapshot()
    assert a == b
    # the latched inputs as well: the next prediction is the one an untouched twin makes
    twin, _ = make_engine(spe, kind, n, prec, wide, gate_chi2=7.81)
    twin.predict(0.01); e.predict(0.01)
    m1, c1, _ = e.state(); m2, c2, _ = twin.state()
    assert np.array_equal(m1, m2) and np.array_equal(c1, c2)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------ 5: statuses
def test_statuses_and_argument_errors(spe, onp):
    n = 8
    mu, cov = spe.synth.pose_initial(n)
    _, z1, Q = spe.synth.pose_cycle_inputs(n, 0, mu[:, :3])
    bad = cov.copy()
    bad[2, 1, 1] = -1.0     # S = Sigma[0:3, 0:3] + Q of the position models is not positive definite
    bad[3, 5, 5] = -1.0     # not factorisable in the six columns the orientation measurement reads; the position block is fine
    e = spe.BatchPoseUKF(n, gate_chi2=7.81)
    e.initialize(mu[:7], bad[:7])                    # filter 7 never initialised
    z = np.array([z1, z1 + 0.01, z1 + 0.02])
    z[0, 4, 1] = np.nan                               # one candidate of filter 4
    z[:, 5, 2] = np.inf                               # every candidate of filter 5
    models = np.full(n, 0, dtype=np.int32); models[6] = -1; models[0] = 9   # 9 is not a Pose model: inactive
    own_status = e.status()
    out = run_innovation(e, models, z, Q)
    st = out["status"]
    assert st[0] == onp.ST_INACTIVE and st[6] == onp.ST_INACTIVE and st[7] == onp.ST_UNINITIALISED
    assert st[2] == onp.ST_ERR_CHOLESKY and st[1] == 0 and st[3] == 0 and st[4] == 0 and st[5] == onp.ST_ERR_NONFINITE_MEAS
    for f in (0, 2, 6, 7):
        assert out["best"][f] == -1
        assert np.isnan(out["z_pred"][f]).all() and np.isnan(out["S"][f]).all() and np.isnan(out["maha"][:, f]).all()
        assert np.isnan(out["loglik"][:, f]).all() and np.isnan(out["innov"][:, f]).all()
    assert np.isnan(out["maha"][0, 4]) and np.isnan(out["loglik"][0, 4]) and np.isnan(out["innov"][0, 4]).all()
    assert np.isfinite(out["maha"][1:, 4]).all() and out["best"][4] == 1 + int(np.argmin(out["maha"][1:, 4]))
    assert np.isfinite(out["maha"][:, 1]).all() and out["maha"][:, 1].min() <= 7.81 and out["best"][1] == int(np.argmin(out["maha"][:, 1]))
    assert out["best"][5] == -1 and np.isnan(out["maha"][:, 5]).all() and np.isfinite(out["S"][5]).all()
    out3 = run_innovation(e, spe.MEAS_ORIENT_SO3, np.zeros((1, n, 3)), Q)
    assert out3["status"][3] == onp.ST_ERR_CHOLESKY and out3["status"][1] == 0 and out3["status"][7] == onp.ST_UNINITIALISED
    # the engine's own status array is not the call's
    assert np.array_equal(e.status(), own_status)
    # argument errors
    zt, Qt, bt = out["_z_t"], out["_Q_t"], out["_best_t"]
    lib, h = e._lib, e._h
    import ctypes as C
    o = spe.engine.InnovationOut(None, None, None, None, None, bt.data_ptr(), None)
    call = lambda model, k, out_: lib.ukfb_innovation_dev(h, C.c_int(model), None, C.c_int(k), C.c_void_p(zt.data_ptr()),
                                                          C.c_void_p(Qt.data_ptr()), C.c_int(0), out_)
    assert call(0, 3, C.byref(o)) == 0
    e.sync()
    assert call(9, 3, C.byref(o)) == 5            # UKFB_ERR_WRONG_MODEL: an OrientationState model on a Pose engine
    assert call(0, 0, C.byref(o)) == 1 and call(0, 33, C.byref(o)) == 1   # UKFB_ERR_INVALID_ARG
    assert call(0, 3, None) == 1
    assert call(0, 3, C.byref(spe.engine.InnovationOut())) == 1
    with pytest.raises(spe.UkfbError):
        e.select_candidates_dev(0, bt, 0, zt, zt)
    # host-array form
    ho = e.innovation(0, z, Q)
    assert (ho["status"][[1, 4]] == 0).all() and ho["status"][7] == onp.ST_UNINITIALISED and ho["best"][1] == out["best"][1]
    out_u = run_innovation(e, 0, z, Q)
    assert np.array_equal(ho["maha"][:, 1], out_u["maha"][:, 1]) and np.array_equal(ho["S"][1], out_u["S"][1])
    e.close()
    # OrientationState: an indefinite covariance, a non-finite candidate
    s = spe.synth
    mo, co = s.orient_initial(4)
    co[2, 4, 4] = -1.0
    eo = spe.BatchOrientationUKF(4, s.ORIENT_TAU, s.ORIENT_TAU, s.ORIENT_LATITUDE)
    eo.initialize(mo, co)
    zz = np.zeros((2, 4, 3)); zz[1, 1, 0] = np.nan
    oo = run_innovation(eo, 9, zz, np.broadcast_to(0.01 * np.eye(3), (4, 3, 3)).copy())
    assert list(oo["status"]) == [0, 0, onp.ST_ERR_CHOLESKY, 0] and oo["best"][2] == -1 and oo["best"][1] == 0 and oo["best"][0] == 0
    assert np.isnan(oo["maha"][1, 1]) and np.isfinite(oo["maha"][0, 1])
    eo.close()


@pytest.mark.parametrize("name,prec,wide,tol", PRECS[1:], ids=["f32", "f32w"])
@pytest.mark.parametrize("kind,mid", [("pose", 0), ("orient", 9)])
def test_host_array_form_fp32(spe, onp, kind, mid, name, prec, wide, tol):
    """fp32 engines: ukfb_innovation narrows the host doubles itself; every output is the bits of the device form fed the same
    values rounded to float32.  Five filters (one full wavefront and a one-row tail), two candidates."""
    n = 5
    e, Q = make_engine(spe, kind, n, prec, wide, gate_chi2=7.81)
    mu, _, _ = e.state()
    z = clutter(onp, spe, kind, mid, mu)[:2]
    assert not np.array_equal(z, stored(z, e.dtype)) and not np.array_equal(Q, stored(Q, e.dtype))   # doubles that are NOT fp32 values
    ho = e.innovation(mid, z, Q)
    out = run_innovation(e, mid, stored(z, e.dtype), stored(Q, e.dtype))
    assert (ho["status"] == 0).all() and np.isfinite(ho["maha"]).all()
    for key in ("z_pred", "S", "innov", "maha", "loglik", "best", "status"):
        assert np.array_equal(ho[key], out[key]), key
    e.close()


def test_thirty_two_candidates_and_ties(spe, onp):
    """two passes of the sixteen lanes; equal distances keep the lower index"""
    n, k = 70, 32
    e, Q = make_engine(spe, "pose", n, 0, 0)
    mu, cov, _ = e.state()
    base = clutter(onp, spe, "pose", 0, mu)          # 4 candidates
    z = np.array([base[j % 4] + 0.01 * (j // 4) for j in range(k)])
    z[20] = z[3]; z[9] = z[3]                         # a three-way tie between candidates 3, 9 and 20
    out = run_innovation(e, 0, z, Q)
    m, manz, mz, S, ok, conv = reference(onp, "pose", 0, mu, cov, Q)
    _, d2, _ = reference_scores(onp, False, m, manz, mz, S, z)
    assert scaled(out["maha"], d2) <= 1e-9
    assert np.array_equal(out["maha"][3], out["maha"][9]) and np.array_equal(out["maha"][3], out["maha"][20])
    expect = np.argmin(out["maha"], axis=0)           # (NumPy's argmin returns the first minimum)
    assert (out["best"] == expect).all() and (out["best"] != 9).all() and (out["best"] != 20).all()
    e.close()


# ---------------------------------------------------------------------------------------------------------- 6: NIS sanity
@pytest.mark.parametrize("kind,mid,prec", [("pose", 0, 0), ("pose", 3, 1), ("pose", 6, 0), ("orient", 9, 1)])
def test_nis_mean(spe, onp, kind, mid, prec):
    """z = z-bar + chol(S) n, n standard normal: the batch mean of maha lies within 4 sqrt(2 m / N) of m"""
    n = 65536
    e, Q = make_engine(spe, kind, n, prec, 0)
    mu, cov, _ = e.state()
    m, manz, mz, S, ok, conv = reference(onp, kind, mid, mu, cov, stored(Q, e.dtype))
    rng = np.random.default_rng(20240607)
    d = np.einsum("bij,bj->bi", np.linalg.cholesky(S), rng.standard_normal((n, m)))
    zk = manz.boxplus(mz, d)
    z = np.zeros((1, n, 3))
    z[0, :, :m] = onp.so3_log(zk) if (kind == "pose" and mid == 3) else zk
    out = run_innovation(e, mid, z, Q, want=("maha", "status"))
    assert (out["status"] == 0).all()
    mean = float(out["maha"][0].mean())
    print(f"NIS {kind} model={mid} prec={prec}: mean={mean:.4f} expected {m} +- {4 * np.sqrt(2 * m / n):.4f}")
    assert abs(mean - m) <= 4.0 * np.sqrt(2.0 * m / n)
    e.close()
