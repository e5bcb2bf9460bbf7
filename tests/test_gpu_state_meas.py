"""Joint state-block measurements on the device (ukfb_update_state_dev / ukfb_update_state / ukfb_pose_update_body_states,
include/ukf_batch.h).

States: synth.pose_initial / orient_initial after two real cycles, so that the covariances are not block-diagonal.  Inputs:
z = mu (+) L xi, Qz = Sigma + (L A)(L A)^T with L = chol(Sigma), A = 0.3 N(0, 1) entries, fixed seeds; both rounded to the
engine's storage.  The reference is tests/state_meas_reference.py (pinned by tests/test_state_meas_reference.py) run on the
state AS DOWNLOADED and the inputs AS STORED.  Parity bound: |x - ref| <= tol (1 + |ref|), tol = 1e-9 (fp64) / 1e-4 (fp32) /
1e-9 + 2^-23 (fp32 engines with wide_arithmetic, against the reference's outputs rounded to fp32), on mean, covariance, d^2
and log-likelihood.  Every comparison prints a PARITY line with its maxima before it asserts.

Every parity comparison also makes the SCALED one (tests/feature_scaled_parity.py): the updated state (mu, C), whitened by the
reference's own sigmas and held block by block -- fp64 1e-9; wide_arithmetic 2 u v + 1e-9 against the float64 reference on the
inputs as stored (the kernel narrows each stored output once); plain fp32 max(M_feat d_32, 20 u v), d_32 the distance of the
all-float32 evaluation of the same call (tests/feature_f32.py) from its float64 evaluation on the same batch.  It prints one
SCALED line: the largest fraction of a bound and the block it belongs to.  d^2 and the log-likelihood are
dimensionless and stay on the bound above.
"""
import numpy as np
import pytest
import torch

import feature_f32 as ff
import feature_scaled_parity as fsp
import state_meas_reference as smr
from engine_support import Case, cycled_engine, engine_of, man_of, pack, same_snapshot, scaled, snapshot, tdt
from oracle import ukf_numpy as on

pytestmark = pytest.mark.gpu

N = 1022   # not a multiple of four: the last workgroup holds two filters
PRECS = [("f64", 0, 0, 1e-9), ("f32", 1, 0, 1e-4), ("f32w", 1, 1, 1e-9 + 2.0 ** -23)]
ST_NONFINITE, ST_CHOLESKY, ST_UNINIT, ST_INACTIVE, ST_REJECTED = 1 << 4, 1 << 5, 1 << 7, 1 << 8, 1 << 9


_CACHE = {}


def case(spe, model, pname, n=N):
    key = (model, pname, n)
    if key not in _CACHE:
        _, prec, wide, tol = [p for p in PRECS if p[0] == pname][0]
        e = cycled_engine(spe, model, n, prec, wide)
        c = Case()
        c.model, c.pname, c.n, c.prec, c.wide, c.tol = model, pname, n, prec, wide, tol
        c.mu, c.cov, _ = e.state()
        c.dtype = e.dtype
        c.z, c.Qz = smr.make_inputs(man_of(model), c.mu, c.cov, e.dtype)
        e.close()
        c.refs = {}
        _CACHE[key] = c
    return _CACHE[key]


def run(e, masks, z, Qz, a=1.0, b=1.0, commit=True):
    """-> (mu, cov, maha, loglik, status) after update_state_dev"""
    n, dt = e.capacity, tdt(e)
    zd = torch.from_numpy(z).to("cuda", dt)
    qd = torch.from_numpy(pack(Qz)).to("cuda", dt)
    md = None if np.isscalar(masks) else torch.from_numpy(np.asarray(masks, dtype=np.int32)).to("cuda")
    maha = torch.full((n,), -7.0, dtype=dt, device="cuda")
    ll = torch.full((n,), -7.0, dtype=dt, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.update_state_dev(int(masks) if md is None else 0, zd, qd, block_mask_dev=md, state_inflation=a, meas_inflation=b,
                       commit=commit, maha=maha, loglik=ll, status=st)
    e.sync()
    torch.cuda.synchronize()
    mu, cov, _ = e.state()
    return mu, cov, maha.double().cpu().numpy(), ll.double().cpu().numpy(), st.cpu().numpy().astype(np.uint32)


def reference(c, masks, z=None, Qz=None, a=1.0, b=1.0, gate=-1.0, initialised=None):
    key = None
    if z is None and Qz is None and initialised is None and np.isscalar(masks):
        key = (int(masks), a, b, gate)
        if key in c.refs:
            return c.refs[key]
    ref = smr.update_state(man_of(c.model), c.mu, c.cov, masks, c.z if z is None else z, c.Qz if Qz is None else Qz, a, b, gate,
                           initialised)
    if key is not None:
        c.refs[key] = ref
    return ref


def check_parity(name, c, got, ref, tol=None, rows=None, masks=None, z=None, Qz=None, a=1.0, b=1.0):
    """the file's bound on mean, covariance, d^2 and log-likelihood, then the scaled check of the updated state
    (tests/feature_scaled_parity.py); masks, z, Qz, a, b: the call, for the fp32 evaluation behind a plain fp32 engine's bound"""
    tol = c.tol if tol is None else tol
    rows = np.ones(c.n, bool) if rows is None else rows
    r = [np.asarray(x, dtype=np.float64) for x in ref[:4]]
    if c.wide:   # the engine stores fp32
        r = [x.astype(np.float32).astype(np.float64) for x in r]
    scored = rows & ~np.isnan(r[2])
    assert np.array_equal(np.isnan(got[2][rows]), np.isnan(r[2][rows])), name
    em, ec = scaled(got[0][rows], r[0][rows]), scaled(got[1][rows], r[1][rows])
    ed, el = scaled(got[2][scored], r[2][scored]), scaled(got[3][scored], r[3][scored])
    print(f"PARITY {name} n={int(rows.sum())} max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} max_scaled_dmaha={ed:.3e} "
          f"max_scaled_dloglik={el:.3e} tol={tol:.3e}")
    assert em <= tol and ec <= tol and ed <= tol and el <= tol, (name, em, ec, ed, el, tol)
    z, Qz = (c.z if z is None else z), (c.Qz if Qz is None else Qz)
    mk = np.broadcast_to(np.asarray(masks, dtype=np.int64), (c.n,))
    keep = np.asarray(ref[4]) != 0   # not committed: gated, inactive

    def f32():
        return tuple(ff.state_meas(c.model, c.mu[rows], c.cov[rows], mk[rows], z[rows], Qz[rows], a, b, keep[rows], prec=p)
                     for p in ("f32", "f64"))
    fsp.judge_state("state_meas/" + name, c.model, c.pname, got[0][rows], got[1][rows], ref[0][rows], ref[1][rows], f32=f32)


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_parity(spe, model, pname):
    c = case(spe, model, pname)
    nb = len(man_of(model).fields)
    masks = [smr.full_mask(model)] + ([3] if model == "pose" else []) + [1 << b for b in range(nb)]
    for m in masks:
        e = engine_of(spe, c)
        got, ref = run(e, m, c.z, c.Qz), reference(c, m)
        e.close()
        assert (ref[4] == 0).all(), (m, np.unique(ref[4]))
        assert (got[4] == 0).all(), (m, np.unique(got[4]))
        check_parity(f"{model}/{pname}/mask={m}", c, got, ref, masks=m)
    per = smr.cycling_masks(model, c.n)
    e = engine_of(spe, c)
    got, ref = run(e, per, c.z, c.Qz), reference(c, per)
    assert np.array_equal(e.status(), got[4])   # commit = 1 writes the engine's own status array too
    e.close()
    expect = np.where(per == 0, ST_INACTIVE, 0).astype(np.uint32)
    assert np.array_equal(ref[4], expect) and np.array_equal(got[4], expect)
    check_parity(f"{model}/{pname}/per-filter-masks", c, got, ref, masks=per)
    idle = per == 0
    assert np.array_equal(got[0][idle], c.mu[idle]) and np.array_equal(got[1][idle], c.cov[idle])


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", ["f64", "f32"])
def test_covariance_intersection(spe, model, pname):
    w = 0.3
    c = case(spe, model, pname)
    e = engine_of(spe, c)
    got = run(e, smr.full_mask(model), c.z, c.Qz, a=1.0 / w, b=1.0 / (1.0 - w))
    e.close()
    ref = reference(c, smr.full_mask(model), a=1.0 / w, b=1.0 / (1.0 - w))
    assert (ref[4] == 0).all() and (got[4] == 0).all()
    check_parity(f"{model}/{pname}/covariance-intersection", c, got, ref, masks=smr.full_mask(model), a=1.0 / w, b=1.0 / (1.0 - w))
    assert np.linalg.eigvalsh(got[1]).min() > 0.0
    assert not np.array_equal(got[1], reference(c, smr.full_mask(model))[1])


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", ["f64", "f32"])
def test_gate(spe, model, pname):
    c = case(spe, model, pname)
    m = smr.full_mask(model)
    free = reference(c, m)
    gate = float(np.median(free[2]))
    ref = reference(c, m, gate=gate)
    e = engine_of(spe, c, gate_chi2=gate)
    got = run(e, m, c.z, c.Qz)
    e.close()
    near = np.abs(free[2] - gate) <= c.tol * (1.0 + free[2])
    assert near.sum() <= c.n // 100, int(near.sum())
    rows = ~near
    assert np.array_equal(got[4][rows], ref[4][rows])
    rej = rows & (ref[4] == ST_REJECTED)
    assert rej.sum() > c.n // 4 and (rows & (ref[4] == 0)).sum() > c.n // 4
    assert np.array_equal(got[0][rej], c.mu[rej]) and np.array_equal(got[1][rej], c.cov[rej])
    assert np.isfinite(got[2][rej]).all()
    check_parity(f"{model}/{pname}/gate", c, got, ref, rows=rows, masks=m)


# ------------------------------------------------------------------------------------------------------- bit-level properties
@pytest.mark.parametrize("model", ["pose", "orient"])
def test_bit_level_properties(spe, model):
    n = 255
    c = case(spe, model, "f64", n)
    m = 0b0110
    per = smr.cycling_masks(model, n)

    def fresh(**kw):
        e = engine_of(spe, c, **kw)
        e.set_last_measurement_time(np.arange(1, n + 1, dtype=np.int64) * 1000 + 7)
        return e

    e = fresh()
    base = run(e, m, c.z, c.Qz)
    e.close()
    # a device array filled with m = the uniform mask m
    e = fresh()
    assert same_snapshot(run(e, np.full(n, m, dtype=np.int32), c.z, c.Qz), base)
    e.close()
    # the host form = the device form (per-filter masks too)
    e = fresh()
    d2, ll, st = e.update_state(m, c.z, c.Qz)
    mu, cov, _ = e.state()
    assert same_snapshot((mu, cov, d2, ll, st), base)
    e.close()
    e, e2 = fresh(), fresh()
    d2, ll, st = e.update_state(per, c.z, c.Qz)
    mu, cov, _ = e.state()
    assert same_snapshot((mu, cov, d2, ll, st), run(e2, per, c.z, c.Qz))
    e.close(); e2.close()
    # inflation 1, 1 under a gate nothing reaches = no gate
    e = fresh(gate_chi2=1e300)
    assert same_snapshot(run(e, m, c.z, c.Qz), base)
    e.close()
    # commit = 0: the whole downloadable engine keeps its bits, the outputs are the committing call's, and the next
    # prediction is an untouched twin's
    e, twin = fresh(), fresh()
    before = snapshot(e)
    dry = run(e, m, c.z, c.Qz, commit=False)
    dry_per = run(e, per, c.z, c.Qz, commit=False)
    assert same_snapshot(before, snapshot(e)) and same_snapshot(before, snapshot(twin))
    assert same_snapshot(dry[2:], base[2:]) and np.array_equal(dry[0], c.mu) and np.array_equal(dry[1], c.cov)
    assert np.array_equal(dry_per[4], np.where(per == 0, ST_INACTIVE, 0))
    e.predict(0.013); twin.predict(0.013)
    assert same_snapshot(snapshot(e), snapshot(twin))
    e.close(); twin.close()
    # commit = 0, then commit = 1: the same d^2 as commit = 1 alone
    e = fresh()
    run(e, m, c.z, c.Qz, commit=False)
    assert same_snapshot(run(e, m, c.z, c.Qz), base)
    e.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
@pytest.mark.parametrize("pname", ["f32", "f32w"])
def test_host_array_form_fp32(spe, model, pname):
    """fp32 engines: ukfb_update_state narrows the host doubles and packs Qz itself; its outputs and the committed state are the
    bits of the device form fed the same values rounded to float32.  Five filters: one full wavefront and a one-row tail."""
    n = 5
    c = case(spe, model, pname, n)
    z, Qz = smr.make_inputs(man_of(model), c.mu, c.cov, np.float64)   # doubles that are NOT fp32 values
    z32, Qz32 = z.astype(np.float32).astype(np.float64), Qz.astype(np.float32).astype(np.float64)
    assert not np.array_equal(z, z32) and not np.array_equal(Qz, Qz32)
    full = smr.full_mask(model)
    per = np.array([full, 0, 1, 0b0110, 0b0101], dtype=np.int32)
    for masks in (0b0110, per):
        e, twin = engine_of(spe, c), engine_of(spe, c)
        d2, ll, st = e.update_state(masks, z, Qz)
        mu, cov, _ = e.state()
        dev = run(twin, masks, z32, Qz32)
        assert np.array_equal(st, dev[4]) and np.array_equal(e.status(), twin.status())
        assert np.array_equal(d2, dev[2], equal_nan=True) and np.array_equal(ll, dev[3], equal_nan=True)
        assert np.array_equal(mu, dev[0]) and np.array_equal(cov, dev[1])
        idle = np.broadcast_to(np.asarray(masks) == 0, (n,))
        assert np.array_equal(st, np.where(idle, ST_INACTIVE, 0)), st
        assert np.isfinite(d2[~idle]).all() and not np.array_equal(mu[~idle], c.mu[~idle])
        e.close(); twin.close()


@pytest.mark.parametrize("model", ["pose", "orient"])
def test_failures_stay_inside_their_filter(spe, model):
    n, dead, nan_sel, nan_unsel, neg, idle = 64, 22, 13, 14, 15, 16   # 13 ... 16 share a wavefront
    man = man_of(model)
    m = 0b0101
    _, si, ti = smr.sub_manifold(man, m)
    unsel_s = [s for s in range(man.S) if s not in si]
    e = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    mu, cov, init = e.state()
    assert not init[dead] and init.sum() == n - 1
    live = init.copy()
    mu_f, cov_f = mu.copy(), cov.copy()   # (the dead filter's inputs are made from a neighbour's state: they are never used)
    mu_f[dead], cov_f[dead] = mu[0], cov[0]
    z, Qz = smr.make_inputs(man_of(model), mu_f, cov_f, np.float64, seed=5)
    masks = np.full(n, m, dtype=np.int32)
    clean = run(e, masks, z, Qz, commit=False)
    zb, Qb, mb = z.copy(), Qz.copy(), masks.copy()
    zb[nan_sel, si[1]] = np.nan
    zb[nan_unsel, unsel_s] = np.nan
    Qb[nan_unsel, 3, :] = Qb[nan_unsel, :, 3] = np.nan   # tangent dimension 3 is outside blocks 0 and 2 in both models
    Qb[neg] = -np.eye(man.D)
    mb[idle] = 0
    got = run(e, mb, zb, Qb)
    expect = np.zeros(n, dtype=np.uint32)
    expect[dead], expect[nan_sel], expect[neg], expect[idle] = ST_UNINIT, ST_NONFINITE, ST_CHOLESKY, ST_INACTIVE
    assert np.array_equal(got[4], expect) and np.array_equal(e.status(), expect)
    failing = expect != 0
    assert np.array_equal(got[0][failing], mu[failing], equal_nan=True) and np.array_equal(got[1][failing], cov[failing], equal_nan=True)
    assert np.isnan(got[2][failing]).all() and np.isnan(got[3][failing]).all()
    # everyone else: the bits of the clean run (which committed nothing, so run it again with commit on a twin)
    twin = cycled_engine(spe, model, n, 0, 0, skip_init=(dead,))
    ok = run(twin, masks, z, Qz)
    twin.close(); e.close()
    assert same_snapshot(ok[2:], clean[2:])
    assert np.array_equal(got[0][~failing], ok[0][~failing]) and np.array_equal(got[1][~failing], ok[1][~failing])
    assert np.array_equal(got[2][~failing], ok[2][~failing]) and np.array_equal(got[3][~failing], ok[3][~failing])
    assert not np.array_equal(got[1][nan_unsel], cov[nan_unsel])
    ref = smr.update_state(man, mu_f, cov_f, mb, zb, Qb, initialised=live)
    assert np.array_equal(ref[4], expect)


# ------------------------------------------------------------------------------------- consistency with the existing kernels
@pytest.mark.parametrize("pname", [p[0] for p in PRECS])
def test_single_blocks_agree_with_update_dev(spe, pname):
    """Pose {position}, {velocity}, {angular velocity}, {orientation} against ukfb_update_dev with POS3 / VEL3 / ANGVEL3 /
    ORIENT_SO3 on a twin engine, within 2 tol.  OrientationState {velocity} is compared with nothing: ORIENT_BODYVEL3 measures
    the velocity in the BODY frame, h = q^-1 v, a different h from the selection of the velocity block."""
    c = case(spe, "pose", pname)
    rng = np.random.default_rng(23)
    for block, model_id in ((0, spe.MEAS_POS3), (2, spe.MEAS_VEL3), (3, spe.MEAS_ANGVEL3), (1, spe.MEAS_ORIENT_SO3)):
        kind, s0, t0, _ = on.POSE.fields[block]
        sig = np.sqrt(np.einsum("bii->bi", c.cov[:, t0:t0 + 3, t0:t0 + 3]))
        A = rng.standard_normal((c.n, 3, 3))
        Q3 = (sig.mean() ** 2) * (0.3 * A @ np.swapaxes(A, 1, 2) + np.eye(3))
        Q3 = Q3.astype(c.dtype).astype(np.float64)
        v = (sig * rng.standard_normal((c.n, 3))).astype(c.dtype).astype(np.float64)
        z, Qz = c.mu.copy(), np.zeros_like(c.cov)
        if kind == "so3":
            z3 = v                                          # the existing model takes an axis-angle sample
            z[:, s0:s0 + 4] = on.so3_exp(v)
        else:
            z3 = (c.mu[:, s0:s0 + 3] + v).astype(c.dtype).astype(np.float64)
            z[:, s0:s0 + 3] = z3
        Qz[:, t0:t0 + 3, t0:t0 + 3] = Q3
        e, twin = engine_of(spe, c), engine_of(spe, c)
        got = run(e, 1 << block, z, Qz)
        twin.update(model_id, z3, Q3)
        mu_t, cov_t, _ = twin.state()
        assert (got[4] == 0).all() and twin.status_summary() == 0
        e.close(); twin.close()
        em, ec = scaled(got[0], mu_t), scaled(got[1], cov_t)
        print(f"PARITY pose/{pname}/block={block}-vs-update_dev n={c.n} max_scaled_dmu={em:.3e} max_scaled_dcov={ec:.3e} tol={2 * c.tol:.3e}")
        assert em <= 2 * c.tol and ec <= 2 * c.tol, (block, em, ec)
        # and the joint kernel's result against the reference of ITS call, block by block
        ref = smr.update_state(on.POSE, c.mu, c.cov, 1 << block, z, Qz)
        assert (ref[4] == 0).all()

        def f32():
            return tuple(ff.state_meas("pose", c.mu, c.cov, 1 << block, z, Qz, prec=p) for p in ("f32", "f64"))
        fsp.judge_state(f"state_meas/pose/{pname}/block={block}-single", "pose", pname, got[0], got[1], ref[0], ref[1], f32=f32)


# ---------------------------------------------------------------------------------------------------- RigidBodyState records
def test_body_state_records(spe):
    n = 64
    c = case(spe, "pose", "f64", n)
    src = engine_of(spe, c)
    rec = src.export_body_states()
    src.close()
    rec[:, 0:3] += 0.01
    for b in range(4):
        rec[:, 13 + 9 * b:22 + 9 * b] *= 1.5
    active = (np.arange(n) % 3 != 0).astype(np.uint8)
    z, Qz = on.body_state_import(rec)   # the fields as they are, the four blocks on the diagonal
    for mask in (3, 15):
        e, twin = engine_of(spe, c), engine_of(spe, c)
        e.update_body_states(mask, rec, active)
        _, _, st = twin.update_state(np.where(active != 0, mask, 0).astype(np.int32), z, Qz)
        assert same_snapshot(snapshot(e), snapshot(twin)) and np.array_equal(e.status(), st)
        assert np.array_equal(st, np.where(active != 0, 0, ST_INACTIVE))
        assert not np.array_equal(e.state()[0], c.mu)
        e.close(); twin.close()
    o = case(spe, "orient", "f64", 255)
    e = engine_of(spe, o)
    with pytest.raises(spe.UkfbError, match="code 5"):
        e.update_body_states(3, np.zeros((255, 49)))
    e.close()
