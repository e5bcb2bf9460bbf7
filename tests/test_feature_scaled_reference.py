"""tests/feature_f32.py and tests/feature_scaled_parity.py pinned on the CPU (no GPU anywhere in this file).

The inputs are the GPU files' own families -- states after two real cycles with z = mu (+) L xi and Qz = Sigma + (L A)(L A)^T,
mounts and points of tests/sensor_meas_cases.make_inputs, the recorded window of tests/test_gpu_smooth.record (6 and 12
steps, per-filter noise, latched inputs), the tracks of tests/bank_reference.make_tracks, the predicted state and clutter
of tests/innovation_reference -- with the C++ oracle in the engine's place (feature_scaled_parity.cycled_state /
recorded_window / predicted_state), 203 filters (scaled_parity.SPREAD_N), as an fp64 engine holds them and rounded to float32
as an fp32 engine does.

  1. with every stage float64, feature_f32 is each family's float64 reference to 1e-12 in |x - ref| / (1 + |ref|), and within
     the fp64 bound 1e-9 in the whitened metric on every one of these input sets (measured: <= 1.2e-10, POSE_POINT and
     ORIENT_NAV_VECTOR; every other call <= 3e-12);
  2. M_feat: the ratio, block by block, between the C++ float oracle's update and the all-float32 feature evaluation of the
     two degenerate calls that compute the same thing (profiles/feature_scaled_parity.txt);
  3. four subtly wrong results per family, and a 1e-4 relative defect of a float64 result, against the files' old bound
     |x - ref| <= tol (1 + |ref|) and against the scaled check;
  4. the bounds are attainable: the all-float32 evaluation is inside max(M_feat d_32, floor) of the REFERENCE, the reference
     rounded once to float32 is inside the wide bound.

On defect 3.  The scaled check names exactly the defective block in every family.  Whether the old bound lets a defect pass is
arithmetic on the block's own scale, and the test asserts that arithmetic rather than one outcome: scaling a covariance block
by f moves its largest entry, a variance v, by (f - 1) v, inside 1e-4 (1 + v) while (f - 1) v <= 1e-4.  The zeroed gyro-bias
block (1e-6) passes everywhere.  The accelerometer-bias block times 2 (v ~ 1e-4) and the Pose angular-velocity block times
1.25 (v ~ 4e-4) sit AT that line: they pass where a measurement or the smoother has shrunk the variance and fail by a few
per cent where it still carries its prior plus process noise (v = 1.03e-4, 4.0e-4).  Swapping the gyro-bias and
accelerometer-bias means moves entries by up to 1.2e-2 (the biases are drawn at 1e-3 and 1e-2): the old bound refuses that
one in every family, the scaled check refuses it at 1e0 sigma and up."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bank_reference as br  # noqa: E402
import feature_f32 as ff  # noqa: E402
import feature_scaled_parity as fsp  # noqa: E402
import innovation_reference as ir  # noqa: E402
import scaled_parity as sp  # noqa: E402
import sensor_meas_cases as smc  # noqa: E402
import sensor_meas_reference as ser  # noqa: E402
import smoother_reference as smo  # noqa: E402
import state_meas_reference as smr  # noqa: E402
from engine_support import man_of  # noqa: E402
from oracle import ukf_numpy as on  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = sp.SPREAD_N
MODELS = ("pose", "orient")


def rel(x, ref):
    return float(np.max(np.abs(x - ref) / (1.0 + np.abs(ref)))) if np.size(x) else 0.0


def old_ok(mu, C, mu_r, C_r, tol=1e-4):
    """the bound the five GPU files held mean and covariance to"""
    return rel(mu, mu_r) <= tol and rel(C, C_r) <= tol


# ------------------------------------------------------------------------------------------------ the calls of the GPU files
class Call:
    """name, model, ref: the float64 reference's outputs, ev(prec): feature_f32's.  State outputs as (mu, C) with any leading
    axes; measurement-space outputs as (zbar, S, nu, so3) or None"""

    def __init__(self, name, model, ref, ev, ref_meas=None, ev_meas=None, so3=False):
        self.name, self.model, self.ref, self.ev, self.ref_meas, self.ev_meas, self.so3 = name, model, ref, ev, ref_meas, ev_meas, so3
        self._cache = {}

    def state(self, prec):
        if ("s", prec) not in self._cache:
            self._cache[("s", prec)] = self.ev(prec)
        return self._cache[("s", prec)]

    def meas(self, prec):
        if ("m", prec) not in self._cache:
            self._cache[("m", prec)] = self.ev_meas(prec)
        return self._cache[("m", prec)]


def state_meas_calls(spe, model, prec):
    mu, cov = fsp.cycled_state(spe, model, N, prec)
    man = man_of(model)
    z, Qz = smr.make_inputs(man, mu, cov, np.float32 if prec else np.float64)
    full = smr.full_mask(model)
    masks = [full] + ([3] if model == "pose" else []) + [1 << b for b in range(len(man.fields))] + [smr.cycling_masks(model, N)]
    out = []
    for m in masks:
        for a, b in ((1.0, 1.0),) + (((1.0 / 0.3, 1.0 / 0.7),) if np.isscalar(m) and m == full else ()):
            ref = smr.update_state(man, mu, cov, m, z, Qz, a, b)
            assert (ref[4] & ~np.uint32(on.ST_INACTIVE) == 0).all()
            tag = f"mask={m}" if np.isscalar(m) else "per-filter-masks"
            out.append(Call(f"state_meas/{model}/{tag}/a={a:.2f}", model, ref[:2],
                            lambda p, m=m, a=a, b=b: ff.state_meas(model, mu, cov, m, z, Qz, a, b, prec=p)))
    return out


def sensor_meas_calls(spe, model, prec):
    mu, cov = fsp.cycled_state(spe, model, N, prec)
    man = man_of(model)
    mount, point, gyro, zs, Q = smc.make_inputs(model, mu, np.float32 if prec else np.float64)
    out = []
    for mid in ser.ids_of(man):
        ref = ser.update_sensor(man, mu, cov, mid, zs[mid], Q, mount, point, gyro)
        assert (ref["status"] == 0).all()
        m = ser.meas_dim(mid)
        pick = lambda o, m=m: (o["z_pred"][:, :m], o["S"][:, :m, :m], o["innov"][:, :m])   # noqa: E731
        ev = lambda p, mid=mid: ff.sensor_meas(model, mu, cov, mid, zs[mid], Q, mount, point, gyro, prec=p)   # noqa: E731
        c = Call(f"sensor_meas/{model}/{ser.NAMES[mid]}", model, (ref["mu"], ref["cov"]), None, pick(ref))
        c.ev = lambda p, c=c, ev=ev: (lambda o: (o["mu"], o["cov"]))(c._cache.setdefault(("o", p), ev(p)))
        c.ev_meas = lambda p, c=c, ev=ev, pick=pick: pick(c._cache.setdefault(("o", p), ev(p)))
        out.append(c)
    per = smc.cycling_ids(model, N)
    z = np.zeros((N, 3))
    for mid in ser.ids_of(man):
        z[per == mid] = zs[mid][per == mid]
    ref = ser.update_sensor(man, mu, cov, per, z, Q, mount, point, gyro)
    out.append(Call(f"sensor_meas/{model}/per-filter-ids", model, (ref["mu"], ref["cov"]),
                    lambda p: (lambda o: (o["mu"], o["cov"]))(ff.sensor_meas(model, mu, cov, per, z, Q, mount, point, gyro, prec=p))))
    return out


def smooth_calls(spe, model, prec):
    out = []
    for steps, noise, rings in ((6, False, True), (12, False, True), (6, True, True), (6, True, False)):
        p, mu, cov, dt, ia, ib = fsp.recorded_window(spe, model, N, steps, prec, per_filter_noise=noise)
        if not rings:
            ia, ib = ia[-1], ib[-1]   # the engine's latches serve every step
        ib = ib if model == "orient" else None
        ref = smo.smooth(p, mu, cov, dt, in_a=ia, in_b=ib)
        assert (ref[2] == 0).all()
        out.append(Call(f"smooth/{model}/steps={steps}/{'per-filter-noise' if noise else 'one-noise'}/{'rings' if rings else 'latches'}",
                        model, ref[:2], lambda q, a=(p, mu, cov, dt, ia, ib): ff.smooth(*a, prec=q)))
    return out


def bank_calls(spe, model, prec):
    r = sp.f32r if prec else (lambda x: x)
    man = man_of(model)
    out = []
    for M, cap in ((2, None), (3, None), (4, None), (8, None), (4, 1)):
        _, mu, cov, w = br.make_tracks(spe, on, model, N, M, seed=7)
        mu, cov = r(mu), r(cov)
        w = r(r(w) / r(w).sum(axis=1, keepdims=True))
        Pk = r(br.transition(M))
        kw = {} if cap is None else {"max_it": cap}
        ref = br.mixture(man, mu, cov, w, **kw)
        out.append(Call(f"combine/{model}/M={M}/cap={cap}", model, ref[:2], lambda p, a=(mu, cov, w), kw=kw: ff.mixture(model, *a, p, **kw)))
        ref = br.mix(man, mu, cov, w, Pk, **kw)
        out.append(Call(f"mix/{model}/M={M}/cap={cap}", model, ref[:2], lambda p, a=(mu, cov, w, Pk), kw=kw: ff.mix(model, *a, p, **kw)))
    return out


def innovation_calls(spe, model, prec):
    mu, cov, Q = fsp.predicted_state(spe, model, N, prec)
    r = sp.f32r if prec else (lambda x: x)
    out = []
    for mid in (ir.POSE_MODELS if model == "pose" else [9]):
        z = r(ir.clutter(on, spe, model, mid, mu))
        for uq in (False, True):
            Qh = np.broadcast_to(Q[0], Q.shape).copy() if uq else Q
            m, manz, mz, S, ok, conv = ir.reference(on, model, mid, mu, cov, Qh)
            assert ok.all() and conv.all()
            so3 = model == "pose" and mid == 3
            nu, _, _ = ir.reference_scores(on, so3, m, manz, mz, S, z)
            out.append(Call(f"innovation/{model}/model={mid}/uniform_q={int(uq)}", model, None, None, (mz, S, nu),
                            lambda p, mid=mid, Qh=Qh, z=z: ff.innovation_stats(model, mid, mu, cov, Qh, z, p), so3))
    return out


BUILDERS = {"state_meas": state_meas_calls, "sensor_meas": sensor_meas_calls, "smooth": smooth_calls, "bank": bank_calls,
            "innovation": innovation_calls}
_CALLS = {}


def calls(spe, family, model, prec):
    key = (family, model, prec)
    if key not in _CALLS:
        _CALLS[key] = BUILDERS[family](spe, model, prec)
    return _CALLS[key]


# ------------------------------------------------------------------------------------------------ 1: the same algorithm
@pytest.mark.parametrize("prec", [0, 1], ids=["f64-inputs", "f32-inputs"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("family", list(BUILDERS))
def test_float64_instantiation_is_the_reference(spe, oracle, family, model, prec):
    """1e-12 in |x - ref| / (1 + |ref|), and inside the fp64 engines' bound 1e-9 in the whitened metric: every input set of the
    GPU files is one float64 can resolve to that bound"""
    for c in calls(spe, family, model, prec):
        if c.ref is not None:
            m, C = c.state("f64")
            em, ec = rel(m, c.ref[0]), rel(C, c.ref[1])
            d = sp.distances(model, *fsp._flat(model, m, C), *fsp._flat(model, *c.ref))
            w = max(d.mean.max(), d.cov.max())
            print(f"{c.name}: mean {em:.2e} cov {ec:.2e} whitened {w:.2e}")
            assert em <= 1e-12 and ec <= 1e-12, (c.name, em, ec)
            assert not sp.violations(d, sp.bound_f64(model)), (c.name, sp.violations(d, sp.bound_f64(model)))
        if c.ref_meas is not None:
            zb, S, nu = c.meas("f64")
            zr = c.ref_meas[0]
            sign = np.sign(np.sum(zb * zr, axis=-1, keepdims=True)) if c.so3 else 1.0
            errs = (rel(zb * sign, zr), rel(S, c.ref_meas[1]), rel(nu, c.ref_meas[2]))
            d, _ = fsp.meas_distances(zb, S, nu, *c.ref_meas, c.so3)
            w = max(float(x.max()) for x in d.values())
            print(f"{c.name}: z-bar {errs[0]:.2e} S {errs[1]:.2e} nu {errs[2]:.2e} whitened {w:.2e}")
            assert max(errs) <= 1e-12, (c.name, errs)
            assert w <= sp.TOL_F64, (c.name, w)


# ------------------------------------------------------------------------------------------------ 2: M_feat
def degenerate_spread(spe):
    """[(call, block, d float oracle, d feature_f32, floor, ratio or None)], M_feat.  The two fp32 evaluations of
    (a) a state-block measurement of ONE Euclidean block of the Pose state = pose_update with POS3 / VEL3 / ANGVEL3 (inputs of
        test_single_blocks_agree_with_update_dev), and
    (b) a sensor-frame measurement with r = 0 and qs the identity = pose_update with POS3 / VEL3, orient_update (inputs of
        test_degenerate_mount_agrees_with_update_dev),
    each against the C++ fp64 oracle, block by block as scaled_parity.fp32_spread"""
    from oracle import capi
    rows, worst = [], 1.0
    todo = []
    mu, cov = fsp.cycled_state(spe, "pose", N, 1)
    rng = np.random.default_rng(23)
    for block, mid in ((0, spe.MEAS_POS3), (2, spe.MEAS_VEL3), (3, spe.MEAS_ANGVEL3)):
        _, s0, t0, _ = on.POSE.fields[block]
        sig = np.sqrt(np.einsum("bii->bi", cov[:, t0:t0 + 3, t0:t0 + 3]))
        A = rng.standard_normal((N, 3, 3))
        Q3 = sp.f32r((sig.mean() ** 2) * (0.3 * A @ np.swapaxes(A, 1, 2) + np.eye(3)))
        z3 = sp.f32r(mu[:, s0:s0 + 3] + sp.f32r(sig * rng.standard_normal((N, 3))))
        z, Qz = mu.copy(), np.zeros_like(cov)
        z[:, s0:s0 + 3] = z3
        Qz[:, t0:t0 + 3, t0:t0 + 3] = Q3
        todo.append((f"state block {block} = model {mid}", "pose", mu, cov, mid, z3, Q3,
                     lambda z=z, Qz=Qz, block=block, mu=mu, cov=cov: ff.state_meas("pose", mu, cov, 1 << block, z, Qz, prec="f32")))
    ident = np.array(smc.spe_identity())
    for model, sid, mid in (("pose", ser.POSE_POSITION, spe.MEAS_POS3), ("pose", ser.POSE_VELOCITY, spe.MEAS_VEL3),
                            ("orient", ser.ORIENT_VELOCITY, spe.MEAS_ORIENT_BODYVEL3)):
        mu, cov = fsp.cycled_state(spe, model, N, 1)
        _, _, gyro, _, Q = smc.make_inputs(model, mu, np.float32)
        rng = np.random.default_rng(23)
        z = sp.f32r(ser.h(sid, mu, ident, np.zeros(3), gyro) + 0.05 * rng.standard_normal((N, 3)))
        todo.append((f"{ser.NAMES[sid]} r=0 qs=1 = model {mid}", model, mu, cov, mid, z, Q,
                     lambda model=model, sid=sid, z=z, Q=Q, gyro=gyro, mu=mu, cov=cov: (lambda o: (o["mu"], o["cov"]))(
                         ff.sensor_meas(model, mu, cov, sid, z, Q, ident, np.zeros(3), gyro, prec="f32"))))
    for name, model, mu, cov, mid, z, Q, feature in todo:
        upd = (lambda prec: capi.pose_update(mu, cov, mid, z, Q, prec=prec)) if model == "pose" else \
              (lambda prec: capi.orient_update(mu, cov, z, Q, prec=prec))
        r64, r32 = upd(0), upd(1)
        assert (r64[2] == 0).all() and (r32[2] == 0).all()
        f = feature()
        da, db = sp.distances(model, r32[0], r32[1], r64[0], r64[1]), sp.distances(model, f[0], f[1], r64[0], r64[1])
        fl = sp.floor_f32(model, r64[0], r64[1])
        B = len(fl.mean)
        fa = list(fl.mean) + [fl.cov[p, q] for p in range(B) for q in range(p, B)]
        for (label, va, _), (_, vb, _), flo in zip(da.items(), db.items(), fa):
            ratio = None
            if max(va, vb) > flo:
                ratio = max(va, vb) / max(min(va, vb), flo)
                worst = max(worst, ratio)
            rows.append((name, label, va, vb, flo, ratio))
    return rows, max(sp.M, 2.0 * worst)


def spread_text(rows, m):
    out = ["# CPU: two fp32 evaluations of the degenerate feature calls against the fp64 oracle, whitened block distances",
           f"# (tests/feature_scaled_parity.py); n = {N}, fp32-rounded inputs; ratio = larger / max(smaller, floor); '-' = both under the floor",
           f"# {'call':44s} {'block':38s} {'float oracle':>12s} {'feature_f32':>12s} {'floor':>10s} {'ratio':>7s}"]
    for name, label, va, vb, f, r in rows:
        out.append(f"  {name:44s} {label:38s} {va:12.3e} {vb:12.3e} {f:10.3e} {('%7.2f' % r) if r else '      -'}")
    top = max((r[5] for r in rows if r[5]), default=1.0)
    out.append(f"largest ratio = {top:.3f}")
    out.append(f"M_feat = {m:.3f}   (max(scaled_parity.M, 2 x the largest ratio); feature_scaled_parity.M_FEAT must not be smaller)")
    return "\n".join(out)


def test_margin_constant_covers_the_measured_spread(spe, oracle):
    rows, m = degenerate_spread(spe)
    print("\n" + spread_text(rows, m))
    assert fsp.M_FEAT >= m, (fsp.M_FEAT, m)
    assert fsp.M_FEAT <= 1.25 * m, "M_FEAT is far above what the CPU measures: re-derive it (tools/scaled_parity_report.py --features --cpu)"
    recorded = [ln for ln in open(os.path.join(ROOT, "profiles", "feature_scaled_parity.txt")) if ln.startswith("M_feat = ")]
    # (a ratio of fp32 roundings: another NumPy or BLAS summation order may move it a little)
    assert len(recorded) == 1 and abs(float(recorded[0].split()[2]) - m) <= 0.1 * m and fsp.M_FEAT >= float(recorded[0].split()[2])


# ------------------------------------------------------------------------------------------------ 3: what the old bound misses
DEFECT_CALLS = {"state_meas": 0, "sensor_meas": 0, "smooth": 0, "bank": 4}   # full mask; the first id; 6 steps; combine M = 4
ORIENT_DEFECTS = ("zero gyro-bias covariance", "acc-bias covariance x 2", "swap bias means")


def defective(model, kind, mu, C):
    """-> (mu, C, the blocks the scaled check must name, the old bound's verdict predicted from the block's own scale)"""
    mu, C = mu.copy(), C.copy()
    if kind == "zero gyro-bias covariance":
        C[..., 6:9, 6:9] = 0.0
        return mu, C, ["cov[gyro_bias,gyro_bias]"], True
    if kind == "acc-bias covariance x 2":
        v = np.einsum("...ii->...i", C[..., 9:12, 9:12]).max()
        C[..., 9:12, 9:12] *= 2.0
        return mu, C, ["cov[acc_bias,acc_bias]"], bool(v <= 1e-4 * (1.0 + v))
    if kind == "swap bias means":
        g, a = mu[..., 7:10].copy(), mu[..., 10:13].copy()
        mu[..., 7:10], mu[..., 10:13] = a, g
        return mu, C, ["mean[gyro_bias]", "mean[acc_bias]"], bool(np.abs(a - g).max() <= 1e-4)
    v = np.einsum("...ii->...i", C[..., 9:12, 9:12]).max()
    C[..., 9:12, 9:12] *= 1.25
    return mu, C, ["cov[angular_velocity,angular_velocity]"], bool(0.25 * v <= 1e-4 * (1.0 + v))


@pytest.mark.parametrize("family", ["state_meas", "sensor_meas", "smooth", "combine", "mix"])
@pytest.mark.parametrize("model", MODELS)
def test_defects_the_scaled_check_names(spe, oracle, family, model):
    fam = "bank" if family in ("combine", "mix") else family
    c = calls(spe, fam, model, 1)[DEFECT_CALLS[fam] + (family == "mix")]
    assert c.name.split("/")[0] == family, c.name
    (m32, C32), (m64, C64) = c.state("f32"), c.state("f64")
    flat = lambda a, b: fsp._flat(model, a, b)   # noqa: E731
    d_32 = sp.distances(model, *flat(m32, C32), *flat(m64, C64))
    bound = fsp.state_bound(model, "f32", *flat(*c.ref), d_32)
    assert old_ok(m32, C32, *c.ref) and not sp.violations(sp.distances(model, *flat(m32, C32), *flat(*c.ref)), bound), c.name
    passed = {}
    for kind in (ORIENT_DEFECTS if model == "orient" else ("angular-velocity covariance x 1.25",)):
        m, C, blocks, old_predicted = defective(model, kind, m32, C32)
        bad = [v[0] for v in sp.violations(sp.distances(model, *flat(m, C), *flat(*c.ref)), bound)]
        passed[kind] = old_ok(m, C, *c.ref)
        print(f"{c.name}: {kind}: old bound {'passes' if passed[kind] else 'refuses'}, scaled check names {bad}")
        assert bad == blocks, (c.name, kind, bad)
        # (predicted from the scale of the evaluated block; the reference's differs from it by ~1e-5 of itself)
        assert passed[kind] == old_predicted, (c.name, kind)
    if model == "orient":
        assert passed["zero gyro-bias covariance"] and not passed["swap bias means"]


def test_marginal_defects_pass_the_old_bound_where_the_variance_has_shrunk(spe, oracle):
    """the two defects at the old bound's own line (see the module docstring) do pass it in the families whose call shrinks
    the block: the state-block measurement of the whole state"""
    for model, kind in (("orient", "acc-bias covariance x 2"), ("pose", "angular-velocity covariance x 1.25")):
        c = calls(spe, "state_meas", model, 1)[0]
        m, C, _, predicted = defective(model, kind, *c.state("f32"))
        assert predicted and old_ok(m, C, *c.ref), (model, kind)


@pytest.mark.parametrize("family", ["state_meas", "sensor_meas", "smooth", "combine", "mix"])
def test_relative_defect_of_a_float64_result(spe, oracle, family):
    """1e-4 of itself in the gyro-bias x accelerometer-bias block (scale 1e-5): inside 1e-9 (1 + |ref|), outside 1e-9 sigma"""
    fam = "bank" if family in ("combine", "mix") else family
    c = calls(spe, fam, "orient", 0)[DEFECT_CALLS[fam] + (family == "mix")]
    m, C = (x.copy() for x in c.state("f64"))
    assert not sp.violations(sp.distances("orient", *fsp._flat("orient", m, C), *fsp._flat("orient", *c.ref)), sp.bound_f64("orient"))
    top = np.abs(C[..., 6:9, 9:12]).max()
    C[..., 6:9, 9:12] *= 1.0 + 1e-4
    C[..., 9:12, 6:9] *= 1.0 + 1e-4
    # the old bound lets it pass while the block's largest entry is below 1e-5: everywhere but in the bank, whose hypotheses
    # differ in their biases by ~1e-3 x 1e-2 and carry that spread of means into this very block
    assert old_ok(m, C, *c.ref, tol=1e-9) == bool(1e-4 * top <= 1e-9 * (1.0 + top)), (c.name, top)
    assert old_ok(m, C, *c.ref, tol=1e-9) or fam == "bank", (c.name, top)
    bad = [v[0] for v in sp.violations(sp.distances("orient", *fsp._flat("orient", m, C), *fsp._flat("orient", *c.ref)),
                                       sp.bound_f64("orient"))]
    assert bad == ["cov[gyro_bias,acc_bias]"], (c.name, bad)


# ------------------------------------------------------------------------------------------------ 4: the bounds are attainable
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("family", list(BUILDERS))
def test_bounds_are_attainable(spe, oracle, family, model, capsys):
    """the whole judge with CPU results in the engine's place: the all-float32 evaluation as the fp32 engine, the reference
    rounded once to float32 as the wide engine, the float64 evaluation as the fp64 engine; every comparison prints its line"""
    for c in calls(spe, family, model, 1):
        if c.ref is not None:
            f32 = lambda c=c: (c.state("f32"), c.state("f64"))   # noqa: E731
            fsp.judge_state(c.name, model, "f32", *c.state("f32"), *c.ref, f32=f32)
            fsp.judge_state(c.name, model, "wide", sp.f32r(c.ref[0]), sp.f32r(c.ref[1]), *c.ref)
            fsp.judge_state(c.name, model, "f64", *c.state("f64"), *c.ref)
        if c.ref_meas is not None:
            f32 = lambda c=c: (c.meas("f32"), c.meas("f64"))   # noqa: E731
            fsp.judge_meas(c.name, "f32", *c.meas("f32"), *c.ref_meas, c.so3, f32=f32)
            fsp.judge_meas(c.name, "wide", *(sp.f32r(x) for x in c.ref_meas), *c.ref_meas, c.so3)
            fsp.judge_meas(c.name, "f64", *c.meas("f64"), *c.ref_meas, c.so3)
    out = capsys.readouterr().out
    assert out.count("SCALED ") == sum(3 * ((c.ref is not None) + (c.ref_meas is not None)) for c in calls(spe, family, model, 1))


def test_judges_refuse_and_name(spe, oracle):
    """a gyro-bias block 1e-3 off is named with its flattened row; S 1e-3 off in one entry is named as output S"""
    c = calls(spe, "smooth", "orient", 0)[0]
    m, C = (x.copy() for x in c.state("f64"))
    C[2, 17, 6, 6] *= 1.0 + 1e-3
    with pytest.raises(AssertionError, match=rf"block cov\[gyro_bias,gyro_bias\] filter {2 * N + 17}: "):
        fsp.judge_state("x", "orient", "f64", m, C, *c.ref)
    c = calls(spe, "innovation", "pose", 0)[0]
    zb, S, nu = (x.copy() for x in c.meas("f64"))
    S[5, 0, 1] += 1e-3 * np.sqrt(c.ref_meas[1][5, 0, 0] * c.ref_meas[1][5, 1, 1])
    with pytest.raises(AssertionError, match=r"output S: 1.000e-03 > bound 1.000e-09"):
        fsp.judge_meas("x", "f64", zb, S, nu, *c.ref_meas)
    assert fsp.judge_state("x", "pose", "f32", *calls(spe, "bank", "pose", 1)[0].ref, *calls(spe, "bank", "pose", 1)[0].ref) is None
