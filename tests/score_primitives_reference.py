"""40-digit references, deterministic case tables, error units and NumPy statements for the scoring primitives of the robust and
the relative update: robust_eval, robust_scale (slam-pose_estimation_amd/csrc/ukf_robust.hpp), relative_chol6 and relative_solve6
(ukf_relative.hpp).  A helper with no GPU dependency and no tests: tests/test_score_primitives_reference.py holds the NumPy
statements to these references, tests/test_gpu_score_primitives.py the device (tests/cpp/score_probe.hip).

References (mpmath, 40 digits, from the exact binary inputs, i.e. the T-rounded records):
  eval      S(lambda) = Sigma_z + lambda Q without rounding, x = S^-1 nu, f = nu^T x, g = x^T Q x
  scale     MATCH is judged by the residual r = f(lambda_dev) / c^2 - 1 of the lambda it returned, not by a reference lambda; the
            reference's own Newton (the header's rule in exact arithmetic) gives the step count and the root.  HUBER:
            sqrt(f(1) / c^2)
  chol6     the Cholesky factor of A, ln det A = sum ln x_k (x_k the pivots), y = L^-1 v, d^2 = v^T A^-1 v

Units, in eps(T).  kappa_H is the 2-norm condition number of the diagonally scaled matrix H = diag(A)^-1/2 A diag(A)^-1/2, as
in tests/chol_reference.py, of S(lambda) or of A:
  f      kappa_H(S(lambda)) f_ref
  g      kappa_H (|x|^T |Q| |x|)
  L      the backward residual |A - L L^T|_ij over sqrt(a_ii a_jj)  (max over i, j; L as returned, products unrounded)
  lndet  kappa_H + sum |ln x_k|, absolute
  y      kappa_H |y_ref|_2
  d^2    kappa_H d^2_ref  (the test forms d^2 = |y|^2 from the returned y in extended precision)
A record's bound is its regime's first term (four times the reference-alone maximum, floor 4: base_bound) plus RECIP eps, in the
same unit, once per hardware-seeded reciprocal on the path to the result (N_RECIP): f, g and d0sq two fast_rcp and three
fast_rsqrt; an entry (i, j) of the residual the one rsqrt of column j; lndet the five rsqrt behind the last pivot; y and d^2 six.

Verdict margin.  robust_eval forms S = fl(Sigma_z + lambda Q) (one rounding u per entry, fused) and eliminates as chol16 does,
the trailing update through rcp(pivot): the bound B(T, 3, j) of tests/chol_reference.py holds with D = 3, and the rounding of S
adds u, so m3(T) = 3 (B(T, 3, 2) + u): the pivots are all positive where lambda_min(H) >= m3 and one is not where
lambda_min(H) <= -m3.  relative_chol6 differs: no rcp, dot-product form.  L_ij = fl((a_ij - sum_{k<j} L_ik L_jk) rs_j) with
rs_j = rsqrt(x_j)(1 + d), |d| <= sigma, and L_jj = fl(x_j rs_j): j fused steps and one product round the entry, and
L_ij L_jj = (a_ij - sum)(1 + d)^2 up to those roundings, so Higham's (10.4) reads |A - L L^T|_ij <= e_j (|L||L^T|)_ij with
e_j = (1 + sigma)^2 / (1 - u)^(j + 2) - 1 -- chol_reference's eps_j without its reciprocal term rho.  Cauchy-Schwarz and the
induction of Thm 10.7 go through unchanged: B6(T, j) = e_j / (1 - e_5), m6(T) = 6 B6(T, 5) = 3.1e2 eps (fp64), 45 eps (fp32).
Every record of every table has S(lambda) (at lambda = 1 and at every lambda the reference's Newton visits) or A either clearly
positive definite (lambda_min(H) >= m) or clearly indefinite (<= -m), decided at 40 digits (classify); no family generates a
matrix in between and no record is excluded from a verdict assertion.  The exactly semidefinite records are those whose failing
pivot is 0 in any arithmetic -- a zero row and column, x = 0 - sum 0^2 -- : another singular matrix has lambda_min(H) = 0 inside
the margin, where rounding decides the sign of the pivot and no verdict can be asserted.  The ill-conditioned families run in
decades of kappa_H from 1e1 to the last at which lambda_min(H) >= 2 m is certain (cond_decades' logic with these margins).

Tables of robust_scale.  contracts (inlier, m1, proportional, null, ineligible, s1_indefinite, nan, indefinite_q), benign
(Sigma_z = W W^T, Q = W diag(mu) W^T with mu within a decade, times 1 and 1e-6; nu = Ls u rho at rho = 3 ... 1e6), spread
(mu over e decades, e = 2 ... 8 in fp64, 1 ... 3 in fp32), clamp (scale_max = 30, roots far above and below it), gated (gate 400).
benign keeps kappa_H <= 1e3 in fp64 and <= 10 in fp32: a step count is determined only where tol > 2 slack, which at the
loose fp32 tolerance 1e-4 and a bound of 14 ... 20 units caps kappa_H near 30; and a draw whose reference Newton leaves a
residual within a factor of 3 of the loose tolerance is drawn again.  The cases (SCALE_CASES) put rules on the tables: the loose
tolerance (1e-9 / 1e-4), the suite's (1e-13 / 2e-6), max_iter = 64 on spread, HUBER, and `mixed`, all of contracts, benign and
spread in one launch for the neighbour-independence test.

The rule's thresholds and tolerances are rounded to T, as the kernel receives them.  A table is a Table: X the device records
[n, IN], reg the regime of every record (index into names), match the records robust_scale is expected to solve in MATCH, one
the records it must leave at lambda = 1 with no step."""
import collections
import functools
import math
import os
from types import SimpleNamespace

import numpy as np

import chol_reference as cr
from probe_support import DT, EPS, F32, F64, _m

IN, OUT = 28, 30                     # doubles per record (tests/cpp/score_probe.hip SCOREP_IN / SCOREP_OUT)
SR_LAM, SR_M, SR_ELIGIBLE = 15, 16, 17
PRIM = dict(eval=0, scale=1, chol6=2, solve=3)
RECIP = {F64: 24.0, F32: 2.0}        # fast_rsqrt / fast_rcp, relative, in eps(T): the bounds of tests/test_gpu_so3_primitives.py
N_RECIP = dict(f=5, g=5, L=1, lndet=5, y=6, d2=6)
U = cr.U
MATCH, HUBER = 0, 1
CHI2_M1, CHI2_M3 = 3.8415, 7.8147
TOL_LOOSE = {F64: 1e-9, F32: 1e-4}
TOL_SUITE = {F64: 1e-13, F32: 2e-6}  # tests/test_gpu_robust.py
Rule = collections.namedtuple("Rule", "mode chi2_m1 chi2_m3 scale_max tol max_iter gate_chi2")


def mp():
    import mpmath
    return mpmath


def rule(prec, mode=MATCH, scale_max=1e30, tol=None, max_iter=16, gate_chi2=-1.0):
    t = lambda v: float(DT[prec](v))
    return Rule(int(mode), t(CHI2_M1), t(CHI2_M3), t(scale_max), t(TOL_LOOSE[prec] if tol is None else tol), int(max_iter), t(gate_chi2))


def Table(X, reg, names, match=None, one=None):
    X = np.ascontiguousarray(X, dtype=np.float64)
    reg = np.asarray(reg, dtype=np.int64)
    z = np.zeros(len(X), dtype=bool)
    return SimpleNamespace(X=X, reg=reg, names=tuple(names), cls=reg, match=z if match is None else np.asarray(match, dtype=bool),
                           one=z if one is None else np.asarray(one, dtype=bool))


# ------------------------------------------------------------------------------------------------ margins and verdicts
def margin3(prec):
    return 3.0 * (cr.B(prec, 3, 2) + U[prec])


def eps6(prec, j):
    u, s = U[prec], RECIP[prec] * EPS[prec]
    return math.expm1(2.0 * math.log1p(s) - (j + 2) * math.log1p(-u))


def B6(prec, j):
    return eps6(prec, j) / (1.0 - eps6(prec, 5))


def margin6(prec):
    return 6.0 * B6(prec, 5)


def cond_decades(prec, m):
    """decades of kappa_H: 1e1 .. the last below 0.1 / u at which lambda_min(H) >= 1 / kappa >= 2 m"""
    return list(range(1, min(int(math.floor(math.log10(0.1 / U[prec]))), int(math.floor(math.log10(1.0 / (2.0 * m))))) + 1))


def classify(a, m):
    """a: a symmetric matrix as rows of mp values (or floats).  +1: lambda_min(H) >= m, -1: <= -m, 0: in between; by factorising
    H - m I and H + m I at 40 digits.  H scales by |a_ii|"""
    M = mp()
    D = len(a)
    with M.workdps(40):
        a = [[_m(x) for x in r] for r in a]
        d = [1 / M.sqrt(abs(a[i][i])) for i in range(D)]
        h = [[a[i][j] * d[i] * d[j] for j in range(D)] for i in range(D)]
        if cr._mp_chol(h, D, M.mpf(m)) is not None:
            return 1
        return -1 if cr._mp_chol(h, D, -M.mpf(m)) is None else 0


def kappa_H(A):
    """float64 estimate of the condition number of the diagonally scaled matrix (inf where it is not positive definite)"""
    with np.errstate(all="ignore"):
        H = cr.unit_diagonal(np.asarray(A, dtype=np.float64))
        if not np.isfinite(H).all():
            return np.inf
        w = np.linalg.eigvalsh(H)
    return float(w[-1] / w[0]) if w[0] > 0 else np.inf


# ------------------------------------------------------------------------------------------------ packing
TRI3 = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
TRI6 = [(r, c) for r in range(6) for c in range(r + 1)]


def pack(A):
    return np.array([A[r, c] for r, c in (TRI3 if A.shape[0] == 3 else TRI6)])


def unpack(p, D):
    A = np.zeros(p.shape[:-1] + (D, D))
    for k, (r, c) in enumerate(TRI3 if D == 3 else TRI6):
        A[..., r, c] = A[..., c, r] = p[..., k]
    return A


def _T(x, prec):
    return np.asarray(x, dtype=np.float64).astype(DT[prec]).astype(np.float64)


def rec3(prec, Sz, Q, nu, lam=1.0, m=3, eligible=1):
    r = np.zeros(IN)
    r[0:6], r[6:12], r[12:15], r[SR_LAM] = pack(0.5 * (Sz + Sz.T)), pack(0.5 * (Q + Q.T)), nu, lam
    r = _T(r, prec)
    r[SR_M], r[SR_ELIGIBLE] = m, eligible
    return r


def parts3(r):
    return unpack(r[0:6], 3), unpack(r[6:12], 3), r[12:15].copy()


def S_of(r, lam):
    Sz, Q, _ = parts3(r)
    return Sz + lam * Q


# ------------------------------------------------------------------------------------------------ the 40-digit evaluation
def mp_eval(r, lam):
    """(f, g, |x|^T |Q| |x|) of record r at lambda (an mp value or a float), as mp values; S is formed without rounding"""
    M = mp()
    lam = _m(lam)
    s = [_m(r[k]) + lam * _m(r[6 + k]) for k in range(6)]
    q = [_m(r[6 + k]) for k in range(6)]
    n = [_m(r[12 + k]) for k in range(3)]
    a, b, c, d, e, f_ = s[0], s[1], s[2], s[3], s[4], s[5]
    C = [[c * f_ - e * e, d * e - b * f_, b * e - c * d], [0, a * f_ - d * d, b * d - a * e], [0, 0, a * c - b * b]]
    C[1][0], C[2][0], C[2][1] = C[0][1], C[0][2], C[1][2]
    det = a * C[0][0] + b * C[0][1] + d * C[0][2]
    x = [sum(C[i][k] * n[k] for k in range(3)) / det for i in range(3)]
    Qm = [[q[0], q[1], q[3]], [q[1], q[2], q[4]], [q[3], q[4], q[5]]]
    f = sum(n[k] * x[k] for k in range(3))
    g = sum(x[i] * Qm[i][k] * x[k] for i in range(3) for k in range(3))
    ag = sum(abs(x[i]) * abs(Qm[i][k]) * abs(x[k]) for i in range(3) for k in range(3))
    return f, g, ag


def _S_rows(r, lam):
    lam = _m(lam)
    s = [_m(r[k]) + lam * _m(r[6 + k]) for k in range(6)]
    return [[s[0], s[1], s[3]], [s[1], s[2], s[4]], [s[3], s[4], s[5]]]


def classify_S(r, lam, prec):
    with mp().workdps(40):
        return classify(_S_rows(r, lam), margin3(prec))


def c2_of(r, rl):
    return rl.chi2_m1 if int(r[SR_M]) == 1 else rl.chi2_m3


def mp_newton(r, rl):
    """the header's rule in exact arithmetic on one record: [(lambda_k, r_k = f(lambda_k) / c^2 - 1)] for k = 0 .. its; the loop
    stops on r_k <= tol, lambda_k >= scale_max or its = max_iter, as robust_scale does"""
    c2 = _m(c2_of(r, rl))
    lam, its, out = _m(1.0), 0, []
    while True:
        f, g, _ = mp_eval(r, lam)
        out.append((lam, f / c2 - 1))
        if not (f - c2 > _m(rl.tol) * c2) or not (lam < _m(rl.scale_max)) or its >= rl.max_iter or not g > 0:
            return out
        lam = lam + f * (f - c2) / (c2 * g)
        its += 1


# ------------------------------------------------------------------------------------------------ generators
def _h3(rng, kappa):
    return cr._unit_diag_with_lmin(rng, 3, kappa)


def _benign3(rng, kmax=4.0):
    return _h3(rng, 10.0 ** rng.uniform(0.2, math.log10(kmax)))


def _at_radius(rng, S1, rho):
    """nu = Ls u rho, Ls the factor of S1, u a random unit vector: nu^T S1^-1 nu = rho^2"""
    u = rng.normal(size=3)
    return np.linalg.cholesky(S1) @ (u / np.linalg.norm(u)) * rho


def _pair(rng, ksz, mu):
    """Sigma_z = W W^T of condition ksz and Q = W diag(mu) W^T: generalised eigenvalues mu"""
    sv = 10.0 ** (-0.5 * math.log10(ksz) * np.array([0.0, rng.uniform(0.2, 0.8), 1.0]))
    W = cr._orth(rng, 3) * sv @ cr._orth(rng, 3).T
    return W @ W.T, (W * mu) @ W.T


def _indef3(rng, prec, near):
    """L diag(1, -s, 1) L^T at position p: clearly indefinite, close to the margin (near) or far from it"""
    p = int(rng.integers(3))
    L = np.linalg.cholesky(_h3(rng, 10.0 ** rng.uniform(1, 2)))
    d = np.ones(3)
    x = np.linalg.solve(L.T, np.eye(3)[p])
    d[p] = -(10.0 ** rng.uniform(0.7, 1.5) * margin3(prec) * float(x @ x)) if near else -(10.0 ** rng.uniform(-1, 0))
    return (L * d) @ L.T


EVAL_REGIMES = ("identity", "random", "graded", "illcond", "m1", "lam_large", "indefinite", "nan")
LAM_LARGE = (1e4, 1e8, 1e12, 1e16, 1e20)


@functools.lru_cache(maxsize=None)
def eval_table(prec, seed=3101):
    rng = np.random.default_rng([seed, prec])
    rows, reg = [], []

    def add(name, *a, **k):
        rows.append(rec3(prec, *a, **k))
        reg.append(EVAL_REGIMES.index(name))

    for q in (0.0, 0.5, 1.0, 2.0):
        for lam in (1.0, 2.5, 7.0):
            add("identity", np.eye(3), q * np.eye(3), rng.normal(size=3), lam)
    n = 0
    while n < 36:
        Sz, Q, lam = _benign3(rng), 10.0 ** rng.uniform(-1, 0.5) * _benign3(rng), (1.0, 3.0, 30.0)[n % 3]
        if kappa_H(Sz + lam * Q) <= 8.0:
            add("random", Sz, Q, 10.0 ** rng.uniform(-1, 1) * rng.normal(size=3), lam)
            n += 1
    for i in range(36):
        d = 10.0 ** rng.permutation(np.linspace(-3.0, 3.0, 3))
        Sz, Q = _benign3(rng), 10.0 ** rng.uniform(-1, 0.5) * _benign3(rng)
        add("graded", d[:, None] * Sz * d[None, :], d[:, None] * Q * d[None, :], d * rng.normal(size=3), (1.0, 3.0, 30.0)[i % 3])
    for e in cond_decades(prec, margin3(prec)):
        for i in range(8):
            H, lam = _h3(rng, 10.0 ** e), (1.0, 2.0)[i % 2]
            if i < 4:       # Sigma_z = H - lambda Q: the sum cancels to H
                Q = 0.3 * _benign3(rng)
                add("illcond", H - lam * Q, Q, rng.normal(size=3), lam)
            else:           # Sigma_z and Q proportional to H
                add("illcond", 0.5 * H, 0.5 * H / lam, rng.normal(size=3), lam)
    for s in (1e-6, 1.0, 1e6):
        for q in (1e-6, 1.0, 1e3):
            for lam in (1.0, 10.0, 1e6):
                add("m1", np.diag([s, 1.0, 1.0]), np.diag([q, 0.0, 0.0]), np.array([math.sqrt(s + lam * q) * rng.uniform(1, 5), 0.0, 0.0]), lam, m=1)
    for lam in LAM_LARGE:
        for _ in range(6):
            add("lam_large", _benign3(rng), 10.0 ** rng.uniform(-1, 0.5) * _benign3(rng), math.sqrt(lam) * rng.normal(size=3), lam)
    for i in range(24):
        near = i % 2 == 0
        add("indefinite", _indef3(rng, prec, near), np.zeros((3, 3)) if near else 1e-4 * _benign3(rng), rng.normal(size=3), 1.0)
    base = rows[reg.index(EVAL_REGIMES.index("random"))]
    for k in list(range(15)) + [SR_LAM]:
        r = base.copy()
        r[k] = np.nan
        rows.append(r)
        reg.append(EVAL_REGIMES.index("nan"))
    return Table(np.array(rows), reg, EVAL_REGIMES)


def _scale_tables(prec):
    """the records of robust_scale by table: contracts, benign, spread, clamp, gated"""
    rng = np.random.default_rng([3102, prec])
    fp64 = prec == F64
    c3, c1 = float(DT[prec](CHI2_M3)), float(DT[prec](CHI2_M1))
    out = {}

    def start(names):
        return SimpleNamespace(rows=[], reg=[], match=[], one=[], names=names)

    def add(t, name, r, match=False, one=False):
        t.rows.append(r)
        t.reg.append(t.names.index(name))
        t.match.append(match)
        t.one.append(one)

    def outlier(ksz, mu, rho, **k):
        Sz, Q = _pair(rng, ksz, np.asarray(mu))
        return rec3(prec, Sz, Q, _at_radius(rng, Sz + Q, rho), **k)

    ksz = (1.0, 10.0, 100.0) if fp64 else (1.0, 2.0)
    mu3 = lambda: 10.0 ** rng.uniform(-0.5, 0.5 if fp64 else 0.0, 3)
    # ---- contracts
    t = start(("inlier", "m1", "proportional", "null", "ineligible", "s1_indefinite", "nan", "indefinite_q"))
    for dlt in ((1e-6 if fp64 else 1e-3), 0.1, 0.5, 0.99):
        for k in ksz:
            for _ in range(3):
                add(t, "inlier", outlier(k, mu3(), math.sqrt(c3 * (1 - dlt))), one=True)
        for s in (1e-3, 1.0, 1e3):
            add(t, "inlier", rec3(prec, np.diag([s, 1.0, 1.0]), np.diag([s, 0.0, 0.0]), [math.sqrt(2 * s * c1 * (1 - dlt)), 0.0, 0.0], m=1), one=True)
    for s in (1e-3, 1.0, 1e3):
        for q in (1e-6, 1.0, 1e3):
            for rho in (3.0, 30.0, 1e3):
                add(t, "m1", rec3(prec, np.diag([s, 1.0, 1.0]), np.diag([q, 0.0, 0.0]), [math.sqrt(s + q) * rho, 0.0, 0.0], m=1), match=True)
    for tq in (1e-3, 1.0, 10.0):
        for rho in (3.0, 30.0, 1e3):
            for _ in range(3):
                A = _benign3(rng, 8.0)
                add(t, "proportional", rec3(prec, A, tq * A, _at_radius(rng, (1 + tq) * A, rho)), match=True)
    for s in (1e-3, 1.0, 1e3):
        for q in (1e-3, 1.0):
            for rho in (3.0, 1e3):
                add(t, "null", rec3(prec, np.diag([s, 2.0 * s, 0.5]), np.diag([0.0, q, q]), [math.sqrt(s) * rho, 0.0, 0.0]), one=True)
    for rho in (3.0, 30.0, 1e3):
        for k in ksz:
            add(t, "ineligible", outlier(k, mu3(), rho, eligible=0), one=True)
    for i in range(12):
        near = i % 2 == 0
        add(t, "s1_indefinite", rec3(prec, _indef3(rng, prec, near), np.zeros((3, 3)) if near else 1e-4 * _benign3(rng), 10.0 * rng.normal(size=3)), one=True)
    base = outlier(1.0, mu3(), 30.0)
    for k in range(15):
        r = base.copy()
        r[k] = np.nan
        add(t, "nan", r, one=True)
    for _ in range(12):
        Sz, Q = _pair(rng, 10.0, np.array([1.0, -0.5, 0.2]) * 10.0 ** rng.uniform(-1, 0))
        add(t, "indefinite_q", rec3(prec, Sz, Q, _at_radius(rng, Sz + Q, 10.0)))
    out["contracts"] = t
    # ---- benign
    t = start(("q1", "q1e-6"))
    for k in ksz:
        for rho in (3.0, 10.0, 1e2, 1e3, 1e4, 1e5, 1e6):
            for qs in (1.0, 1e-6):
                for _ in range(3):
                    # the step count at the loose tolerance must be determined (unambiguous): no iterate of the reference's own
                    # Newton may leave a residual within a factor of 3 of it -- far more than 2 slack at kappa_H <= 1e3 (fp64), 10 (fp32)
                    while True:
                        r = outlier(k, qs * mu3(), rho)
                        with mp().workdps(60):
                            res = [float(x[1]) for x in mp_newton(r, rule(prec))]
                        if not any(0.3 * TOL_LOOSE[prec] <= x <= 3.0 * TOL_LOOSE[prec] for x in res):
                            break
                    add(t, "q1" if qs == 1.0 else "q1e-6", r, match=True)
    out["benign"] = t
    # ---- spread
    dec = range(2, 9) if fp64 else range(1, 4)
    t = start(tuple(f"1e{e}" for e in dec))
    for e in dec:
        for rho in (5.0, 30.0, 300.0):
            for _ in range(4):
                mu = 10.0 ** (-e * np.array([0.0, rng.uniform(0.2, 0.8), 1.0]))[rng.permutation(3)]
                add(t, f"1e{e}", outlier(2.0, mu, rho), match=True)
    out["spread"] = t
    # ---- clamp (scale_max = 30): roots far above it, and roots below it in the same launch
    t = start(("clamp", "below"))
    for rho in (1e2, 1e3, 1e4):
        for k in ksz:
            for _ in range(4):
                add(t, "clamp", outlier(k, mu3(), rho), match=True)
    for rho in (3.0, 4.0, 6.0):
        for k in ksz:
            for _ in range(4):
                add(t, "below", outlier(k, mu3(), rho), match=True)
    out["clamp"] = t
    # ---- gated (gate_chi2 = 400)
    t = start(("gated", "passed"))
    for rho in (30.0, 1e2, 1e3):
        for k in ksz:
            for _ in range(4):
                add(t, "gated", outlier(k, mu3(), rho), one=True)
    for rho in (3.0, 10.0, 15.0):
        for k in ksz:
            for _ in range(4):
                add(t, "passed", outlier(k, mu3(), rho), match=True)
    out["gated"] = t
    return {k: Table(np.array(v.rows), v.reg, v.names, v.match, v.one) for k, v in out.items()}


SCALE_TABLES = ("contracts", "benign", "spread", "clamp", "gated")
SCALE_MAX_CLAMP, GATE = 30.0, 400.0


@functools.lru_cache(maxsize=None)
def scale_table(prec, name):
    if name == "mixed":          # the neighbour-independence launch: every trip count and the NaN records in one table
        parts = [scale_table(prec, k) for k in ("contracts", "benign", "spread")]
        names, reg, off = [], [], 0
        for k, p in zip(("contracts", "benign", "spread"), parts):
            names += [f"{k}.{n}" for n in p.names]
            reg.append(p.reg + off)
            off += len(p.names)
        return Table(np.concatenate([p.X for p in parts]), np.concatenate(reg), names, np.concatenate([p.match for p in parts]),
                     np.concatenate([p.one for p in parts]))
    return _scale_tables_cached(prec)[name]


@functools.lru_cache(maxsize=None)
def _scale_tables_cached(prec):
    return _scale_tables(prec)


# (case name of robust_scale) -> (table, rule keywords)
SCALE_CASES = collections.OrderedDict([
    ("contracts", ("contracts", dict())),
    ("benign_loose", ("benign", dict())),
    ("benign_tight", ("benign", dict(tol="suite"))),
    ("spread", ("spread", dict(tol="suite", max_iter=64))),
    ("clamp", ("clamp", dict(scale_max=SCALE_MAX_CLAMP))),
    ("gated", ("gated", dict(gate_chi2=GATE))),
    ("huber_benign", ("benign", dict(mode=HUBER))),
    ("huber_spread", ("spread", dict(mode=HUBER))),
    ("mixed", ("mixed", dict(tol="suite", max_iter=64))),
])


def scale_case(prec, name):
    """(table, Rule) of a case of robust_scale"""
    tname, kw = SCALE_CASES[name]
    kw = dict(kw)
    if kw.get("tol") == "suite":
        kw["tol"] = TOL_SUITE[prec]
    return scale_table(prec, tname), rule(prec, **kw)


# ---- the 6 x 6 tables
CHOL_REGIMES = ("identity", "random", "graded", "illcond", "margin", "padded", "indefinite", "semidefinite", "nan")


def rec6(prec, A, v):
    r = np.zeros(IN)
    r[0:21], r[21:27] = pack(0.5 * (A + A.T)), v
    return _T(r, prec)


@functools.lru_cache(maxsize=None)
def chol_table(prec, seed=3103):
    rng = np.random.default_rng([seed, prec])
    m = margin6(prec)
    rows, reg = [], []

    def add(name, A, v):
        rows.append(rec6(prec, A, v))
        reg.append(CHOL_REGIMES.index(name))

    for _ in range(3):
        add("identity", np.eye(6), rng.normal(size=6))
    for _ in range(36):
        G = rng.normal(size=(6, 6))
        add("random", G @ G.T + 0.5 * np.eye(6), 10.0 ** rng.uniform(-3, 0) * rng.normal(size=6))
    for _ in range(36):
        d = 10.0 ** rng.permutation(np.linspace(-3.0, 3.0, 6))
        H = cr._unit_diag_with_lmin(rng, 6, 10.0 ** rng.uniform(0.5, 2))
        add("graded", d[:, None] * H * d[None, :], d * rng.normal(size=6))
    for e in cond_decades(prec, m):
        for _ in range(8):
            add("illcond", cr._unit_diag_with_lmin(rng, 6, 10.0 ** e), rng.normal(size=6))
    for t in (2.0, 3.0, 5.0, 10.0, 30.0, 100.0):
        for _ in range(4):
            add("margin", cr._unit_diag_with_lmin(rng, 6, 10.0 ** rng.uniform(1, 2), t * m), rng.normal(size=6))
    for i in range(18):          # pairs: the model's 3 x 3 part first and last, the identity in the other part
        kind = i % 3
        A3 = _benign3(rng, 8.0) if kind == 0 else _h3(rng, 10.0 ** rng.uniform(2, 4 if prec == F64 else 3))
        if kind == 1:
            d = 10.0 ** rng.permutation(np.linspace(-3.0, 3.0, 3))
            A3 = d[:, None] * A3 * d[None, :]
        v = rng.normal(size=6)
        for first in (True, False):
            A = np.eye(6)
            sl = slice(0, 3) if first else slice(3, 6)
            A[sl, sl] = A3
            add("padded", A, v if first else np.concatenate([v[3:], v[:3]]))
    for p in range(6):
        for i in range(6):
            L = np.linalg.cholesky(cr._unit_diag_with_lmin(rng, 6, 10.0 ** rng.uniform(1, 2)))
            d = np.ones(6)
            x = np.linalg.solve(L.T, np.eye(6)[p])
            d[p] = -(10.0 ** rng.uniform(0.7, 1.5) * m * float(x @ x) if i % 2 else 10.0 ** rng.uniform(-3, 0))
            add("indefinite", (L * d) @ L.T, rng.normal(size=6))
    G = rng.normal(size=(6, 6))
    base = G @ G.T + 0.5 * np.eye(6)
    for p in range(6):
        A = base.copy()
        A[p, :] = 0.0
        A[:, p] = 0.0
        add("semidefinite", A, rng.normal(size=6))
    for k in range(21):
        r = rec6(prec, base, rng.normal(size=6))
        r[k] = np.nan
        rows.append(r)
        reg.append(CHOL_REGIMES.index("nan"))
    return Table(np.array(rows), reg, CHOL_REGIMES)


PD6 = ("identity", "random", "graded", "illcond", "margin", "padded")


def pd_mask(tb, names):
    return np.isin(tb.reg, [tb.names.index(n) for n in names if n in tb.names])


# ------------------------------------------------------------------------------------------------ references
def _hl(v):
    h = float(v)
    return h, (float(v - h) if np.isfinite(h) else 0.0)


@functools.lru_cache(maxsize=None)
def eval_reference(prec):
    """dict: f, g (hi, lo) [n], unit_f, unit_g [n], kappa [n], pd [n] (+1 / -1 / 0 of classify; NaN records 0)"""
    tb = eval_table(prec)
    n = len(tb.X)
    o = dict(f=np.full((n, 2), np.nan), g=np.full((n, 2), np.nan), unit_f=np.ones(n), unit_g=np.ones(n), kappa=np.full(n, np.inf),
             pd=np.zeros(n, dtype=np.int64))
    with mp().workdps(60):
        for i, r in enumerate(tb.X):
            if not np.isfinite(r).all():
                continue
            o["pd"][i] = classify_S(r, r[SR_LAM], prec)
            if o["pd"][i] != 1:
                continue
            f, g, ag = mp_eval(r, r[SR_LAM])
            k = kappa_H(S_of(r, r[SR_LAM]))
            o["f"][i], o["g"][i], o["kappa"][i] = _hl(f), _hl(g), k
            o["unit_f"][i], o["unit_g"][i] = k * float(f), max(k * float(ag), np.finfo(np.float64).tiny)
    return o


def _err(val, hilo, unit, prec):
    """|val - ref| / (eps unit); 0 where the reference is NaN; inf for a non-finite value elsewhere"""
    with np.errstate(all="ignore"):
        d = np.abs((val - hilo[..., 0]) - hilo[..., 1])
        e = np.where(d == 0, 0.0, d / (EPS[prec] * unit))
    e = np.where(np.isfinite(val) & ~np.isnan(e), e, np.inf)
    return np.where(np.isnan(hilo[..., 0]), 0.0, e)


def eval_errors(prec, Y):
    ref = eval_reference(prec)
    return dict(f=_err(Y[:, 0], ref["f"], ref["unit_f"], prec), g=_err(Y[:, 1], ref["g"], ref["unit_g"], prec))


def f_errors(tb, prec, lam, f):
    """the error of f, a value of robust_eval at lam [n] on the records of tb, in its unit; (errors, f_40 [n], kappa [n]);
    NaN / inf in lam, a non-finite record or an S(lam) that is not positive definite: error 0, f_40 NaN"""
    n = len(tb.X)
    e, f40, kap = np.zeros(n), np.full(n, np.nan), np.full(n, np.nan)
    with mp().workdps(60):
        for i, r in enumerate(tb.X):
            if not (np.isfinite(r).all() and np.isfinite(lam[i])):
                continue
            k = kappa_H(S_of(r, lam[i]))
            if not np.isfinite(k):
                continue
            fr = mp_eval(r, lam[i])[0]
            f40[i], kap[i] = float(fr), k
            e[i] = float(abs(_m(f[i]) - fr) / (EPS[prec] * k * fr)) if np.isfinite(f[i]) else np.inf
    return e, f40, kap


@functools.lru_cache(maxsize=None)
def scale_first(prec, tname):
    """per record of a table of robust_scale: pd = classify(S(1)) (0: non-finite record), f1 = f_40(1) (hi, lo), kappa1"""
    tb = scale_table(prec, tname)
    n = len(tb.X)
    o = dict(pd=np.zeros(n, dtype=np.int64), f1=np.full((n, 2), np.nan), kappa1=np.full(n, np.nan))
    with mp().workdps(60):
        for i, r in enumerate(tb.X):
            if np.isfinite(r).all():
                o["pd"][i] = classify_S(r, 1.0, prec)
                if o["pd"][i] == 1:
                    o["f1"][i], o["kappa1"][i] = _hl(mp_eval(r, 1.0)[0]), kappa_H(S_of(r, 1.0))
    return o


def scale_f_errors(prec, case, Y):
    """per record: the larger of the errors of d0sq (against f_40(1)) and of the returned f (against f_40 at the returned
    lambda), in the unit of f; records whose S(1) is not clearly positive definite: 0"""
    tb, _ = scale_case(prec, case)
    first = scale_first(prec, SCALE_CASES[case][0])
    pdm = first["pd"] == 1
    e0 = np.where(pdm, _err(Y[:, 2], first["f1"], first["kappa1"] * first["f1"][:, 0], prec), 0.0)
    ok = pdm & np.isfinite(tb.X).all(axis=1)
    e1, _, _ = f_errors(tb, prec, np.where(ok, Y[:, 0], np.nan), Y[:, 4])
    return np.maximum(e0, e1)


def match_residuals(prec, case, lam, fbound):
    """MATCH: per record r = f_40(lam) / c^2 - 1 and slack = fbound eps kappa_H(S(lam)) (NaN where lam is not finite)"""
    tb, rl = scale_case(prec, case)
    n = len(tb.X)
    res, slack = np.full(n, np.nan), np.full(n, np.nan)
    with mp().workdps(60):
        for i in np.nonzero(tb.match)[0]:
            if np.isfinite(lam[i]):
                c2 = _m(c2_of(tb.X[i], rl))
                res[i] = float(mp_eval(tb.X[i], lam[i])[0] / c2 - 1)
                slack[i] = fbound[i] * EPS[prec] * kappa_H(S_of(tb.X[i], lam[i]))
    return res, slack


@functools.lru_cache(maxsize=None)
def newton_reference(prec, case):
    """the reference's own Newton on the match records of a case: its [n] (-1 elsewhere), root [n] (its last lambda), reached [n]
    (stopped on the tolerance), clamped [n], resid / kappa: lists per record of every iterate's residual and kappa_H(S(lambda_k)),
    pd [n]: every S(lambda_k) is clearly positive definite"""
    tb, rl = scale_case(prec, case)
    n = len(tb.X)
    o = dict(its=np.full(n, -1), root=np.full(n, np.nan), reached=np.zeros(n, bool), clamped=np.zeros(n, bool), resid=[None] * n,
             kappa=[None] * n, pd=np.ones(n, bool))
    with mp().workdps(60):
        for i in np.nonzero(tb.match)[0]:
            it = mp_newton(tb.X[i], rl)
            o["its"][i], o["root"][i] = len(it) - 1, float(it[-1][0])
            o["reached"][i] = bool(it[-1][1] <= _m(rl.tol))
            o["clamped"][i] = bool(it[-1][0] >= _m(rl.scale_max))
            o["resid"][i] = np.array([float(x[1]) for x in it])
            o["kappa"][i] = np.array([kappa_H(S_of(tb.X[i], float(x[0]))) for x in it])
            o["pd"][i] = all(classify_S(tb.X[i], x[0], prec) == 1 for x in (it[0], it[-1]))
    return o


def unambiguous(prec, case, fbound):
    """the match records whose step count is determined: every iterate's residual is clear of tol by more than 2 slack"""
    tb, rl = scale_case(prec, case)
    ref = newton_reference(prec, case)
    out = np.zeros(len(tb.X), bool)
    for i in np.nonzero(tb.match)[0]:
        out[i] = bool(np.all(np.abs(ref["resid"][i] - rl.tol) > 2.0 * fbound[i] * EPS[prec] * ref["kappa"][i]))
    return out


def huber_reference(prec, case):
    """lambda = sqrt(f_40(1) / c^2) (hi, lo) on the match records, NaN elsewhere"""
    tb, rl = scale_case(prec, case)
    out = np.full((len(tb.X), 2), np.nan)
    with mp().workdps(60):
        for i in np.nonzero(tb.match)[0]:
            out[i] = _hl(mp().sqrt(mp_eval(tb.X[i], 1.0)[0] / _m(c2_of(tb.X[i], rl))))
    return out


@functools.lru_cache(maxsize=None)
def chol_reference(prec):
    """dict over the 6 x 6 table: pd [n] (classify; NaN and semidefinite records 0), kappa, lndet (hi, lo), unit_ln, y (hi, lo)
    [n, 6, 2], ynorm, d2 (hi, lo)"""
    M = mp()
    tb = chol_table(prec)
    n = len(tb.X)
    o = dict(pd=np.zeros(n, dtype=np.int64), kappa=np.full(n, np.inf), lndet=np.full((n, 2), np.nan), unit_ln=np.ones(n),
             y=np.full((n, 6, 2), np.nan), ynorm=np.ones(n), d2=np.full((n, 2), np.nan))
    semi = tb.names.index("semidefinite")
    with M.workdps(60):
        for i, r in enumerate(tb.X):
            if not np.isfinite(r).all() or tb.reg[i] == semi:
                continue
            A = unpack(r[0:21], 6)
            a = cr._mp_rows(A)
            o["pd"][i] = classify(a, margin6(prec))
            if o["pd"][i] != 1:
                continue
            L = cr._mp_chol(a, 6)
            y = []
            for k in range(6):
                y.append((_m(r[21 + k]) - sum(L[k][j] * y[j] for j in range(k))) / L[k][k])
            lns = [2 * M.log(L[k][k]) for k in range(6)]
            k_ = kappa_H(A)
            o["kappa"][i], o["lndet"][i], o["unit_ln"][i] = k_, _hl(sum(lns)), k_ + float(sum(abs(x) for x in lns))
            o["y"][i] = [_hl(x) for x in y]
            d2 = sum(x * x for x in y)
            o["ynorm"][i], o["d2"][i] = float(M.sqrt(d2)), _hl(d2)
    return o


def chol_errors(prec, Y):
    """errors of P_CHOL6 outputs Y [n, OUT]: dict L (backward residual), lndet; records that are not clearly PD: 0"""
    tb, ref = chol_table(prec), chol_reference(prec)
    n = len(tb.X)
    eL = np.zeros(n)
    with mp().workdps(40):
        for i in np.nonzero(ref["pd"] == 1)[0]:
            A = unpack(tb.X[i, 0:21], 6)
            if not np.isfinite(Y[i, 0:21]).all():
                eL[i] = np.inf
                continue
            R = cr.residual(A, np.tril(unpack(Y[i, 0:21], 6)), F64)
            dg = np.sqrt(np.diag(A))
            eL[i] = float(np.max(np.abs(R) / (dg[:, None] * dg[None, :]))) / EPS[prec]
    return dict(L=eL, lndet=_err(Y[:, 28], ref["lndet"], ref["unit_ln"], prec))


def solve_errors(prec, Y):
    """errors of P_CHOL6_SOLVE outputs: dict y (max over the entries), d2 (|y|^2 formed in extended precision)"""
    ref = chol_reference(prec)
    ey = _err(Y[:, 0:6], ref["y"], (ref["kappa"] * ref["ynorm"])[:, None], prec).max(axis=1)
    yl = Y[:, 0:6].astype(np.longdouble)
    d2 = np.sum(yl * yl, axis=1)
    with np.errstate(all="ignore"):
        dd = np.abs((d2 - ref["d2"][:, 0].astype(np.longdouble)) - ref["d2"][:, 1].astype(np.longdouble)).astype(np.float64)
        e2 = np.where(dd == 0, 0.0, dd / (EPS[prec] * ref["kappa"] * ref["d2"][:, 0]))
    e2 = np.where(np.isnan(ref["d2"][:, 0]), 0.0, np.where(np.isfinite(e2), e2, np.inf))
    return dict(y=ey, d2=e2)


# ------------------------------------------------------------------------------------------------ the NumPy statements in T
def _fma(a, b, c, T):
    if T is np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(T)
    with np.errstate(all="ignore"):
        r = cr._fma64(a, b, c)
    return np.where(np.isfinite(r), r, a * b + c)


def np_eval(X, lam, T):
    """robust_eval in T, as plain NumPy over records X [n, IN]: -> f, g, ok"""
    X = np.asarray(X)
    sz, q, nu = X[:, 0:6].astype(T), X[:, 6:12].astype(T), X[:, 12:15].astype(T)
    lam = np.asarray(lam).astype(T)
    one = T(1)
    with np.errstate(all="ignore"):
        s = [_fma(lam, q[:, k], sz[:, k], T) for k in range(6)]
        d0 = s[0]
        i0 = one / d0
        t10, t20 = s[1] * i0, s[3] * i0
        d1, a21 = _fma(-t10, s[1], s[2], T), _fma(-t20, s[1], s[4], T)
        i1 = one / d1
        d2 = _fma(-(a21 * i1), a21, _fma(-t20, s[3], s[5], T), T)
        ok = (d0 > 0) & (d1 > 0) & (d2 > 0)
        rs = [one / np.sqrt(d0), one / np.sqrt(d1), one / np.sqrt(d2)]
        l10, l20, l21 = s[1] * rs[0], s[3] * rs[0], a21 * rs[1]
        y0 = nu[:, 0] * rs[0]
        y1 = _fma(-l10, y0, nu[:, 1], T) * rs[1]
        y2 = _fma(-l21, y1, _fma(-l20, y0, nu[:, 2], T), T) * rs[2]
        f = _fma(y0, y0, _fma(y1, y1, y2 * y2, T), T)
        x2 = y2 * rs[2]
        x1 = _fma(-l21, x2, y1, T) * rs[1]
        x0 = _fma(-l20, x2, _fma(-l10, x1, y0, T), T) * rs[0]
        qx0 = _fma(q[:, 3], x2, _fma(q[:, 1], x1, q[:, 0] * x0, T), T)
        qx1 = _fma(q[:, 4], x2, _fma(q[:, 2], x1, q[:, 1] * x0, T), T)
        qx2 = _fma(q[:, 5], x2, _fma(q[:, 4], x1, q[:, 3] * x0, T), T)
        g = _fma(x2, qx2, _fma(x1, qx1, x0 * qx0, T), T)
    return f, g, ok


def np_eval_outputs(prec):
    tb = eval_table(prec)
    f, g, ok = np_eval(tb.X, tb.X[:, SR_LAM], DT[prec])
    Y = np.zeros((len(tb.X), OUT))
    Y[:, 0], Y[:, 1], Y[:, 2] = f, g, ok
    return Y


def np_scale(X, rl, T):
    """robust_scale in T, as plain NumPy: -> outputs [n, OUT] in the probe's layout (lam, its, d0sq, accept, f, g, ok at lam)"""
    X = np.asarray(X)
    n = len(X)
    c2 = np.where(X[:, SR_M] == 1, T(rl.chi2_m1), T(rl.chi2_m3)).astype(T)
    tol, smax, gate = T(rl.tol), T(rl.scale_max), T(rl.gate_chi2)
    with np.errstate(all="ignore"):
        f, g, ok = np_eval(X, np.ones(n), T)
        d0 = f.copy()
        accept = (gate < 0) | (f <= gate)
        inflate = (X[:, SR_ELIGIBLE] != 0) & ok & accept & (f > c2)
        lam, its = np.ones(n, dtype=T), np.zeros(n, dtype=np.int64)
        if rl.mode == HUBER:
            lam = np.where(inflate, np.sqrt(f / c2), T(1)).astype(T)
        else:
            active = inflate & (f - c2 > tol * c2)
            trip = 0
            while active.any() and trip < rl.max_iter:
                lam_new = (lam + f * (f - c2) / (c2 * g)).astype(T)
                go = active & (g > 0) & np.isfinite(g) & (lam_new > lam)
                lam = np.where(go, lam_new, lam).astype(T)
                its = its + go
                f2, g2, ok2 = np_eval(X, lam, T)
                f, g = np.where(go, f2, f), np.where(go, g2, g)
                active = go & ok2 & (f - c2 > tol * c2) & (lam < smax) & (its < rl.max_iter)
                trip += 1
        lam = np.minimum(lam, smax)
        fe, ge, oke = np_eval(X, lam, T)
    Y = np.zeros((n, OUT))
    Y[:, 0], Y[:, 1], Y[:, 2], Y[:, 3], Y[:, 4], Y[:, 5], Y[:, 6] = lam, its, d0, accept, fe, ge, oke
    return Y


def np_chol6(X, T, solve=False):
    """relative_chol6 (and relative_solve6) in T, dot-product form: -> outputs [n, OUT] in the probe's layout"""
    X = np.asarray(X)
    n = len(X)
    idx = lambda r, c: r * (r + 1) // 2 + c
    s = [X[:, k].astype(T) for k in range(21)]
    rs, ok, lndet = [None] * 6, np.ones(n, bool), np.zeros(n, dtype=T)
    with np.errstate(all="ignore"):
        for k in range(6):
            x = s[idx(k, k)]
            for j in range(k):
                x = _fma(-s[idx(k, j)], s[idx(k, j)], x, T)
            ok &= (x > 0) & np.isfinite(x)
            lndet = (lndet + np.log(x)).astype(T)
            rs[k] = T(1) / np.sqrt(x)
            s[idx(k, k)] = x * rs[k]
            for i in range(k + 1, 6):
                v = s[idx(i, k)]
                for j in range(k):
                    v = _fma(-s[idx(i, j)], s[idx(k, j)], v, T)
                s[idx(i, k)] = v * rs[k]
        Y = np.zeros((n, OUT))
        if not solve:
            Y[:, 0:21], Y[:, 21:27], Y[:, 27], Y[:, 28] = np.stack(s, axis=1), np.stack(rs, axis=1), ok, lndet
            return Y
        v = [X[:, 21 + k].astype(T) for k in range(6)]
        for k in range(6):
            x = v[k]
            for j in range(k):
                x = _fma(-s[idx(k, j)], v[j], x, T)
            v[k] = x * rs[k]
        Y[:, 0:6], Y[:, 6] = np.stack(v, axis=1), ok
    return Y


# ------------------------------------------------------------------------------------------------ the table of maxima and bounds
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "score_primitives_parity.txt")
FLOOR, FACTOR = 4.0, 4.0
PRECS = ((F64, "f64"), (F32, "f32"))
# the lines of the table: (quantity id without the precision, N_RECIP key)
LINES = ([("eval_f", "f"), ("eval_g", "g")] + [(f"scale_{t}_f", "f") for t in SCALE_TABLES]
         + [("chol6_L", "L"), ("chol6_lndet", "lndet"), ("solve_y", "y"), ("solve_d2", "d2")])
LINE_IDS = [f"{q}-{p}" for _, p in PRECS for q, _ in LINES]


def base_bound(ref_alone):
    """the first term of the bound, in units: four times the reference-alone maximum, at least 4 (written with 3 digits)"""
    return float(f"{max(FACTOR * ref_alone, FLOOR):.3g}")


def parse_table(text):
    """{line id: {regime: (reference-alone maximum, bound, device maximum or NaN)}} from lines `<line id> <regime> a/b/c ...`"""
    out = {}
    for line in text.splitlines():
        f = line.split()
        if len(f) >= 3 and f[0] in LINE_IDS:
            out[f[0]] = {r: tuple(float(x) if x != "-" else float("nan") for x in v.split("/")) for r, v in zip(f[1::2], f[2::2])}
    return out


def profile_table():
    with open(PROFILE) as fh:
        return parse_table(fh.read())


def _round_up(v):
    """v rounded up to two significant digits"""
    if v <= 0:
        return 0.0
    q = 10.0 ** (int(np.floor(np.log10(v))) - 1)
    return float(f"{np.ceil(v / q - 1e-9) * q:.2g}")


def format_table(ref_alone, device=None):
    """the lines of the table from {line id: {regime: maximum}} of the NumPy statements (CPU) and of the device (or None)"""
    lines = []
    for lid in LINE_IDS:
        cells = []
        for r, v in ref_alone[lid].items():
            listed = _round_up(1.05 * v)          # two digits, 5 % to spare for another libm or SIMD path of NumPy
            dev = "-" if device is None or lid not in device or r not in device[lid] else f"{device[lid][r]:.3g}"
            cells.append(f"{r} {listed:g}/{base_bound(listed):g}/{dev}")
        lines.append(f"{lid:22s} " + "  ".join(f"{x:30s}" for x in cells).rstrip())
    return "\n".join(lines)


def by_regime(tb, e):
    return {tb.names[c]: float(e[tb.reg == c].max()) for c in sorted(set(tb.reg.tolist()))}


def merge_max(a, b):
    return {k: max(a.get(k, 0.0), b.get(k, 0.0)) for k in list(a) + [x for x in b if x not in a]}


def record_bounds(tb, listed, lid, key, prec):
    """per record, in the quantity's unit: the regime's first term plus RECIP once per reciprocal on the path"""
    row = listed[lid]
    return np.array([row[tb.names[c]][1] for c in tb.reg]) + N_RECIP[key] * RECIP[prec]


def scale_fbound(prec, case, listed):
    """the bound of f per record of a case of robust_scale (the mixed table: from the lines of its parts)"""
    tb, _ = scale_case(prec, case)
    tname = SCALE_CASES[case][0]
    p = dict(PRECS)[prec]
    if tname != "mixed":
        return record_bounds(tb, listed, f"scale_{tname}_f-{p}", "f", prec)
    first = np.array([listed[f"scale_{n.split('.')[0]}_f-{p}"][n.split(".")[1]][1] for n in tb.names])
    return first[tb.reg] + N_RECIP["f"] * RECIP[prec]


def numpy_maxima():
    """{line id: {regime: maximum}} of the NumPy statements against the 40-digit references: the first column of the table"""
    out = {}
    for prec, p in PRECS:
        T = DT[prec]
        tb = eval_table(prec)
        e = eval_errors(prec, np_eval_outputs(prec))
        out[f"eval_f-{p}"], out[f"eval_g-{p}"] = by_regime(tb, e["f"]), by_regime(tb, e["g"])
        for t in SCALE_TABLES:
            acc = {}
            for case, (tname, _) in SCALE_CASES.items():
                if tname == t:
                    tbs, rl = scale_case(prec, case)
                    acc = merge_max(acc, by_regime(tbs, scale_f_errors(prec, case, np_scale(tbs.X, rl, T))))
            out[f"scale_{t}_f-{p}"] = acc
        tb = chol_table(prec)
        e = chol_errors(prec, np_chol6(tb.X, T))
        out[f"chol6_L-{p}"], out[f"chol6_lndet-{p}"] = by_regime(tb, e["L"]), by_regime(tb, e["lndet"])
        e = solve_errors(prec, np_chol6(tb.X, T, solve=True))
        out[f"solve_y-{p}"], out[f"solve_d2-{p}"] = by_regime(tb, e["y"]), by_regime(tb, e["d2"])
    return out


# ------------------------------------------------------------------------------------------------ the assertions, for any outputs
# (the device's in tests/test_gpu_score_primitives.py, the NumPy statements' in tests/test_score_primitives_reference.py)
def _bits(A):
    return np.ascontiguousarray(A, dtype=np.float64).view(np.int64)


def _over(tb, name, e, bound, fails):
    bad = np.nonzero(~(e <= bound))[0]
    if bad.size:
        fails.append((name, int(bad.size), [(tb.names[tb.reg[i]], int(i), float(e[i]), float(bound[i])) for i in bad[:4]]))


def eval_failures(prec, Y, listed):
    """-> (maxima {line id: {regime: max}}, failures) of P_ROBUST_EVAL outputs on eval_table(prec)"""
    p = dict(PRECS)[prec]
    tb, ref, e = eval_table(prec), eval_reference(prec), eval_errors(prec, Y)
    fails = []
    for key in ("f", "g"):
        _over(tb, key, e[key], record_bounds(tb, listed, f"eval_{key}-{p}", key, prec), fails)
    fin = np.isfinite(tb.X).all(axis=1)
    if not np.array_equal(Y[fin, 2], (ref["pd"][fin] == 1).astype(np.float64)):
        fails.append(("ok is the verdict", np.nonzero(fin & (Y[:, 2] != (ref["pd"] == 1)))[0][:6].tolist()))
    nan = np.nonzero(~fin)[0]
    if not np.isnan(Y[nan, 0]).all():
        fails.append(("NaN in, NaN f out", Y[nan, 0].tolist()))
    in_s = np.array([bool(np.isnan(np.r_[tb.X[i, 0:12], tb.X[i, SR_LAM]]).any()) for i in nan])
    if not (Y[nan[in_s], 2] == 0).all():
        fails.append(("NaN in S: ok = 0", Y[nan, 2].tolist()))
    return {f"eval_f-{p}": by_regime(tb, e["f"]), f"eval_g-{p}": by_regime(tb, e["g"])}, fails


def scale_failures(prec, case, Y, listed):
    """-> (maxima {regime: max error of f}, lines, failures) of P_ROBUST_SCALE outputs on a case"""
    tb, rl = scale_case(prec, case)
    first = scale_first(prec, SCALE_CASES[case][0])
    fb = scale_fbound(prec, case, listed)
    lam, its, d0, acc = Y[:, 0], Y[:, 1], Y[:, 2], Y[:, 3]
    fails, lines = [], []
    if not ((lam >= 1.0) & (lam <= rl.scale_max)).all():
        fails.append(("1 <= lambda <= scale_max", np.nonzero(~((lam >= 1.0) & (lam <= rl.scale_max)))[0][:6].tolist()))
    if not ((its >= 0) & (its <= rl.max_iter)).all():
        fails.append(("its <= max_iter", its[~((its >= 0) & (its <= rl.max_iter))][:6].tolist()))
    bad = np.nonzero(tb.one & ~((_bits(lam) == _bits(1.0)) & (its == 0)))[0]
    if bad.size:
        fails.append(("lambda == 1 and its == 0", [(tb.names[tb.reg[i]], int(i), float(lam[i]), float(its[i])) for i in bad[:6]]))
    ef = scale_f_errors(prec, case, Y)
    _over(tb, "f", ef, fb, fails)
    pdm = first["pd"] == 1
    want = (rl.gate_chi2 < 0) | (first["f1"][:, 0] <= rl.gate_chi2)
    if not np.array_equal(acc[pdm], want[pdm].astype(np.float64)):
        fails.append(("accept", np.nonzero(pdm & (acc != want))[0][:6].tolist()))
    m = tb.match
    if rl.mode == HUBER:
        href = huber_reference(prec, case)
        rel = _err(lam, href, href[:, 0], prec)
        bound = 0.5 * fb * first["kappa1"] + 2.0
        _over(tb, "huber lambda", np.where(m, rel, 0.0), np.where(m, bound, np.inf), fails)
        if not (its == 0).all():
            fails.append(("HUBER takes no step",))
        lines.append(("lambda rel / bound", by_regime(tb, np.where(m, rel / bound, 0.0))))
    else:
        ref = newton_reference(prec, case)
        res, slack = match_residuals(prec, case, lam, fb)
        clamped, capped = lam == rl.scale_max, its == rl.max_iter
        free = m & ~clamped & ~capped
        with np.errstate(invalid="ignore"):
            bad = np.nonzero(free & ~((res >= -slack) & (res <= rl.tol + slack)))[0]
        if bad.size:
            fails.append(("-slack <= r <= tol + slack", int(bad.size), [(tb.names[tb.reg[i]], int(i), float(res[i]), float(slack[i]), float(its[i])) for i in bad[:6]]))
        if not np.array_equal(clamped[m], ref["clamped"][m]):
            fails.append(("lambda == scale_max where the root lies above it", np.nonzero(m & (clamped != ref["clamped"]))[0][:6].tolist()))
        un = unambiguous(prec, case, fb)
        bad = np.nonzero(un & (its != ref["its"]))[0]
        if bad.size:
            fails.append(("its == its_ref", [(tb.names[tb.reg[i]], int(i), float(its[i]), int(ref["its"][i])) for i in bad[:6]]))
        with np.errstate(invalid="ignore"):
            lines.append(("max -r / slack (<= 1: how far past the root)", by_regime(tb, np.where(free, -res / slack, 0.0))))
            lines.append(("max (r - tol) / slack (<= 1)", by_regime(tb, np.where(free, (res - rl.tol) / slack, -np.inf))))
        lines.append(("capped rows", by_regime(tb, (m & capped).astype(np.float64))))
        lines.append(("max its", by_regime(tb, its)))
        lines.append(("rows with a determined step count", int(un.sum())))
    return by_regime(tb, ef), lines, fails


def _padded_part(tb):
    """per record of the 6 x 6 table: 0 not padded, 1 the identity in rows 3 .. 5, 2 in rows 0 .. 2"""
    pad = tb.reg == tb.names.index("padded")
    A = unpack(tb.X[:, 0:21], 6)
    low = pad & np.all(A[:, 3:, 3:] == np.eye(3), axis=(1, 2))
    return np.where(low, 1, np.where(pad, 2, 0))


def chol_failures(prec, Y, Ys, listed):
    """-> (maxima, failures) of P_CHOL6 outputs Y and P_CHOL6_SOLVE outputs Ys on chol_table(prec)"""
    p = dict(PRECS)[prec]
    tb, ref = chol_table(prec), chol_reference(prec)
    e, es = chol_errors(prec, Y), solve_errors(prec, Ys)
    fails = []
    for (lid, key), err in zip((("chol6_L", "L"), ("chol6_lndet", "lndet"), ("solve_y", "y"), ("solve_d2", "d2")), (e["L"], e["lndet"], es["y"], es["d2"])):
        _over(tb, key, err, record_bounds(tb, listed, f"{lid}-{p}", key, prec), fails)
    want = (ref["pd"] == 1).astype(np.float64)
    for name, ok in (("chol6", Y[:, 27]), ("solve", Ys[:, 6])):
        if not np.array_equal(ok, want):
            fails.append((name + ": ok is the verdict", [(tb.names[tb.reg[i]], int(i)) for i in np.nonzero(ok != want)[0][:6]]))
    L, rs, part = unpack(Y[:, 0:21], 6), Y[:, 21:27], _padded_part(tb)
    for i in np.nonzero(part)[0]:
        sl = slice(3, 6) if part[i] == 1 else slice(0, 3)
        exact = (np.array_equal(np.tril(L[i])[sl, :], np.eye(6)[sl, :]) and np.array_equal(np.tril(L[i])[3:, 0:3], np.zeros((3, 3)))
                 and np.array_equal(rs[i, sl], np.ones(3)) and np.array_equal(_bits(Ys[i, 0:6][sl]), _bits(tb.X[i, 21:27][sl])))
        if not exact:
            fails.append(("padded entries are exact", int(i), np.tril(L[i]).tolist(), rs[i].tolist()))
    first = np.nonzero(part == 1)[0]
    for i in first:      # the pair: the same 3 x 3 part behind the identity
        k = i + 1
        same = (part[k] == 2 and _bits(Y[i, 28]) == _bits(Y[k, 28]) and np.array_equal(_bits(rs[i, 0:3]), _bits(rs[k, 3:6]))
                and np.array_equal(_bits(np.tril(L[i])[0:3, 0:3]), _bits(np.tril(L[k])[3:6, 3:6])) and np.array_equal(_bits(Ys[i, 0:3]), _bits(Ys[k, 3:6])))
        if not same:
            fails.append(("the identity part adds exactly 0 to lndet and leaves the model's part its bits", int(i), float(Y[i, 28]), float(Y[k, 28])))
    idn = tb.reg == tb.names.index("identity")
    if not (np.all(_bits(Y[idn, 28]) == 0) and np.array_equal(np.tril(L[idn]), np.broadcast_to(np.eye(6), L[idn].shape)) and np.all(rs[idn] == 1.0)):
        fails.append(("the identity: L = I, rs = 1, lndet = +0",))
    mx = {f"chol6_L-{p}": by_regime(tb, e["L"]), f"chol6_lndet-{p}": by_regime(tb, e["lndet"]), f"solve_y-{p}": by_regime(tb, es["y"]),
          f"solve_d2-{p}": by_regime(tb, es["d2"])}
    return mx, fails
