"""The device Cholesky on its own: chol16 / load_row / load_column (slam-pose_estimation_amd/csrc/ukf_kernel16.hpp) and
chol_rows_to_lds (ukf_kernel.hpp) against a plain high-precision Cholesky of the same matrix.

tests/cpp/chol_probe.hip includes the shipped headers and calls the shipped functions in the tuned launch geometry (one
wavefront per workgroup, one matrix per 16-lane row, the LDS slice of Layout16, the factor region pre-filled with NaN) for
every (D, KS, PUB) the library instantiates, in fp64 and fp32, and chol_rows_to_lds for G = 32, 64 in fp32.
tests/chol_reference.py holds the reference (mpmath at 40 digits for fp64, float64 for fp32), the input families and the
derivation of the bounds; tests/test_chol_reference.py checks those on the CPU.

The factor is rebuilt on the host in the reference precision, L[c][k] = Lc[k LS + c] rs_k, and held to

 * backward error  |A - L L^T|_ij <= B(T, D, min(i, j)) sqrt(a_ii a_jj) on every finite PD family (the entries of the
   published columns; for KS < D these lie in or below the leading block).  B is derived, not measured: Higham Thm 10.3 with
   the u of each division and square root replaced by the bounds test_gpu_so3_primitives.py pins for fast_rcp / fast_rsqrt
   (24 eps fp64, 2 eps fp32), one reciprocal and two rsqrt errors per column term -- chol_reference's docstring.
   chol_rows_to_lds scales its columns by rsqrt(pivot) as it goes: two rsqrt errors and j + 2 roundings per term, which the
   same B covers (the reciprocal's share of B is 4 u in fp32).
 * forward error   ||L_H - Lref_H||_F / ||Lref_H||_F <= c kappa_2(H) B on the graded-condition family, c = sqrt(D / 2) /
   (1 - kappa_2(H) sqrt(D) B): Higham Thm 10.8 (Sun) applied to the unit-diagonal scaling H.
 * verdict         ok on every clearly-PD input (lambda_min(H) >= m = D B), not ok on every clearly-indefinite one
   (<= -m; Demmel's condition, Higham Thm 10.7), not ok for a NaN or a zero pivot in any row the variant factorises (rows
   < KS); for KS < D a first bad pivot at a position >= KS reports ok, and the same matrix under (D, RT + 3) does not.
 * ok implies a usable factor: every published entry, every rs and every load_column value is finite.  Rows >= KS of a
   short variant are copied out unexamined by design ("pivots KS.. are then not checked": the complete factorisation that
   follows owns them), so the non-finite inputs of this assertion are those of rows < KS.
 * KS and PUB change nothing else: columns [0, PUB) and rs of lanes < PUB are bit-identical to the full variant.
 * published shape: exact +0 above the diagonal, nothing stored beyond row D - 1 or column PUB - 1 (the NaN prefill is still
   there), load_column of lanes >= D exactly zero.
 * neighbour independence, bit for bit: the result of a record among benign wave-mates is its result at every row position
   beside a NaN, an indefinite, an Inf matrix and a matrix of another family, with another large finite fill beyond the
   diagonal, in the ragged tail of the launch, and loaded through load_row from the packed triangle.

Largest |A - L L^T|_ij / (B sqrt(a_ii a_jj)) observed on the MI355X per family (a record; the bound is the derivation's):

    variant                 well    cond    scale   block
    f64-D12-KS12-PUB12      0.427   0.335   0.325   0.388
    f64-D12-KS6-PUB6        0.427   0.335   0.325   0.388
    f64-D12-KS12-PUB6       0.427   0.335   0.325   0.388
    f64-D13-KS13-PUB13      0.160   0.405   0.432   0.322
    f64-D13-KS6-PUB6        0.160   0.405   0.432   0.322
    f64-D13-KS3-PUB3        0.157   0.405   0.432   0.243
    f64-D13-KS13-PUB3       0.157   0.405   0.432   0.243
    f32-D12-KS12-PUB12      0.254   0.212   0.211   0.233
    f32-D12-KS6-PUB6        0.254   0.212   0.211   0.233
    f32-D12-KS12-PUB6       0.254   0.212   0.211   0.233
    f32-D13-KS13-PUB13      0.242   0.204   0.193   0.225
    f32-D13-KS6-PUB6        0.242   0.204   0.193   0.225
    f32-D13-KS3-PUB3        0.191   0.204   0.193   0.225
    f32-D13-KS13-PUB3       0.191   0.204   0.193   0.225
    f32-D12-KS12-PUB12-G32  0.309   0.241   0.276   0.246
    f32-D12-KS12-PUB12-G64  0.309   0.241   0.276   0.246
    f32-D13-KS13-PUB13-G32  0.285   0.211   0.253   0.242
    f32-D13-KS13-PUB13-G64  0.285   0.211   0.253   0.242

(forward error on the graded-condition family: at most 0.0026 of its bound; the emulation of tests/test_chol_reference.py, whose
primitive errors are drawn up to the pinned bounds, reaches 0.5 - 0.8 of B.)
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytest.importorskip("mpmath")

import chol_reference as R  # noqa: E402
from probe_support import load  # noqa: E402

IN, OK, RS, LC, COL, OUT = 176, 0, 1, 17, 225, 481     # doubles per record and offsets (tests/cpp/chol_probe.hip CHP_*)
PACKED, ROWS = 0, 1
F64, F32 = R.F64, R.F32
# large finite values beyond the diagonal of the rows form (load_row's contract: finite)
FILLS = {F64: (2.0 ** 1000, -(2.0 ** 900)), F32: (2.0 ** 100, -(2.0 ** 120))}
# (D, KS, PUB, G) of the probe's variant table, G = 0: chol16.  The probe is asked for its own table (and LS) at run time and
# must agree; listed here so that the cases can be collected without the library.
TUNED = [(12, 12, 12), (12, 6, 6), (12, 12, 6), (13, 13, 13), (13, 6, 6), (13, 3, 3), (13, 13, 3)]
GENERIC = [(12, 32), (12, 64), (13, 32), (13, 64)]
CASES = [(p, d, ks, pub, 0) for p in (F64, F32) for d, ks, pub in TUNED] + [(F32, d, d, d, g) for d, g in GENERIC]
IDS = [f"{'f64' if p == F64 else 'f32'}-D{d}-KS{ks}-PUB{pub}" + (f"-G{g}" if g else "") for p, d, ks, pub, g in CASES]
FULL_CASES = [c for c in CASES if c[3] == c[1]]
FULL_IDS = [i for c, i in zip(CASES, IDS) if c[3] == c[1]]
SHORT_CASES = [c for c in CASES if c[4] == 0 and (c[2], c[3]) != (c[1], c[1])]
SHORT_IDS = [i for c, i in zip(CASES, IDS) if c in SHORT_CASES]


# ------------------------------------------------------------------------------------------------------------ the device
def _lib():
    return load("libchol_probe",
                chol_probe=(C.c_int, (C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double))),
                chol_probe_variant=(C.c_int, (C.c_int, C.c_int, C.POINTER(C.c_int))))


@functools.lru_cache(maxsize=None)
def variant(prec, D, KS, PUB, G):
    """(index in the probe's table, LS): the first entry with these parameters"""
    lib = _lib()
    info = (C.c_int * 5)()
    for v in range(lib.chol_probe_variant(-1, prec, info)):
        lib.chol_probe_variant(v, prec, info)
        if tuple(info[:4]) == (D, KS, PUB, G):
            return v, int(info[4])
    raise KeyError((D, KS, PUB, G))


def test_probe_table_matches_the_cases():
    """every (D, KS, PUB, G) of the probe's table is a case here and the reverse (no GPU: the table is host data)"""
    lib = _lib()
    info = (C.c_int * 5)()
    table = set()
    for v in range(lib.chol_probe_variant(-1, 0, info)):
        lib.chol_probe_variant(v, 0, info)
        table.add(tuple(info[:4]))
    assert table == {c[1:] for c in CASES}


def device(v, prec, D, form, X):
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert X.ndim == 2 and X.shape[1] == IN
    Y = np.zeros((X.shape[0], OUT))
    rc = _lib().chol_probe(v | (form << 8), prec, D, X.shape[0], X.ctypes.data_as(C.POINTER(C.c_double)),
                           Y.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, rc
    return Y


def rows_form(A, fill):
    """records of the rows form: the lower triangle and the diagonal from A, the caller's fill beyond the diagonal"""
    n, D, _ = A.shape
    X = np.zeros((n, IN))
    X[:, :D * D] = np.where(np.tri(D, dtype=bool)[None], A, fill).reshape(n, D * D)
    return X


def packed_form(A):
    n, D, _ = A.shape
    X = np.zeros((n, IN))
    i, j = np.tril_indices(D)
    X[:, :len(i)] = A[:, i, j]
    return X


# -------------------------------------------------------------------------------------------------------------- inputs
SETS = R.FINITE_PD + ("indef", "nan", "inf", "zero_row", "dup_row")


@functools.lru_cache(maxsize=None)
def records(prec, D):
    """all matrices of one (T, D), the set of every record and the slice of every set"""
    parts, span, n0 = [], {}, 0
    for name in SETS:
        A = R.family(name, prec, D) if name in R.FINITE_PD + ("indef",) else R.special(name, prec, D)[0]
        parts.append(A)
        span[name] = slice(n0, n0 + len(A))
        n0 += len(A)
    return np.concatenate(parts), span


def placements(prec, D, FPW, tail):
    """Record order of one launch, as indices into records() -- the idea of placements() in probe_support.py:
    every record at row 0 among copies of one benign matrix (its base result), then a subset of targets at each of the FPW
    row positions with a NaN, an indefinite, an Inf matrix and a matrix of another family in the other rows, then `tail`
    records that leave the last wavefront ragged (rows past the end re-evaluate the last record)."""
    A, span = records(prec, D)
    n = len(A)
    benign = span["well"].start + 1
    src = np.full((n, FPW), benign)
    src[:, 0] = np.arange(n)
    src = [src.ravel()]
    foreign = [span["nan"].start, span["indef"].start + 40, span["inf"].start, span["scale"].start, span["inf"].start + 4]
    targets = np.concatenate([np.arange(span[s].start, span[s].stop, st) for s, st in
                              (("well", 9), ("cond", 6), ("scale", 5), ("block", 5), ("indef", 8), ("nan", 7), ("inf", 7),
                               ("zero_row", 3), ("dup_row", 5))])
    for t in targets:
        other = span["well"].start if span["scale"].start <= t < span["scale"].stop else span["scale"].start
        f = [foreign[0], foreign[1], foreign[2], other, foreign[4]]
        for p in range(FPW):
            w = [f[(p + q) % len(f)] for q in range(FPW)]
            w[p] = t
            src.append(np.array(w))
    src.append(np.arange(tail))
    return np.concatenate(src), n


def _same(a, b):
    """bit-identical rows (any NaN equals any NaN: the payload of a propagated NaN is not the matrix's business)"""
    eq = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return eq.all(axis=1)


@functools.lru_cache(maxsize=None)
def evaluate(prec, D, KS, PUB, G):
    """base result of every record (rows form, first fill, benign wave-mates) and the launch positions whose result differs
    from the base result of the same record: under other neighbours / in the tail, with the second fill, in the packed form"""
    v, LS = variant(prec, D, KS, PUB, G)
    FPW = 64 // G if G else 4
    A, span = records(prec, D)
    tail = 1 + v % 3
    src, n = placements(prec, D, FPW, tail)
    f1, f2 = FILLS[prec]
    Y = device(v, prec, D, ROWS, rows_form(A[src], f1))
    base = Y[0:n * FPW:FPW]
    moved = {"neighbours": src[~_same(Y, base[src])]}
    # the other fill and the packed form: four different records per wavefront, a ragged tail of another length
    t2 = 1 + (v + 1) % 3
    src2 = np.concatenate([np.arange(n), np.arange((t2 - n) % 4)])
    Y2 = device(v, prec, D, ROWS, rows_form(A[src2], f2))
    moved["fill"] = src2[~_same(Y2, base[src2])]
    if G == 0:
        Y3 = device(v, prec, D, PACKED, packed_form(A[src2]))
        moved["packed"] = src2[~_same(Y3, base[src2])]
    return dict(base=base, LS=LS, moved=moved, ragged=(len(src) % FPW, len(src2) % FPW))


def fields(prec, D, KS, PUB, G):
    e = evaluate(prec, D, KS, PUB, G)
    Y, LS = e["base"], e["LS"]
    Lc = Y[:, LC:LC + D * LS].reshape(-1, D, LS)                       # [record, column k, row c]
    col = Y[:, COL:COL + 256].reshape(-1, 16, 16)[:, :, :D]           # [record, lane, c]
    return Y[:, OK] != 0, Y[:, RS:RS + 16], Lc, col


# --------------------------------------------------------------------------------------------------------------- tests
@functools.lru_cache(maxsize=None)
def backward_ratios(prec, D, KS, PUB, G):
    """{family: (largest |A - L L^T|_ij / (B sqrt(a_ii a_jj)) over the entries of the published columns, its record)}"""
    A, span = records(prec, D)
    ok, rs, Lc, _ = fields(prec, D, KS, PUB, G)
    Bm = R.B_matrix(prec, D)
    pub = np.minimum.outer(np.arange(D), np.arange(D)) < PUB
    out = {}
    for name in R.FINITE_PD:
        worst, at = 0.0, -1
        for i in range(span[name].start, span[name].stop):
            res = np.abs(R.residual_from_device(A[i], Lc[i, :PUB, :D], rs[i, :PUB], prec))
            d = np.sqrt(np.diag(A[i]))
            w = float(np.where(pub, res / (Bm * np.outer(d, d)), 0.0).max())
            w = np.inf if np.isnan(w) else w
            if w > worst:
                worst, at = w, i
        out[name] = (worst, at)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec,D,KS,PUB,G", CASES, ids=IDS)
def test_backward_error(prec, D, KS, PUB, G):
    r = backward_ratios(prec, D, KS, PUB, G)
    print("observed/bound", {k: round(v[0], 4) for k, v in r.items()})
    for name, (w, at) in r.items():
        assert w <= 1.0, (name, w, at)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,D,KS,PUB,G", FULL_CASES, ids=FULL_IDS)
def test_forward_error(prec, D, KS, PUB, G):
    A, span = records(prec, D)
    ok, rs, Lc, _ = fields(prec, D, KS, PUB, G)
    worst, covered = 0.0, 0
    for i in range(span["cond"].start, span["cond"].stop):
        d = 1.0 / np.sqrt(np.diag(A[i]))
        lam = np.linalg.eigvalsh(R.unit_diagonal(A[i]))
        lmin = R.lambda_min_H(A[i], prec)
        bound = R.forward_bound(prec, D, lam[-1] / lmin)
        covered += np.isfinite(bound)
        L = np.tril((Lc[i, :, :D] * rs[i, :D, None]).T) * d[:, None]
        Lref = R.ref_chol(A[i], prec) * d[:, None]
        err = np.linalg.norm(L - Lref) / np.linalg.norm(Lref)
        worst = max(worst, err / bound)
        assert err <= bound, (i, err, bound, lam[-1] / lmin)
    # every decade of the family is inside the theorem's range; only the draws pushed to the margin can leave it
    assert covered >= 16 * len(R.cond_decades(prec, D))
    print("forward error / bound, worst:", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,D,KS,PUB,G", CASES, ids=IDS)
def test_verdict(prec, D, KS, PUB, G):
    A, span = records(prec, D)
    ok = fields(prec, D, KS, PUB, G)[0]
    for name in R.FINITE_PD:
        assert ok[span[name]].all(), (name, np.nonzero(~ok[span[name]])[0][:8].tolist())
    pos = R.indef_position(D)
    got = ok[span["indef"]]
    assert (got == (pos >= KS)).all(), np.nonzero(got != (pos >= KS))[0][:8].tolist()
    for name in ("nan", "zero_row"):
        row = R.special(name, prec, D)[1][:, 0]
        got = ok[span[name]]
        assert (got == (row >= KS)).all(), (name, np.nonzero(got != (row >= KS))[0][:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("prec,D,KS,PUB,G", CASES, ids=IDS)
def test_ok_implies_a_usable_factor(prec, D, KS, PUB, G):
    A, span = records(prec, D)
    ok, rs, Lc, col = fields(prec, D, KS, PUB, G)
    examined = np.ones(len(A), dtype=bool)
    for name in ("nan", "inf"):
        examined[span[name]] = R.special(name, prec, D)[1][:, 0] < KS
    lanes = 16 if PUB == D else PUB        # lanes >= PUB of a short variant have no column of their own
    usable = (np.isfinite(Lc[:, :PUB, :D]).all(axis=(1, 2)) & np.isfinite(rs).all(axis=1)
              & (np.isfinite(col[:, :lanes]).all(axis=(1, 2)) if G == 0 else True))
    bad = np.nonzero(ok & examined & ~usable)[0]
    where = {name: int(((bad >= s.start) & (bad < s.stop)).sum()) for name, s in span.items()}
    assert bad.size == 0, (where, bad[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("prec,D,KS,PUB,G", SHORT_CASES, ids=SHORT_IDS)
def test_short_variants_change_nothing_they_publish(prec, D, KS, PUB, G):
    """columns [0, PUB) and rs of lanes < PUB: bit-identical to chol16<T, D, LS> on every finite input"""
    A, span = records(prec, D)
    _, rs, Lc, _ = fields(prec, D, KS, PUB, G)
    _, rsf, Lcf, _ = fields(prec, D, D, D, 0)
    finite = np.isfinite(A).all(axis=(1, 2))
    assert finite.sum() == len(A) - (span["nan"].stop - span["nan"].start) - (span["inf"].stop - span["inf"].start)
    same = _same(Lc[:, :PUB, :D].reshape(len(A), -1), Lcf[:, :PUB, :D].reshape(len(A), -1)) & _same(rs[:, :PUB], rsf[:, :PUB])
    assert same[finite].all(), np.nonzero(finite & ~same)[0][:8].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("prec,D,KS,PUB,G", CASES, ids=IDS)
def test_published_shape(prec, D, KS, PUB, G):
    A, span = records(prec, D)
    ok, rs, Lc, col = fields(prec, D, KS, PUB, G)
    above = np.arange(D)[None, :] < np.arange(PUB)[:, None]               # [k, c]: c < k
    up = Lc[:, :PUB, :D][:, above]
    assert (up == 0).all() and not np.signbit(up).any(), "exact +0 above the diagonal"
    assert np.isnan(Lc[:, :, D:]).all(), "nothing stored beyond row D - 1"
    assert np.isnan(Lc[:, PUB:, :]).all(), "nothing stored beyond column PUB - 1"
    if G == 0 and PUB == D:
        finite = np.isfinite(Lc[:, :, :D]).all(axis=(1, 2)) & np.isfinite(rs).all(axis=1)
        assert finite[span["well"]].all()
        assert (col[finite][:, D:, :] == 0).all(), "load_column of lanes >= D"


@pytest.mark.gpu
@pytest.mark.parametrize("prec,D,KS,PUB,G", CASES, ids=IDS)
def test_neighbour_independence_and_loading(prec, D, KS, PUB, G):
    e = evaluate(prec, D, KS, PUB, G)
    if G == 0:
        assert e["ragged"][0] != 0 and e["ragged"][1] != 0 and e["ragged"][0] != e["ragged"][1]
    for what, idx in e["moved"].items():
        assert idx.size == 0, (what, idx[:8].tolist())


def observed():
    """the docstring table, from the device (re-measure after a kernel change)"""
    lines = []
    for c, name in zip(CASES, IDS):
        r = backward_ratios(*c)
        lines.append(f"    {name:<24}" + "".join(f"{r[f][0]:<8.3f}" for f in R.FINITE_PD).rstrip())
    return "\n".join(lines)
