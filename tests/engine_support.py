"""Helpers of the GPU tests that need an engine or torch, each defined once: engines, uploads and downloads, the packed lower
triangle, bit-level snapshots and the scaled error.  No tests here; the scenario of a feature lives with its reference
(tests/*_reference.py) or in its *_cases.py."""
import numpy as np
import torch

from oracle import ukf_numpy as on
from scaled_parity import f32r  # noqa: F401  (defined with the NumPy-only parity code; the GPU tests take it from here)

ACC_COV = 0.01 * np.eye(3)


def tdt(e):
    return torch.float64 if e.dtype == np.float64 else torch.float32


def man_of(model):
    return on.POSE if model == "pose" else on.ORIENT


# ---------------------------------------------------------------------------------------------------------------- engines
def new_engine(spe, model, n, prec, wide, **kw):
    cfg = dict(kw)
    if wide:
        cfg["wide_arithmetic"] = 1
    if model == "pose":
        return spe.BatchPoseUKF(n, precision=prec, **cfg)
    sy = spe.synth
    e = spe.BatchOrientationUKF(n, sy.ORIENT_TAU, sy.ORIENT_TAU, sy.ORIENT_LATITUDE, precision=prec, **cfg)
    e.set_process_noise(sy.orient_process_noise())
    return e


def cycled_engine(spe, model, n, prec, wide, skip_init=(), **kw):
    """an engine after two real cycles (Pose: acceleration branch, POS3; OrientationState: its body-velocity update)"""
    sy = spe.synth
    e = new_engine(spe, model, n, prec, wide, **kw)
    mu0, cov0 = sy.pose_initial(n) if model == "pose" else sy.orient_initial(n)
    if skip_init:
        for i in range(n):
            if i not in skip_init:
                e.initialize(mu0[i:i + 1], cov0[i:i + 1], first=i)
    else:
        e.initialize(mu0, cov0)
    for c in range(2):
        mu_now = e.state(with_cov=False)[0]
        if model == "pose":
            acc, z, Q = sy.pose_cycle_inputs(n, c, mu_now[:, :3])
            e.set_acceleration(acc, ACC_COV)
            e.cycle(0.01, spe.MEAS_POS3, z, Q)
        else:
            gyro, acc, z, Q = sy.orient_cycle_inputs(n, c, mu_now[:, 0:4])
            e.set_orient_inputs(gyro, acc)
            e.cycle(0.01, spe.MEAS_ORIENT_BODYVEL3, z, Q)
    return e


class Case:
    """the state of an engine as downloaded, and inputs as stored; fresh engines are initialised from it"""


def engine_of(spe, c, **kw):
    """a fresh engine holding the state of the case bit for bit"""
    e = new_engine(spe, c.model, c.n, c.prec, c.wide, **kw)
    e.initialize(c.mu, c.cov)
    m, C, _ = e.state()
    assert np.array_equal(m, c.mu) and np.array_equal(C, c.cov)   # the downloaded state goes back in bit for bit
    return e


# ---------------------------------------------------------------------------------------------- host <-> device, storage
def dev(e, x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype or tdt(e))


def host(t):
    return t.double().cpu().numpy()


class _DevArray:
    """Zero-copy torch view of engine-owned device memory (CUDA array interface)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def dev_state(eng):
    """(mean, packed covariance) of an engine as torch tensors over its own HBM buffers."""
    eng.sync()
    mu_p, cov_p, _ = eng.device_views()
    ts = "<f8" if eng.precision == 0 else "<f4"
    return (torch.as_tensor(_DevArray(mu_p, (eng.capacity, eng.S), ts), device="cuda"),
            torch.as_tensor(_DevArray(cov_p, (eng.capacity, eng.PK), ts), device="cuda"))


def stored(x, dtype):
    """x as an engine of that dtype holds it (fp32 engines round their inputs), in double"""
    return np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)


def pack(M):
    """[..., D, D] -> [..., PK] packed lower triangle (row r at r (r + 1) / 2 ... + r)"""
    r, c = np.tril_indices(M.shape[-1])
    return np.ascontiguousarray(M[..., r, c])


def unpack(packed, D):
    """[..., PK] packed lower triangle -> [..., D, D] symmetric"""
    C = np.zeros(packed.shape[:-1] + (D, D))
    r, c = np.tril_indices(D)
    C[..., r, c] = packed
    C[..., c, r] = packed
    return C


# ------------------------------------------------------------------------------------------------------------ comparisons
def scaled(x, ref):
    """max |x - ref| / (1 + |ref|); NaN anywhere gives NaN, which fails every `<= tol`"""
    return float(np.max(np.abs(x - ref) / (1.0 + np.abs(ref)))) if np.size(x) else 0.0


def scaled_ignoring_nan(x, ref):
    """scaled() over the entries that are not NaN: only next to a check that the NaNs themselves agree"""
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(x - ref) / (1.0 + np.abs(ref)))) if np.size(x) else 0.0


def same(a, b, keys, rows=None):
    """bit equality of two dicts of arrays on `keys`, NaN equal to NaN; rows: a selection of filters"""
    rows = slice(None) if rows is None else rows
    return all(np.array_equal(a[k][rows], b[k][rows], equal_nan=True) for k in keys)


def snapshot(e, noise_of=None):
    """everything of the engine that can be downloaded: mean, covariance, initialised flags, status, last measurement times, the
    process noise of the filters `noise_of` (default: every filter), and the latched rotation rate where there is a getter
    (OrientationState)"""
    mu, cov, init = e.state()
    noise = np.array([e.process_noise(i) for i in (range(e.capacity) if noise_of is None else noise_of)])
    latch = e.rotation_rate() if e.model == 1 else np.zeros(0)
    return mu, cov, init, e.status(), e.last_measurement_time(), noise, latch


def same_snapshot(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
