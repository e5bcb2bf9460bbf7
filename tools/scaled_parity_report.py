#!/usr/bin/env python3
"""profiles/scaled_parity.txt: the whitened per-block distances behind tests/test_gpu_scaled_parity.py.

    python tools/scaled_parity_report.py --cpu [out]   the CPU table: the C++ float oracle and the all-float32 NumPy evaluation
                                                       against the fp64 oracle, and M (no GPU)
    python tools/scaled_parity_report.py [out]         on an MI355X: APPENDS the engine's distances and bounds for every mode
                                                       (fp64, fp32, fp32 wide), model and path (predict, update, fused cycle,
                                                       three cycles in one launch)

    python tools/scaled_parity_report.py --features --cpu [out]   profiles/feature_scaled_parity.txt: the CPU table behind
                                                       M_feat (tests/test_feature_scaled_reference.degenerate_spread), no GPU
    python tools/scaled_parity_report.py --features [out]         on an MI355X: runs the parity tests of the feature files and
                                                       APPENDS, per family, model and mode, the largest distance of every
                                                       block over all their comparisons beside the bound of that comparison
                                                       (--only=NAME: the files whose name contains NAME, e.g. a new family)

M, M_feat and every bound come from the CPU tables alone; the GPU tables are there to be read beside them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def cpu(out):
    import slam_pose_estimation_amd as spe
    import scaled_parity as sp
    rows, m = sp.fp32_spread(spe)
    text = sp.spread_text(rows, m)
    rows_i, m_i = sp.fp32_spread(spe, kernel_ident=True)
    worst = max(rows_i, key=lambda r: r[6] or 0)
    text += ("\n# for information: with the engine's exact identities for affine components (study_f32_mixed.Prec.kernel_ident, "
             f"DESIGN.md 4.2)\n# the NumPy evaluation is far CLOSER to fp64 than the float oracle where the float oracle is "
             f"coarsest: {worst[0]} {worst[1]} {worst[2]}\n# float oracle {worst[3]:.3e}, NumPy {worst[4]:.3e} (ratio {worst[6]:.1f})."
             "  That is another algorithm, not another rounding of the same one, and\n# it errs on the side the bound "
             "max(M d_o32, floor) already allows: it does not enter M.\n")
    with open(out, "w") as f:
        f.write(text)
    print(text)


def gpu(out):
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import numpy as np
    import slam_pose_estimation_amd as spe
    import scaled_parity as sp
    import test_gpu_scaled_parity as t
    dt = t.DT
    lines = ["", "# GPU (MI355X): engine <-> reference, whitened block distances beside their bounds (tests/scaled_parity.py); n = 203",
             f"# M = {sp.M}"]
    for mode in sp.MODES:
        for model in t.MODELS:
            c = t._case(spe, model, mode)
            zs = [c.z_for(c.full3, k) for k in range(3)]
            z_r, Q_r = t._ring(c, zs), t._ring(c, [c.Q] * 3)
            paths = {
                "predict": (lambda e: e.predict(dt), [("predict", dt), ("commit",)]),
                "update": (lambda e: e.update(c.full3, c.z, c.Q), [("update", c.full3, c.z, c.Q), ("commit",)]),
                "cycle": (lambda e: e.cycle_dev(dt, c.full3, z_r[0], Q_r[0]), [("predict", dt), ("update", c.full3, zs[0], c.Q), ("commit",)]),
                "three cycles": (lambda e: e.cycle_multi_dev(3, dt, c.full3, z_r, Q_r, 3, 0),
                                 sum(([("predict", dt), ("update", c.full3, zs[k], c.Q), ("commit",)] for k in range(3)), [])),
            }
            for path, (run, ops) in paths.items():
                e = t._engine(c)
                run(e)
                m, cv, _ = e.state()
                rep = []
                try:
                    sp.judge(c, ops, m, cv, e.status(), path, report=rep)
                    verdict = "within bounds"
                except AssertionError as err:
                    verdict = f"OVER: {err}"
                lines.append(f"## {mode} {model} {path}: {e.last_launch_info()['kernel']}  {verdict}")
                if rep:
                    lines.append(sp.table(rep[0][1], rep[0][2]))
                e.close()
    text = "\n".join(lines) + "\n"
    with open(out, "a") as f:
        f.write(text)
    print(text)


def features_cpu(out):
    import slam_pose_estimation_amd as spe
    import test_feature_scaled_reference as t
    text = t.spread_text(*t.degenerate_spread(spe)) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


FEATURE_FILES = ("test_gpu_innovation.py", "test_gpu_bank.py", "test_gpu_smooth.py", "test_gpu_state_meas.py", "test_gpu_sensor_meas.py",
                 "test_gpu_predict_sampled.py")


ONLY = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]   # --only=predict_sampled: that family's file alone


def features_gpu(out):
    import pytest
    import feature_scaled_parity as fsp
    del fsp.REPORT[:]
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", "parity or against_the_reference or agree or mean_iteration_cap or several_mean_iterations"]
                     + [os.path.join(ROOT, "tests", f) for f in FEATURE_FILES if not ONLY or any(o in f for o in ONLY)])
    groups = {}
    for name, mode, kind, rows in fsp.REPORT:   # names are family/model/...
        family, model = name.split("/")[:2]
        g = groups.setdefault((family, model, mode), {"n": 0, "rows": {}})
        g["n"] += 1
        for label, d, b in rows:
            old = g["rows"].get(label)
            if old is None or d / b > old[0] / old[1]:
                g["rows"][label] = (d, b, name)
    lines = ["", "# GPU (MI355X): engine <-> reference, whitened distances beside their bounds (tests/feature_scaled_parity.py), per family,",
             "# model and mode: of all the comparisons the feature files make, the one where each block comes closest to its bound"
             + (f" (only: {', '.join(ONLY)})" if ONLY else ""),
             f"# M_feat = {fsp.M_FEAT}; pytest exit code {int(rc)}"]
    for (family, model, mode), g in sorted(groups.items()):
        top = max(g["rows"].values(), key=lambda r: r[0] / r[1])
        lines.append(f"## {family} {model} {mode}: {g['n']} comparisons, largest fraction of a bound {top[0] / top[1]:.3f}")
        for label, (d, b, name) in g["rows"].items():
            lines.append(f"  {label:38s} {d:10.3e}   bound {b:10.3e}   {d / b:7.3f}   {name}")
    text = "\n".join(lines) + "\n"
    with open(out, "a") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    feat = "--features" in sys.argv
    out = args[0] if args else os.path.join(ROOT, "profiles", "feature_scaled_parity.txt" if feat else "scaled_parity.txt")
    if feat:
        (features_cpu if "--cpu" in sys.argv else features_gpu)(out)
    else:
        (cpu if "--cpu" in sys.argv else gpu)(out)
