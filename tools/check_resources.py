#!/usr/bin/env python3
"""Build gate for EVERY shipped kernel instantiation (the name fragments of GATED below): no scratch and no AGPRs, and
the tuned kernels keep the wavefronts per SIMD their design counts on (fp64: three, fp32: five) -- a register regression
that costs a wavefront fails the build instead of showing up as a slower bench line.

ROCm 7.2's hipcc places VGPR spill / live-range-split copies at the join label of a divergent `if`
in front of the EXEC restore; reached through s_cbranch_execz they save nothing (see the note in
slam-pose_estimation_amd/csrc/ukf_kernel16.hpp).  A kernel that needs spills is therefore
rejected at build time instead of being trusted.  Usage: check_resources.py <hipcc remark log>..."""
import re
import sys


def parse(text):
    out, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            out.append(cur)
            continue
        for key, pat in (("vgpr", r"remark:\s+VGPRs: (\d+)"), ("agpr", r"remark:\s+AGPRs: (\d+)"),
                         ("scratch", r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"remark:\s+Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds", r"remark:\s+LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


# every kernel whose name holds one of these fragments is gated
GATED = ("ukf_kernel", "ukf_innovation_kernel", "ukf_bank_", "ukf_smooth_kernel", "ukf_forecast_kernel", "ukf_lifecycle_",
         "ukf_state_meas_kernel", "ukf_sensor_meas_kernel", "ukf_sampled_kernel", "ukf_sigma_points_kernel",
         "ukf_predict_sampled_kernel", "ukf_delayed_kernel", "ukf_condition_kernel", "ukf_bearing_kernel", "ukf_associate_kernel",
         "ukf_relative_kernel", "ukf_robust_kernel", "ukf_delayed_sensor_kernel", "ukf_pda_kernel", "ukf_assign_kernel",
         "ukf_weighted_kernel", "ukf_jpda_kernel")

# (name fragments, fragments that exclude, wavefronts per SIMD the kernel must keep, what the error calls it), checked in this
# order.  The tuned kernels (the register side; LDS is checked by the layout's static_asserts): ukf_kernel16<double, ...> three
# wavefronts per SIMD (<= 168 VGPRs), ukf_kernel16<float, ...> five (<= 96); --no-occupancy-floor lifts these two.  The feature
# kernels are sized for two in either precision: that is their launch bound; in fp64 their LDS slices (15 ... 38 KB per
# workgroup) admit one to two, in fp32 two to three.
TUNED = "tuned"
FLOORS = (
    (("ukf_kernel16Id",), (), 3, "tuned fp64 kernels", TUNED),
    (("ukf_kernel16I",), ("ukf_kernel16Id",), 5, "tuned fp32 kernels", TUNED),
    (("ukf_state_meas_kernel",), (), 2, "state-measurement kernels", None),
    (("ukf_sensor_meas_kernel",), (), 2, "sensor-measurement kernels", None),
    (("ukf_sampled_kernel", "ukf_sigma_points_kernel"), (), 2, "sampled-update / sigma-point kernels", None),
    (("ukf_predict_sampled_kernel",), (), 2, "sampled-prediction kernels", None),
    (("ukf_delayed_kernel",), (), 2, "delayed-measurement kernels", None),
    (("ukf_condition_kernel",), (), 2, "conditioning kernels", None),
    (("ukf_bearing_kernel",), (), 2, "bearing kernels", None),
    (("ukf_associate_kernel",), (), 2, "sensor-association kernels", None),
    (("ukf_forecast_kernel",), (), 2, "forecast kernels", None),
    (("ukf_relative_kernel",), (), 2, "relative-measurement kernels", None),
    (("ukf_robust_kernel",), (), 2, "robust sensor-measurement kernels", None),
    (("ukf_delayed_sensor_kernel",), (), 2, "delayed sensor-frame kernels", None),
    (("ukf_pda_kernel",), (), 2, "probabilistic-association kernels", None),
    (("ukf_weighted_kernel",), (), 2, "weighted-update kernels", None),
)


def main(paths):
    # --allow-agpr: diagnostic builds with the fp64 one-wavefront-per-filter kernels (make GENERIC_F64=1)
    allow_agpr = "--allow-agpr" in paths
    # (a log named by two patterns of the command line -- ukf_delayed_*.remarks also names ukf_delayed_sensor_*.remarks -- is read once)
    paths = list(dict.fromkeys(p for p in paths if not p.startswith("--")))
    bad, rows = [], []
    for p in paths:
        for k in parse(open(p).read()):
            if not any(frag in k["name"] for frag in GATED):
                continue
            rows.append(k)
            if k.get("scratch", 0) or (k.get("agpr", 0) and not allow_agpr):
                bad.append(k)
    for k in rows:
        print(f"{k['name'][:70]:70s} vgpr={k.get('vgpr')} agpr={k.get('agpr')} scratch={k.get('scratch')} "
              f"occ={k.get('occupancy')}")
    if bad:
        print("ERROR: kernels with scratch or AGPR spills (unsafe with this toolchain):", [b["name"] for b in bad])
        return 1
    for frags, excluded, floor, what, kind in FLOORS:
        if kind == TUNED and "--no-occupancy-floor" in sys.argv:
            continue
        low = [k for k in rows if any(frag in k["name"] for frag in frags) and not any(frag in k["name"] for frag in excluded)
               and k.get("occupancy", 0) < floor]
        if low:
            print(f"ERROR: {what} below their floor of {floor} wavefronts per SIMD:",
                  [(k["name"], k.get("vgpr"), k.get("occupancy")) for k in low])
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
