"""The host half of the feature launches without a GPU: the choice of instantiation by precision and model, the commit rule,
the process block and its input precedence, the rounding of every scalar through the storage type and the sensor-frame inputs
of ukf_feature_bind.hpp, under ASan / UBSan (tests/cpp/feature_launch_host.cpp, compiled here as a stand-alone program that
links no HIP: the engine's header needs the HIP headers for its types only)."""
import os

from host_support import run_sanitized

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_feature_launch_binders_under_sanitizers(tmp_path):
    run_sanitized("feature_launch_host.cpp", tmp_path,
                  extra_flags=("-isystem", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__=1"))
