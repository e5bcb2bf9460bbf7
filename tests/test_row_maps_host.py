"""The LDS maps of the row-layout kernels without a GPU: every *_map of ukf_host.hpp lists its regions in ascending order
without overlap, keeps its aliases inside the table they alias and sums to the pinned totals, under ASan / UBSan
(tests/cpp/row_maps_host.cpp, compiled here as a stand-alone program)."""
from host_support import run_sanitized


def test_row_maps_under_sanitizers(tmp_path):
    run_sanitized("row_maps_host.cpp", tmp_path)
