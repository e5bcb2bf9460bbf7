"""The filter lifecycle's entry points without a GPU: the symbols of include/ukf_batch.h are exported, bound and documented, the
host decisions of ukf_host.hpp (check_lifecycle_args, check_compact_args, lifecycle_geometry) hold under ASan / UBSan
(tests/cpp/lifecycle_host.cpp, compiled here as a stand-alone program), and a NULL engine is refused before anything touches a
device."""
import ctypes as C
import os

import lifecycle_reference as lr
from host_support import header_text, run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ukfb_gather_filters_dev", "ukfb_scatter_filters_dev", "ukfb_retire_dev", "ukfb_compact_dev", "ukfb_gather_filters",
         "ukfb_scatter_filters", "ukfb_compact")


def test_symbols_and_bindings(spe):
    lib = spe.load_library()
    header = header_text()
    for name in NAMES:
        assert name in spe.engine.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    for method in ("gather_filters_dev", "scatter_filters_dev", "retire_dev", "compact_dev", "gather_filters", "scatter_filters",
                   "compact"):
        assert callable(getattr(spe.BatchUKF, method))
    section = header[header.index("---- filter lifecycle"):header.index("int ukfb_compact(")]
    for text in ("typedef struct ukfb_filter_records", "READ-ONLY", "LOWEST item index wins", "UKFB_ST_INACTIVE",
                 "ukfb_set_process_noise_per_filter", "must not overlap", "IN PLACE", "old_index_dev", "ukfb_last_model_groups",
                 "ukfb_group_shard", "UKFB_ERR_OUT_OF_RANGE", "capacity % group == 0", "NOT moved"):
        assert text in section, text
    # the binding's struct has the header's fields, in its order
    fields = [f[0] for f in spe.engine.FilterRecords._fields_]
    struct = section[section.index("typedef struct ukfb_filter_records"):section.index("} ukfb_filter_records;")]
    assert fields == ["mu", "cov_packed", "last_ts_us", "initialised", "in_a", "in_b", "noise", "status"]
    assert [struct.index(" " + f + ";") for f in fields] == sorted(struct.index(" " + f + ";") for f in fields)
    assert C.sizeof(spe.engine.FilterRecords) == 8 * C.sizeof(C.c_void_p)
    batch = open(os.path.join(ROOT, "include", "pose_estimation", "Batch.hpp")).read()
    for call in ("ukfb_gather_filters(", "ukfb_scatter_filters(", "ukfb_retire_dev(", "ukfb_compact("):
        assert call in batch, call
    for method in ("gatherFilters(", "scatterFilters(", "retire(", "compact("):
        assert method in batch, method


def test_null_engine_is_refused(spe):
    lib = spe.load_library()
    rec = spe.engine.FilterRecords()
    buf = (C.c_double * 512)(); idx = (C.c_int32 * 4)(); mask = (C.c_uint8 * 4)()
    assert lib.ukfb_gather_filters_dev(None, C.c_int64(1), idx, C.byref(rec)) == 1   # UKFB_ERR_INVALID_ARG
    assert lib.ukfb_scatter_filters_dev(None, C.c_int64(1), idx, C.byref(rec)) == 1
    assert lib.ukfb_retire_dev(None, mask) == 1
    assert lib.ukfb_compact_dev(None, C.c_int(1), None, None, None) == 1
    assert lib.ukfb_gather_filters(None, C.c_int64(1), idx, buf, buf, None, None) == 1
    assert lib.ukfb_scatter_filters(None, C.c_int64(1), idx, buf, buf, None, None, None) == 1
    assert lib.ukfb_compact(None, C.c_int(1), None, None, None) == 1


def test_host_decisions_under_sanitizers(tmp_path):
    # the capacity of the GPU compact test: the program asserts that it spans three count blocks with a ragged last one
    run_sanitized("lifecycle_host.cpp", tmp_path, args=(lr.COMPACT_N,))
