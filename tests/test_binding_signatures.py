"""The binding's statement of the C ABI (slam-pose_estimation_amd/abi.py) against include/ukf_batch.h, type by type.

The header is read with regular expressions: every ukfb_* prototype as a return type and parameter types, every
`typedef struct ukfb_* { ... }` body as member types with array extents.  The C spellings are mapped to ctypes through the
dictionaries below, which state the binding's rules from the header's side; a spelling they do not know fails the test, so a
new header type cannot slip through.  Nothing here touches a device: the calls at the end pass a NULL engine or compute
on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P = C.POINTER

# scalars by exact width and signedness
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double}

# parameters: arrays by their element (a `const double[3]` parameter is a pointer); opaque handles and untyped device addresses
# as addresses; handle and device-pointer out-parameters and per-shard pointer arrays as arrays of addresses
PARAMETERS = dict(SCALARS)
PARAMETERS.update({
    "const double*": P(C.c_double), "double*": P(C.c_double), "const double[3]": P(C.c_double),
    "const int32_t*": P(C.c_int32), "int32_t*": P(C.c_int32),
    "const int64_t*": P(C.c_int64), "int64_t*": P(C.c_int64),
    "const uint8_t*": P(C.c_uint8), "uint8_t*": P(C.c_uint8),
    "uint32_t*": P(C.c_uint32), "float*": P(C.c_float), "const int*": P(C.c_int), "int*": P(C.c_int),
    "ukfb_engine*": C.c_void_p, "const ukfb_engine*": C.c_void_p, "ukfb_group*": C.c_void_p, "const ukfb_group*": C.c_void_p,
    "void*": C.c_void_p, "const void*": C.c_void_p,
    "ukfb_engine**": P(C.c_void_p), "ukfb_group**": P(C.c_void_p), "void**": P(C.c_void_p), "uint32_t**": P(C.c_void_p),
    "const void* const*": P(C.c_void_p), "void* const*": P(C.c_void_p), "const int32_t* const*": P(C.c_void_p),
    "char*": C.c_char_p,
})
RETURNS = {"int": C.c_int, "const char*": C.c_char_p}

# struct members: the header's structs hold device addresses, typed or not, which the binding fills from tensors and plain
# ints (c_void_p); the one host array among them is the `const double*` window of ukfb_delayed_in
MEMBERS = dict(SCALARS)
MEMBERS.update({
    "void*": C.c_void_p, "const void*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p, "int64_t*": C.c_void_p,
    "uint32_t*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p,
    "const double*": P(C.c_double),
})


def header_text():
    text = open(os.path.join(ROOT, "include", "ukf_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))


def spelling(declaration):
    """`const double* dt` -> "const double*", `double mount_uniform[7]` -> "double[7]": the type without the name"""
    m = re.fullmatch(r"(.*?)\b(\w+)((?:\[\w*\])*)", " ".join(declaration.split()))
    assert m and m.group(1).strip(), f"unreadable declaration: {declaration!r}"
    return re.sub(r"\s+\*", "*", m.group(1).strip()) + m.group(3)


def header_prototypes():
    """name -> (return spelling, [parameter spellings])"""
    found = re.findall(r"\b(int|const\s+char\s*\*)\s*(ukfb_\w+)\s*\(([^)]*)\)\s*;", header_text())
    protos = {}
    for ret, name, params in found:
        assert name not in protos, f"{name} is declared twice"
        params = [] if params.strip() in ("", "void") else [spelling(p) for p in params.split(",")]
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), params)
    return protos


def header_structs():
    """struct name -> [(member name, type spelling, extent or None)], a declaration `int a, b;` giving two members"""
    structs = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(ukfb_\w+)\s*\{(.*?)\}\s*(\w+)\s*;", header_text(), flags=re.S):
        assert name == alias
        members = []
        for decl in (d for d in body.split(";") if d.strip()):
            first, *more = [part.strip() for part in decl.split(",")]
            base = re.sub(r"\[\w*\]", "", spelling(first))
            for part in [first] + [f"{base} {p}" for p in more]:
                m = re.fullmatch(r".*?\b(\w+)(?:\[(\d+)\])?", part)
                members.append((m.group(1), base, int(m.group(2)) if m.group(2) else None))
        structs[name] = members
    return structs


def structure_of(spe, struct_name):
    """ukfb_state_meas_out -> spe.StateMeasOut"""
    return getattr(spe.abi, "".join(word.capitalize() for word in struct_name[len("ukfb_"):].split("_")))


def map_parameter(spe, c_type):
    m = re.fullmatch(r"(?:const )?(ukfb_\w+)\*", c_type)
    if m and m.group(1) in header_structs():
        return P(structure_of(spe, m.group(1)))
    assert c_type in PARAMETERS, f"no ctypes mapping for the parameter type {c_type!r}"
    return PARAMETERS[c_type]


def test_the_header_parses_completely(spe):
    protos = header_prototypes()
    assert len(protos) == 122
    assert sorted(protos) == sorted(spe.EXPORTS)
    assert {ret for ret, _ in protos.values()} == {"int", "const char*"}
    assert spe.EXPORTS == list(spe.abi.SIGNATURES) and spe.engine.EXPORTS is spe.abi.EXPORTS


def test_every_signature_is_the_headers(spe):
    protos = header_prototypes()
    assert set(spe.abi.SIGNATURES) == set(protos)
    for name, (ret, params) in protos.items():
        restype, argtypes = spe.abi.SIGNATURES[name]
        assert restype is RETURNS[ret], name
        assert len(argtypes) == len(params), name
        for i, (c_type, argtype) in enumerate(zip(params, argtypes)):
            assert argtype is map_parameter(spe, c_type), f"{name}: argument {i} is {c_type} in the header"


def test_every_structure_is_the_headers(spe):
    structs = header_structs()
    assert "ukfb_config" in structs and "ukfb_filter_records" in structs
    assert structure_of(spe, "ukfb_config") is spe.Config and structure_of(spe, "ukfb_filter_records") is spe.FilterRecords
    declared = [v for v in vars(spe.abi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    assert sorted(s.__name__ for s in declared) == sorted(structure_of(spe, n).__name__ for n in structs)
    assert len(declared) == len(structs) == 16
    for name, members in structs.items():
        fields = structure_of(spe, name)._fields_
        assert [f[0] for f in fields] == [m[0] for m in members], name
        for (field, ctype), (_, c_type, extent) in zip(fields, members):
            assert c_type in MEMBERS, f"no ctypes mapping for the member type {c_type!r} of {name}.{field}"
            want = MEMBERS[c_type] if extent is None else MEMBERS[c_type] * extent
            assert ctype is want, f"{name}.{field} is {c_type}{'[%d]' % extent if extent else ''} in the header"
    assert dict(spe.SensorIn._fields_)["mount_uniform"] is C.c_double * 7


def test_the_loaded_library_carries_the_table(spe):
    lib = spe.load_library()
    for name, (restype, argtypes) in spe.abi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert tuple(fn.argtypes) == tuple(argtypes), name
        assert fn.errcheck is None, name   # raw calls keep returning their codes


def test_a_pointer_of_another_element_type_is_refused(spe):
    import numpy as np
    lib = spe.load_library()
    wrong = np.zeros(4, dtype=np.int32).ctypes.data_as(P(C.c_int32))
    with pytest.raises(C.ArgumentError):
        lib.ukfb_predict_dt(None, wrong)


def test_a_32_bit_box_for_int64_is_refused(spe):
    lib = spe.load_library()
    with pytest.raises(C.ArgumentError):
        lib.ukfb_initialize(None, C.c_int(0), C.c_int(1), None, None)


def test_a_bare_python_int_reaches_int64_whole(spe):
    lib = spe.load_library()
    first, count = C.c_int64(-1), C.c_int64(-1)
    assert lib.ukfb_group_shard_range(1 << 40, 2, 1, C.byref(first), C.byref(count)) == 0
    assert (first.value, count.value) == spe.shard_range(1 << 40, 2, 1)
