"""Model reductions on the host side (dust_hip_model_reduce): the entry point is declared, exported, bound, documented and mirrored;
the two records' layouts and the constant are the same in the C header, the ctypes binding, the numpy dtypes and the witness; the call
refuses null arguments without a device and leaves `out` and the result alone; the header says what is out of scope; the C++ mirror
compiles; api.lod_transform writes the matrix the header describes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import reduce_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_reduce"


def test_entry_point_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mirror = open(os.path.join(ROOT, "include", "dust_hip.hpp")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    lib = L.load()
    assert re.search(r"\b" + NAME + r"\s*\(", header)
    assert NAME in L.SYMBOLS and getattr(lib, NAME) is not None
    assert re.search(r"pub fn " + NAME + r"\(", doc)
    assert re.search(r"\b" + NAME + r"\(", mirror) and re.search(r"`" + NAME + r"`", readme)
    for struct in ("DustHipReduce", "DustHipReduceResult"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct
    assert callable(api.Model.reduce) and callable(api.lod_transform)
    for scope in ("sub-box of the source", "asynchronous form", "4096^3", "level selection is the host's"):   # what the header rules out
        assert scope in header[header.index("Model reductions:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "reduce_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "reduce_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constant_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipReduce"] == C.sizeof(L.Reduce) == W.QUERY_DTYPE.itemsize == 16
    assert c["DustHipReduceResult"] == C.sizeof(L.ReduceResult) == api.REDUCE_RESULT_DTYPE.itemsize == W.RESULT_DTYPE.itemsize == 16
    assert [f for f, _ in L.Reduce._fields_] == list(W.QUERY_DTYPE.names)
    for field, _ in L.Reduce._fields_:
        off = c[f"DustHipReduce.{field}"]
        assert getattr(L.Reduce, field).offset == off == W.QUERY_DTYPE.fields[field][1], field
        assert getattr(L.Reduce, field).size == W.QUERY_DTYPE.fields[field][0].itemsize, field
    assert [f for f, _ in L.ReduceResult._fields_] == list(api.REDUCE_RESULT_DTYPE.names) == list(W.RESULT_DTYPE.names)
    for field, _ in L.ReduceResult._fields_:
        off = c[f"DustHipReduceResult.{field}"]
        assert getattr(L.ReduceResult, field).offset == off, field
        assert api.REDUCE_RESULT_DTYPE.fields[field][1] == off == W.RESULT_DTYPE.fields[field][1], field
        assert api.REDUCE_RESULT_DTYPE.fields[field][0] == W.RESULT_DTYPE.fields[field][0], field
        assert getattr(L.ReduceResult, field).size == api.REDUCE_RESULT_DTYPE.fields[field][0].itemsize, field
    assert c["DUST_HIP_REDUCE_MAX_LEVELS"] == L.REDUCE_MAX_LEVELS == W.MAX_LEVELS == 8


def test_call_refuses_null_arguments_and_leaves_the_outputs_alone():
    lib = L.load()
    q = L.Reduce(struct_size=C.sizeof(L.Reduce), levels=1, min_solid=1, flags=0)
    out = C.c_void_p(0x5A5A5A5A)
    result = np.full(1, 0x5A, np.uint8).repeat(16).view(api.REDUCE_RESULT_DTYPE)
    before = result.tobytes()
    rp = result.ctypes.data_as(C.c_void_p)
    assert lib.dust_hip_model_reduce(None, C.byref(q), C.byref(out), rp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_reduce(None, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_reduce(None, None, C.byref(out), rp) == L.ERR_INVALID_ARGUMENT
    assert out.value == 0x5A5A5A5A and result.tobytes() == before


def test_cpp_mirror_reductions_compile(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "reduce_mirror.cpp"), "-o", str(tmp_path / "reduce_mirror.o")])


def test_lod_transform_scales_the_columns_and_keeps_the_translation():
    m = [[0.0, 0.0, 1.5, 40.0], [0.0, 0.5, 0.0, -60.0], [-1.0, 0.0, 0.25, 90.0]]
    want = [[0.0, 0.0, 12.0, 40.0], [0.0, 4.0, 0.0, -60.0], [-8.0, 0.0, 2.0, 90.0]]
    got = api.lod_transform(m, 3)
    assert got.dtype == np.float32 and got.shape == (3, 4) and got.tolist() == want
    assert api.lod_transform(np.float32(m).reshape(12), 3).tolist() == want        # the flat form add_instance takes
    assert api.lod_transform(m, 8)[2].tolist() == [-256.0, 0.0, 64.0, 90.0]
