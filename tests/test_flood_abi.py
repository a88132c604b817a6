"""Model floods on the host side (dust_hip_model_flood / flood_at / flood_paths / flood_apply): the entry points are declared, exported,
bound, documented and mirrored; the two records' layouts and the constants are the same in the C header, the ctypes binding, the numpy
dtypes and the witness; every call refuses a null model without a device and leaves its outputs alone; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import flood_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_flood", "dust_hip_model_flood_at", "dust_hip_model_flood_paths", "dust_hip_model_flood_apply")


def test_entry_points_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mirror = open(os.path.join(ROOT, "include", "dust_hip.hpp")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS, name
        assert re.search(r"pub fn " + name + r"\(", doc), name
        assert getattr(lib, name) is not None, name
        assert re.search(r"\b" + name + r"\(", mirror) and re.search(r"`" + name + r"`", readme), name
    for struct in ("DustHipFloodQuery", "DustHipFloodResult"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct
    for method in ("flood", "flood_at", "flood_paths", "flood_apply"):
        assert callable(getattr(api.Model, method))
    for scope in ("ground-walking", "26-neighbour", "instances of a scene", "4096^3", "asynchronous"):      # what the header rules out
        assert scope in header, scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "flood_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "flood_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipFloodQuery"] == C.sizeof(L.FloodQuery) == W.QUERY_DTYPE.itemsize == 40
    assert c["DustHipFloodResult"] == C.sizeof(L.FloodResult) == api.FLOOD_RESULT_DTYPE.itemsize == W.RESULT_DTYPE.itemsize == 32
    assert [f for f, _ in L.FloodQuery._fields_] == list(W.QUERY_DTYPE.names)
    for field, _ in L.FloodQuery._fields_:
        off = c[f"DustHipFloodQuery.{field}"]
        assert getattr(L.FloodQuery, field).offset == off == W.QUERY_DTYPE.fields[field][1], field
        assert getattr(L.FloodQuery, field).size == W.QUERY_DTYPE.fields[field][0].itemsize, field
    assert [f for f, _ in L.FloodResult._fields_] == list(api.FLOOD_RESULT_DTYPE.names) == list(W.RESULT_DTYPE.names)
    for field, _ in L.FloodResult._fields_:
        off = c[f"DustHipFloodResult.{field}"]
        assert getattr(L.FloodResult, field).offset == off, field
        assert api.FLOOD_RESULT_DTYPE.fields[field][1] == off == W.RESULT_DTYPE.fields[field][1], field
        assert api.FLOOD_RESULT_DTYPE.fields[field][0] == W.RESULT_DTYPE.fields[field][0], field
        assert getattr(L.FloodResult, field).size == api.FLOOD_RESULT_DTYPE.fields[field][0].itemsize, field
    assert c["DUST_HIP_FLOOD_EMPTY"] == L.FLOOD_EMPTY == W.EMPTY == 0
    assert c["DUST_HIP_FLOOD_SOLID"] == L.FLOOD_SOLID == W.SOLID == 1
    assert c["DUST_HIP_FLOOD_MATERIAL"] == L.FLOOD_MATERIAL == W.MATERIAL == 2
    assert c["DUST_HIP_FLOOD_UNREACHED"] == L.FLOOD_UNREACHED == W.UNREACHED == 0xFFFF
    assert c["DUST_HIP_FLOOD_MAX_STEPS"] == L.FLOOD_MAX_STEPS == W.MAX_STEPS == 65534
    assert c["DUST_HIP_MAX_FLOOD_SEEDS"] == L.MAX_FLOOD_SEEDS == W.MAX_SEEDS == 65536


def test_calls_refuse_without_a_model():
    lib = L.load()
    q = L.FloodQuery(struct_size=C.sizeof(L.FloodQuery), medium=L.FLOOD_EMPTY, max_steps=10)
    q.hi[:] = [255, 255, 255]
    out = np.full(1, 0x5A, np.uint8).repeat(32).view(api.FLOOD_RESULT_DTYPE)
    before = out.tobytes()
    xyz = np.zeros((3, 3), np.uint32)
    xp = xyz.ctypes.data_as(C.c_void_p)
    assert lib.dust_hip_model_flood(None, C.byref(q), xp, 3, out.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_flood(None, C.byref(q), None, 0, None) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert out.tobytes() == before
    steps = np.full(3, 77, np.uint16)
    assert lib.dust_hip_model_flood_at(None, xp, steps.ctypes.data_as(C.c_void_p), 3) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_flood_at(None, None, None, 0) == L.ERR_INVALID_ARGUMENT
    assert steps.tolist() == [77] * 3
    keys = np.full((3, 2), 77, np.uint32)
    lengths = np.full(3, 77, np.uint32)
    assert lib.dust_hip_model_flood_paths(None, xp, 3, 2, keys.ctypes.data_as(C.c_void_p), lengths.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_flood_paths(None, None, 0, 0, None, lengths.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID_ARGUMENT
    assert (keys == 77).all() and (lengths == 77).all()
    changed = C.c_uint32(77)
    assert lib.dust_hip_model_flood_apply(None, 5, 3, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_flood_apply(None, 0, -1, None) == L.ERR_INVALID_ARGUMENT
    assert changed.value == 77
    assert b"null" in lib.dust_hip_last_error()


def test_cpp_mirror_floods_compile(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "flood_mirror.cpp"), "-o", str(tmp_path / "flood_mirror.o")])
