"""Model distances on the host side (dust_hip_model_distance / distance_at / distance_apply): the entry points are declared, exported,
bound, documented and mirrored; the two records' layouts and the constants are the same in the C header, the ctypes binding, the numpy
dtypes and the witness; every call refuses a null model without a device and leaves its outputs alone; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import distance_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_distance", "dust_hip_model_distance_at", "dust_hip_model_distance_apply")


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
    for struct in ("DustHipDistanceQuery", "DustHipDistanceResult"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct
    for method in ("distance", "distance_at", "distance_apply"):
        assert callable(getattr(api.Model, method))
    for scope in ("flood restricted by clearance", "listing the voxels above a value", "Manhattan distance", "instances of a scene", "4096^3",
                  "asynchronous"):      # what the header rules out
        assert scope in header[header.index("Model distances:"):], scope
    for identity in ("EUCLIDEAN value is above r^2", "CHEBYSHEV value is above k", "how deep"):
        assert identity in header, identity


def _c_layout(tmp_path):
    exe = str(tmp_path / "distance_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "distance_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipDistanceQuery"] == C.sizeof(L.DistanceQuery) == W.QUERY_DTYPE.itemsize == 32
    assert c["DustHipDistanceResult"] == C.sizeof(L.DistanceResult) == api.DISTANCE_RESULT_DTYPE.itemsize == W.RESULT_DTYPE.itemsize == 32
    assert [f for f, _ in L.DistanceQuery._fields_] == list(W.QUERY_DTYPE.names)
    for field, _ in L.DistanceQuery._fields_:
        off = c[f"DustHipDistanceQuery.{field}"]
        assert getattr(L.DistanceQuery, field).offset == off == W.QUERY_DTYPE.fields[field][1], field
        assert getattr(L.DistanceQuery, field).size == W.QUERY_DTYPE.fields[field][0].itemsize, field
    assert [f for f, _ in L.DistanceResult._fields_] == list(api.DISTANCE_RESULT_DTYPE.names) == list(W.RESULT_DTYPE.names)
    for field, _ in L.DistanceResult._fields_:
        off = c[f"DustHipDistanceResult.{field}"]
        assert getattr(L.DistanceResult, field).offset == off, field
        assert api.DISTANCE_RESULT_DTYPE.fields[field][1] == off == W.RESULT_DTYPE.fields[field][1], field
        assert api.DISTANCE_RESULT_DTYPE.fields[field][0] == W.RESULT_DTYPE.fields[field][0], field
        assert getattr(L.DistanceResult, field).size == api.DISTANCE_RESULT_DTYPE.fields[field][0].itemsize, field
    assert c["DUST_HIP_DISTANCE_TO_SOLID"] == L.DISTANCE_TO_SOLID == W.TO_SOLID == 0
    assert c["DUST_HIP_DISTANCE_TO_EMPTY"] == L.DISTANCE_TO_EMPTY == W.TO_EMPTY == 1
    assert c["DUST_HIP_DISTANCE_TO_MATERIAL"] == L.DISTANCE_TO_MATERIAL == W.TO_MATERIAL == 2
    assert c["DUST_HIP_DISTANCE_EUCLIDEAN"] == L.DISTANCE_EUCLIDEAN == W.EUCLIDEAN == 0
    assert c["DUST_HIP_DISTANCE_CHEBYSHEV"] == L.DISTANCE_CHEBYSHEV == W.CHEBYSHEV == 1
    assert c["DUST_HIP_DISTANCE_WALLS"] == L.DISTANCE_WALLS == W.WALLS == 1
    assert c["DUST_HIP_DISTANCE_FAR"] == L.DISTANCE_FAR == W.FAR == 0xFFFF
    assert c["DUST_HIP_DISTANCE_MAX_RADIUS"] == L.DISTANCE_MAX_RADIUS == W.MAX_RADIUS == 255
    assert c["DUST_HIP_DISTANCE_NO_KEY"] == L.DISTANCE_NO_KEY == W.NO_KEY == 0xFFFFFFFF


def test_calls_refuse_without_a_model():
    lib = L.load()
    q = L.DistanceQuery(struct_size=C.sizeof(L.DistanceQuery), target=L.DISTANCE_TO_SOLID, metric=L.DISTANCE_EUCLIDEAN, max_radius=10)
    out = np.full(1, 0x5A, np.uint8).repeat(32).view(api.DISTANCE_RESULT_DTYPE)
    before = out.tobytes()
    assert lib.dust_hip_model_distance(None, C.byref(q), out.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_distance(None, None, None) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert out.tobytes() == before
    xyz = np.zeros((3, 3), np.uint32)
    values = np.full(3, 77, np.uint16)
    assert lib.dust_hip_model_distance_at(None, xyz.ctypes.data_as(C.c_void_p), values.ctypes.data_as(C.c_void_p), 3) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_distance_at(None, None, None, 0) == L.ERR_INVALID_ARGUMENT
    assert values.tolist() == [77] * 3
    changed = C.c_uint32(77)
    assert lib.dust_hip_model_distance_apply(None, 1, 4, 3, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_distance_apply(None, 0, 0, -1, None) == L.ERR_INVALID_ARGUMENT
    assert changed.value == 77
    assert b"null" in lib.dust_hip_last_error()


def test_cpp_mirror_distances_compile(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "distance_mirror.cpp"), "-o", str(tmp_path / "distance_mirror.o")])
