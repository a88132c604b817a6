"""Model islands on the host side (dust_hip_model_find_islands / island_of / detach_islands): the entry points are declared, exported,
bound and documented; the two records' layouts and the constants are the same in the C header, the ctypes binding, the numpy dtype
and the witness; every call refuses a null model without a device and leaves its outputs alone; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import island_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_find_islands", "dust_hip_model_island_of", "dust_hip_model_detach_islands")


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
        assert name in mirror and name in readme, name
    for struct in ("DustHipIslandQuery", "DustHipIsland"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct
    for method in ("find_islands", "island_of", "detach_islands"):
        assert callable(getattr(api.Model, method))


def _c_layout(tmp_path):
    exe = str(tmp_path / "island_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "island_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipIslandQuery"] == C.sizeof(L.IslandQuery) == W.QUERY_DTYPE.itemsize == 32
    assert c["DustHipIsland"] == C.sizeof(L.Island) == api.ISLAND_DTYPE.itemsize == W.ISLAND_DTYPE.itemsize == 40
    assert [f for f, _ in L.IslandQuery._fields_] == list(W.QUERY_DTYPE.names)
    for field, _ in L.IslandQuery._fields_:
        off = c[f"DustHipIslandQuery.{field}"]
        assert getattr(L.IslandQuery, field).offset == off == W.QUERY_DTYPE.fields[field][1], field
    assert [f for f, _ in L.Island._fields_] == list(api.ISLAND_DTYPE.names) == list(W.ISLAND_DTYPE.names)
    for field, _ in L.Island._fields_:
        off = c[f"DustHipIsland.{field}"]
        assert getattr(L.Island, field).offset == off, field
        assert api.ISLAND_DTYPE.fields[field][1] == off == W.ISLAND_DTYPE.fields[field][1], field
        assert api.ISLAND_DTYPE.fields[field][0] == W.ISLAND_DTYPE.fields[field][0], field
        assert getattr(L.Island, field).size == api.ISLAND_DTYPE.fields[field][0].itemsize, field
    assert c["DUST_HIP_ISLANDS_FACES"] == L.ISLANDS_FACES == W.FACES == 0
    assert c["DUST_HIP_ISLANDS_CORNERS"] == L.ISLANDS_CORNERS == W.CORNERS == 1
    assert c["DUST_HIP_ISLAND_ANCHORED"] == L.ISLAND_ANCHORED == W.ANCHORED == 1
    assert c["DUST_HIP_NO_ISLAND"] == L.NO_ISLAND == W.NO_ISLAND == 0xFFFFFFFF
    assert c["DUST_HIP_DETACH_KEEP_SOURCE"] == L.DETACH_KEEP_SOURCE == W.KEEP_SOURCE == 1


def test_calls_refuse_without_a_model():
    lib = L.load()
    q = L.IslandQuery(struct_size=C.sizeof(L.IslandQuery), connectivity=L.ISLANDS_FACES)
    n = C.c_uint32(77)
    records = np.full(4, 0x5A, np.uint8).repeat(40).view(api.ISLAND_DTYPE)
    before = records.tobytes()
    rp = records.ctypes.data_as(C.c_void_p)
    assert lib.dust_hip_model_find_islands(None, C.byref(q), C.byref(n), rp, 4) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_find_islands(None, C.byref(q), C.byref(n), None, 0) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert n.value == 77 and records.tobytes() == before
    xyz = np.zeros((3, 3), np.uint32)
    keys = np.full(3, 77, np.uint32)
    assert lib.dust_hip_model_island_of(None, xyz.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), 3) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_island_of(None, None, None, 0) == L.ERR_INVALID_ARGUMENT
    assert keys.tolist() == [77] * 3
    out = C.c_void_p(0x1234)
    assert lib.dust_hip_model_detach_islands(None, keys.ctypes.data_as(C.c_void_p), 3, 0, C.byref(out)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_detach_islands(None, None, 0, 0, C.byref(out)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_detach_islands(None, None, 0, L.DETACH_KEEP_SOURCE, None) == L.ERR_INVALID_ARGUMENT
    assert out.value == 0x1234
    assert b"null" in lib.dust_hip_last_error()


def test_cpp_mirror_islands_compile(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "island_mirror.cpp"), "-o", str(tmp_path / "island_mirror.o")])
