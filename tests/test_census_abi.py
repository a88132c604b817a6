"""Model censuses on the host side (dust_hip_model_census): the entry point is declared, exported, bound, documented and mirrored; the
record's layout and the three constants are the same in the C header, the ctypes binding, the numpy dtype and the witness; the call
refuses null arguments without a device and leaves the outputs alone; the header says what is out of scope; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import census_witness as W
import shape_edit_witness as SW
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_census"


def test_entry_point_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mirror = open(os.path.join(ROOT, "include", "dust_hip.hpp")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    lib = L.load()
    assert re.search(r"\b" + NAME + r"\s*\(", header)
    assert NAME in L.SYMBOLS and getattr(lib, NAME) is not None
    assert re.search(r"pub fn " + NAME + r"\(", doc)
    assert re.search(r"\b" + NAME + r"\(", mirror) and re.search(r"`" + NAME + r"`", readme) and re.search(r"`" + NAME + r"`", design)
    assert re.search(r"#\[repr\(C\)\] pub struct DustHipCensus \{", doc)
    assert callable(api.Model.census)
    for scope in ("asynchronous form", "world-space shapes", "island key", "field's range", "second moments"):   # what the header rules out
        assert scope in header[header.index("Model censuses:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "census_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "census_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layout_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipCensus"] == C.sizeof(L.Census) == api.CENSUS_DTYPE.itemsize == W.RECORD_DTYPE.itemsize == 40
    assert [f for f, _ in L.Census._fields_] == list(api.CENSUS_DTYPE.names) == list(W.RECORD_DTYPE.names)
    for field, _ in L.Census._fields_:
        off = c[f"DustHipCensus.{field}"]
        assert getattr(L.Census, field).offset == off, field
        assert api.CENSUS_DTYPE.fields[field][1] == off == W.RECORD_DTYPE.fields[field][1], field
        assert api.CENSUS_DTYPE.fields[field][0] == W.RECORD_DTYPE.fields[field][0], field
        assert getattr(L.Census, field).size == api.CENSUS_DTYPE.fields[field][0].itemsize, field
    # laid out like DustHipIsland: the bounds and the sums stand where an island's do
    assert c["DustHipIsland"] == 40 and all(c[f"DustHipIsland.{f}"] == c[f"DustHipCensus.{f}"] for f in ("lo", "hi", "sum"))
    assert c["DUST_HIP_MAX_CENSUS_SHAPES"] == L.MAX_CENSUS_SHAPES == W.MAX_SHAPES == 65536
    assert c["DUST_HIP_MAX_CENSUS_TABLES"] == L.MAX_CENSUS_TABLES == W.MAX_TABLES == 4096
    assert c["DUST_HIP_CENSUS_BINS"] == L.CENSUS_BINS == W.BINS == 256
    # the shapes are edit_shapes' records
    assert c["DustHipEditShape"] == C.sizeof(L.EditShape) == api.EDIT_SHAPE_DTYPE.itemsize == SW.SHAPE_DTYPE.itemsize == 48


def test_call_refuses_null_arguments_and_leaves_the_outputs_alone():
    lib = L.load()
    shapes = np.zeros(2, api.EDIT_SHAPE_DTYPE)
    records = np.full(2 * 40, 0x5A, np.uint8).view(api.CENSUS_DTYPE)
    counts = np.full((2, 256), 0x5A5A5A5A, np.uint32)
    before = records.tobytes(), counts.tobytes()
    sp, rp, cp = (a.ctypes.data_as(C.c_void_p) for a in (shapes, records, counts))
    assert lib.dust_hip_model_census(None, sp, 2, rp, cp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_census(None, None, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_census(None, None, 2, rp, cp) == L.ERR_INVALID_ARGUMENT
    assert (records.tobytes(), counts.tobytes()) == before


def test_cpp_mirror_census_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "census_mirror.cpp"), "-o", str(tmp_path / "census_mirror.o")])
