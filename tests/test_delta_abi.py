"""Model deltas on the host side (dust_hip_model_delta, dust_hip_model_delta_apply): the entry points are declared, exported, bound,
documented and mirrored; the three records' layouts and the constants are the same in the C header, the ctypes binding, the numpy
dtypes and the witness; the query is a surface query field for field; the calls refuse null arguments without a device and leave the
outputs alone; the header says what is out of scope; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import delta_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_delta", "dust_hip_model_delta_apply")


def test_entry_points_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mirror = open(os.path.join(ROOT, "include", "dust_hip.hpp")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header)
        assert name in L.SYMBOLS and getattr(lib, name) is not None
        assert re.search(r"pub fn " + name + r"\(", doc)
        assert re.search(r"\b" + name + r"\(", mirror) and re.search(r"`" + name + r"`", readme) and re.search(r"`" + name + r"`", design)
    for record in ("DustHipDeltaQuery", "DustHipDeltaResult", "DustHipDeltaVoxel"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.delta) and callable(api.Model.delta_apply)
    assert header.index("Model meshes:") < header.index("Model deltas:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model deltas:"):])        # (the comment's line breaks and margin stars out of the way)
    for scope in ("an offset or orientation between the two models", "a device-side copy of a model", "run-length or otherwise packed deltas",
                  "4096^3 trees", "an asynchronous form", "a strict apply that changes nothing on a conflict"):   # what the header rules out
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "delta_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "delta_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipDeltaQuery", L.DeltaQuery, None, W.QUERY_DTYPE, 48), ("DustHipDeltaResult", L.DeltaResult, api.DELTA_RESULT_DTYPE, W.RESULT_DTYPE, 64),
               ("DustHipDeltaVoxel", L.DeltaVoxel, api.DELTA_VOXEL_DTYPE, W.VOXEL_DTYPE, 8))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == size and (dtype is None or dtype.itemsize == size)
        assert [f for f, _ in struct._fields_] == list(witness.names) and (dtype is None or list(dtype.names) == list(witness.names))
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            if dtype is not None:
                assert dtype.fields[field][1] == off and dtype.fields[field][0] == witness.fields[field][0], (name, field)
    for kind, bit in (("ADDED", 1), ("REMOVED", 2), ("REPAINTED", 4), ("ALL", 7)):
        assert c["DUST_HIP_DELTA_" + kind] == getattr(L, "DELTA_" + kind) == getattr(W, kind) == bit
    assert c["DUST_HIP_DELTA_NONE"] == L.DELTA_NONE == W.NONE == 255
    assert c["DUST_HIP_DELTA_BACKWARD"] == L.DELTA_BACKWARD == W.BACKWARD == 1
    assert c["DUST_HIP_DELTA_BINS"] == L.DELTA_BINS == W.BINS == 256
    assert c["DUST_HIP_MAX_DELTA_RECORDS"] == L.MAX_DELTA_RECORDS == W.MAX_RECORDS == 16777216


def test_the_query_is_a_surface_query_field_for_field(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipDeltaQuery"] == c["DustHipSurfaceQuery"] == C.sizeof(L.SurfaceQuery)
    ours, theirs = L.DeltaQuery._fields_, L.SurfaceQuery._fields_
    assert [n for n, _ in ours] == ["kinds" if n == "faces" else n for n, _ in theirs]
    for (mine, mine_type), (other, other_type) in zip(ours, theirs):
        assert mine_type is other_type or (C.sizeof(mine_type) == C.sizeof(other_type) and mine_type._type_ is other_type._type_), mine
        assert getattr(L.DeltaQuery, mine).offset == getattr(L.SurfaceQuery, other).offset == c["DustHipDeltaQuery." + mine] == c["DustHipSurfaceQuery." + other]


def test_calls_refuse_null_arguments_and_leave_the_outputs_alone():
    lib = L.load()
    q = L.DeltaQuery(struct_size=C.sizeof(L.DeltaQuery), kinds=L.DELTA_ALL, palette=-1)
    q.hi[:] = [255, 255, 255]
    result = np.full(64, 0x5A, np.uint8).view(api.DELTA_RESULT_DTYPE)
    voxels = np.full(4 * 8, 0x5A, np.uint8).view(api.DELTA_VOXEL_DTYPE)
    counts = np.full((2, 256), 0x5A5A5A5A, np.uint32)
    changed, conflicts = C.c_uint32(0x5A5A5A5A), C.c_uint32(0x5A5A5A5A)
    before = result.tobytes(), voxels.tobytes(), counts.tobytes()
    rp, vp, cp = (a.ctypes.data_as(C.c_void_p) for a in (result, voxels, counts))
    assert lib.dust_hip_model_delta(None, None, C.byref(q), rp, vp, 4, cp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_delta(None, None, None, None, None, 0, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_delta(None, None, None, rp, vp, 4, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_delta_apply(None, vp, 4, 0, C.byref(changed), C.byref(conflicts)) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_delta_apply(None, None, 0, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), voxels.tobytes(), counts.tobytes()) == before and changed.value == conflicts.value == 0x5A5A5A5A


def test_cpp_mirror_delta_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "delta_mirror.cpp"), "-o", str(tmp_path / "delta_mirror.o")])
