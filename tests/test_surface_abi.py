"""Model surfaces on the host side (dust_hip_model_surface, dust_hip_model_surface_apply): the entry points are declared, exported,
bound, documented and mirrored; the three records' layouts and the constants are the same in the C header, the ctypes binding, the
numpy dtypes and the witness; the calls refuse null arguments without a device and leave the outputs alone; the header says what is
out of scope; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import surface_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_surface", "dust_hip_model_surface_apply")


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
    for record in ("DustHipSurfaceQuery", "DustHipSurfaceResult", "DustHipSurfaceVoxel"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.surface) and callable(api.Model.surface_apply)
    block = re.sub(r"[\s*]+", " ", header[header.index("Model surfaces:"):])      # (the comment's line breaks and margin stars out of the way)
    for scope in ("merged quads (greedy meshing)", "seams between different materials as faces", "faces across the instances of a scene in world space",
                  "4096^3 trees", "an asynchronous form"):   # what the header rules out
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "surface_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "surface_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipSurfaceQuery", L.SurfaceQuery, None, W.QUERY_DTYPE, 48), ("DustHipSurfaceResult", L.SurfaceResult, api.SURFACE_RESULT_DTYPE, W.RESULT_DTYPE, 64),
               ("DustHipSurfaceVoxel", L.SurfaceVoxel, api.SURFACE_VOXEL_DTYPE, W.VOXEL_DTYPE, 8))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == size and (dtype is None or dtype.itemsize == size)
        assert [f for f, _ in struct._fields_] == list(witness.names) and (dtype is None or list(dtype.names) == list(witness.names))
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            if dtype is not None:
                assert dtype.fields[field][1] == off and dtype.fields[field][0] == witness.fields[field][0], (name, field)
    faces = ("NEG_X", "POS_X", "NEG_Y", "POS_Y", "NEG_Z", "POS_Z")
    for d, face in enumerate(faces):
        assert c["DUST_HIP_FACE_" + face] == getattr(L, "FACE_" + face) == getattr(W, face) == 1 << d
    assert c["DUST_HIP_FACES_ALL"] == L.FACES_ALL == W.FACES_ALL == 63
    assert c["DUST_HIP_SURFACE_WALLS"] == L.SURFACE_WALLS == W.WALLS == 1
    assert c["DUST_HIP_SURFACE_BINS"] == L.SURFACE_BINS == W.BINS == 256


def test_calls_refuse_null_arguments_and_leave_the_outputs_alone():
    lib = L.load()
    q = L.SurfaceQuery(struct_size=C.sizeof(L.SurfaceQuery), faces=L.FACES_ALL, palette=-1)
    q.hi[:] = [255, 255, 255]
    result = np.full(64, 0x5A, np.uint8).view(api.SURFACE_RESULT_DTYPE)
    voxels = np.full(4 * 8, 0x5A, np.uint8).view(api.SURFACE_VOXEL_DTYPE)
    counts = np.full((6, 256), 0x5A5A5A5A, np.uint32)
    changed = C.c_uint32(0x5A5A5A5A)
    before = result.tobytes(), voxels.tobytes(), counts.tobytes()
    rp, vp, cp = (a.ctypes.data_as(C.c_void_p) for a in (result, voxels, counts))
    assert lib.dust_hip_model_surface(None, C.byref(q), rp, vp, 4, cp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_surface(None, None, None, None, 0, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_surface(None, None, rp, vp, 4, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_surface_apply(None, C.byref(q), 3, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_surface_apply(None, None, -1, None) == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), voxels.tobytes(), counts.tobytes()) == before and changed.value == 0x5A5A5A5A


def test_cpp_mirror_surface_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "surface_mirror.cpp"), "-o", str(tmp_path / "surface_mirror.o")])
