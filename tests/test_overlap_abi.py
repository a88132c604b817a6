"""Scene box queries on the host side (dust_hip_scene_overlap_boxes / _async): the two entry points are declared, exported, bound and
documented; the records' layout is the same in the C header, the ctypes binding and the numpy dtypes; the calls refuse bad arguments
without a device; the C++ mirror's Scene::overlap_boxes compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_scene_overlap_boxes", "dust_hip_scene_overlap_boxes_async")


def test_entry_points_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS, name
        assert re.search(r"pub fn " + name + r"\(", doc), name
        assert getattr(lib, name) is not None
    for struct in ("DustHipBoxQuery", "DustHipVoxelRef"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct


def _c_layout(tmp_path):
    exe = str(tmp_path / "overlap_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "overlap_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layout_matches_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipBoxQuery"] == C.sizeof(L.BoxQuery) == api.BOX_QUERY_DTYPE.itemsize == 32
    assert c["DustHipVoxelRef"] == C.sizeof(L.VoxelRef) == api.VOXEL_REF_DTYPE.itemsize == 16
    for struct, ct, dt in (("DustHipBoxQuery", L.BoxQuery, api.BOX_QUERY_DTYPE), ("DustHipVoxelRef", L.VoxelRef, api.VOXEL_REF_DTYPE)):
        assert [f for f, _ in ct._fields_] == list(dt.names), struct
        for field, _ in ct._fields_:
            off = c[f"{struct}.{field}"]
            assert getattr(ct, field).offset == off, (struct, field)
            assert dt.fields[field][1] == off, (struct, field)
    assert c["DUST_HIP_QUERY_ANY_HIT"] == L.QUERY_ANY_HIT == 1


def test_calls_refuse_without_a_scene():
    lib = L.load()
    boxes = api.box_queries(np.zeros((4, 3)), np.ones((4, 3)), 2)
    counts, recs = np.zeros(4, np.uint32), np.zeros(8, api.VOXEL_REF_DTYPE)
    bp, cp, rp = (a.ctypes.data_as(C.c_void_p) for a in (boxes, counts, recs))
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn(None, bp, 4, cp, rp, 8, 0) == L.ERR_INVALID_ARGUMENT, name
        assert fn(None, None, 4, None, None, 0, 0) == L.ERR_INVALID_ARGUMENT, name
        assert fn(None, None, 0, None, None, 0, 0) == L.ERR_INVALID_ARGUMENT, name   # (n == 0 with a live scene is a no-op: the GPU tests)
        assert fn(None, bp, 4, cp, rp, 8, 2) == L.ERR_INVALID_ARGUMENT, name


def test_box_queries_lay_the_slices_end_to_end():
    b = api.box_queries([[0, 0, 0], [1, 2, 3], [4, 5, 6]], [[1, 1, 1], [2, 3, 4], [5, 6, 7]], capacity=[3, 0, 5])
    assert b["first"].tolist() == [0, 3, 3] and b["capacity"].tolist() == [3, 0, 5]
    assert b["lo"].tolist()[1] == [1, 2, 3] and b["hi"].tolist()[2] == [5, 6, 7]
    assert api.box_queries(np.zeros((2, 3)), np.ones((2, 3)), 4)["first"].tolist() == [0, 4]


def test_cpp_mirror_scene_overlap_boxes_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "overlap_mirror.cpp"), "-o", str(tmp_path / "overlap_mirror.o")])
