"""Shape edits on the host side (dust_hip_model_edit_shapes): the entry point is declared, exported, bound and documented; the
record's layout and the constants are the same in the C header, the ctypes binding and the numpy dtype; the call refuses a null
model without a device; the edit_shapes helper; the C++ mirror's VoxGeometry::edit_shapes compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import shape_edit_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_edit_shapes"


def test_entry_point_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = L.load()
    assert re.search(r"\b" + NAME + r"\s*\(", header)
    assert NAME in L.SYMBOLS
    assert re.search(r"pub fn " + NAME + r"\(", doc)
    assert getattr(lib, NAME) is not None
    assert re.search(r"#\[repr\(C\)\] pub struct DustHipEditShape \{", doc)
    assert NAME in open(os.path.join(ROOT, "include", "dust_hip.hpp")).read()
    assert NAME in open(os.path.join(ROOT, "README.md")).read()


def _c_layout(tmp_path):
    exe = str(tmp_path / "edit_shape_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "edit_shape_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layout_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipEditShape"] == C.sizeof(L.EditShape) == api.EDIT_SHAPE_DTYPE.itemsize == W.SHAPE_DTYPE.itemsize == 48
    assert [f for f, _ in L.EditShape._fields_] == list(api.EDIT_SHAPE_DTYPE.names) == list(W.SHAPE_DTYPE.names)
    for field, _ in L.EditShape._fields_:
        off = c[f"DustHipEditShape.{field}"]
        assert getattr(L.EditShape, field).offset == off, field
        assert api.EDIT_SHAPE_DTYPE.fields[field][1] == off, field
        assert W.SHAPE_DTYPE.fields[field][1] == off, field
        assert api.EDIT_SHAPE_DTYPE.fields[field][0] == W.SHAPE_DTYPE.fields[field][0], field
    assert c["DUST_HIP_SHAPE_BOX"] == L.SHAPE_BOX == W.BOX == 0
    assert c["DUST_HIP_SHAPE_SPHERE"] == L.SHAPE_SPHERE == W.SPHERE == 1
    assert c["DUST_HIP_SHAPE_CAPSULE"] == L.SHAPE_CAPSULE == W.CAPSULE == 2
    assert c["DUST_HIP_EDIT_CARVE"] == L.EDIT_CARVE == W.CARVE == 0
    assert c["DUST_HIP_EDIT_FILL"] == L.EDIT_FILL == W.FILL == 1
    assert c["DUST_HIP_EDIT_PAINT"] == L.EDIT_PAINT == W.PAINT == 2
    assert c["DUST_HIP_EDIT_PLACE"] == L.EDIT_PLACE == W.PLACE == 3
    assert c["DUST_HIP_MAX_EDIT_SHAPES"] == L.MAX_EDIT_SHAPES == W.MAX_SHAPES == 65536


def test_call_refuses_without_a_model():
    lib = L.load()
    shapes = api.edit_shapes(L.SHAPE_SPHERE, np.full((4, 3), 8.5), radius=2.0)
    changed = np.full(4, 77, np.uint32)
    sp, cp = (a.ctypes.data_as(C.c_void_p) for a in (shapes, changed))
    fn = getattr(lib, NAME)
    assert fn(None, sp, 4, cp) == L.ERR_INVALID_ARGUMENT
    assert fn(None, sp, 4, None) == L.ERR_INVALID_ARGUMENT
    assert fn(None, None, 4, None) == L.ERR_INVALID_ARGUMENT
    assert fn(None, None, 0, None) == L.ERR_INVALID_ARGUMENT   # (n == 0 with a live model is a no-op: the GPU tests)
    assert changed.tolist() == [77] * 4
    assert b"null" in lib.dust_hip_last_error()


def test_edit_shapes_helper():
    s = api.edit_shapes(L.SHAPE_CAPSULE, [[1, 2, 3], [4, 5, 6]], [[7, 8, 9], [10, 11, 12]], radius=[1.5, 2.5], op=L.EDIT_PLACE, palette=[3, 254])
    assert s.dtype == api.EDIT_SHAPE_DTYPE and len(s) == 2
    assert s["a"].tolist() == [[1, 2, 3], [4, 5, 6]] and s["b"].tolist() == [[7, 8, 9], [10, 11, 12]]
    assert s["kind"].tolist() == [2, 2] and s["radius"].tolist() == [1.5, 2.5] and s["op"].tolist() == [3, 3] and s["palette"].tolist() == [3, 254]
    assert not s["reserved"].any()
    one = api.edit_shapes(L.SHAPE_SPHERE, [100.5, 100.5, 100.5], radius=24.0)      # a crater: b is not needed, the op defaults to CARVE
    assert len(one) == 1 and one["op"][0] == L.EDIT_CARVE and one["b"].tolist() == one["a"].tolist() and one["radius"][0] == 24.0
    assert one.tobytes() == W.shapes(W.shape(W.SPHERE, (100.5, 100.5, 100.5), radius=24.0)).tobytes()
    assert len(api.edit_shapes(L.SHAPE_BOX, np.zeros((0, 3)), np.zeros((0, 3)))) == 0


def test_cpp_mirror_edit_shapes_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "edit_shape_mirror.cpp"), "-o", str(tmp_path / "edit_shape_mirror.o")])
