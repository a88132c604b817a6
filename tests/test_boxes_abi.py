"""Model boxes on the host side (dust_hip_model_boxes): the entry point is declared, exported, bound, documented and mirrored; the
three records' layouts and the constant are the same in the C header, the ctypes binding, the numpy dtypes and the witness, and the
query has a surface query's layout; the call refuses null arguments without a device and leaves the outputs alone; the header says
what the rule is not and what is out of scope; the host-only helpers turn records into bounds and shapes; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import boxes_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_boxes"


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
    for record in ("DustHipBoxesQuery", "DustHipBox", "DustHipBoxesResult"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.boxes) and callable(api.box_shapes) and callable(api.box_bounds)
    assert header.index("Model meshes:") < header.index("Model boxes:") < header.index("Model deltas:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model boxes:"):])         # (the comment's line breaks and margin stars out of the way)
    assert "NOT the minimum-count decomposition" in block[:block.index("Out of scope:")]
    for scope in ("the minimum-count decomposition", "boxes across materials other than by ANY_PALETTE", "convex pieces other than boxes", "4096^3 trees",
                  "an asynchronous form", "boxes across the instances of a scene"):
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "boxes_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "boxes_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipBoxesQuery", L.BoxesQuery, None, W.QUERY_DTYPE, 48), ("DustHipBox", L.Box, api.BOX_DTYPE, W.BOX_DTYPE, 8),
               ("DustHipBoxesResult", L.BoxesResult, api.BOXES_RESULT_DTYPE, W.RESULT_DTYPE, 64))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == size and (dtype is None or dtype.itemsize == size)
        assert [f for f, _ in struct._fields_] == list(witness.names) and (dtype is None or list(dtype.names) == list(witness.names))
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            if dtype is not None:
                assert dtype.fields[field][1] == off and dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert c["DustHipBoxesQuery"] == c["DustHipSurfaceQuery"]
    for mine, surface in zip(L.BoxesQuery._fields_, L.SurfaceQuery._fields_):     # a surface query's layout, `axis` where `faces` stands
        assert c[f"DustHipBoxesQuery.{mine[0]}"] == c[f"DustHipSurfaceQuery.{surface[0]}"] and mine[1] is surface[1]
        assert mine[0] == surface[0] or (mine[0], surface[0]) == ("axis", "faces")
    assert c["DUST_HIP_BOXES_ANY_PALETTE"] == L.BOXES_ANY_PALETTE == W.ANY_PALETTE == 1
    assert c["DUST_HIP_MAX_EDIT_SHAPES"] == L.MAX_EDIT_SHAPES
    # the device writes a box as one 64-bit word: key | palette << 32 | dx << 40 | dy << 48 | dz << 56
    box = np.array([(0x00ABCDEF, 254, 5, 7, 255)], api.BOX_DTYPE)
    assert int(box.view("<u8")[0]) == 0x00ABCDEF | (254 << 32) | (5 << 40) | (7 << 48) | (255 << 56)


def test_call_refuses_null_arguments_and_leaves_the_outputs_alone():
    lib = L.load()
    q = L.BoxesQuery(struct_size=C.sizeof(L.BoxesQuery), axis=0, palette=-1)
    q.hi[:] = [255, 255, 255]
    result = np.full(64, 0x5A, np.uint8).view(api.BOXES_RESULT_DTYPE)
    boxes = np.full(4 * 8, 0x5A, np.uint8).view(api.BOX_DTYPE)
    before = result.tobytes(), boxes.tobytes()
    rp, bp = (a.ctypes.data_as(C.c_void_p) for a in (result, boxes))
    assert lib.dust_hip_model_boxes(None, C.byref(q), rp, bp, 4) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_boxes(None, None, None, None, 0) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_boxes(None, None, rp, bp, 4) == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), boxes.tobytes()) == before


def test_box_bounds_and_box_shapes():
    """host only: a box's shape record holds the centres of exactly its voxels, and the witness's bounds are the binding's"""
    rng = np.random.default_rng(90)
    grid = np.where(rng.random((24, 20, 28)) < 0.9, rng.integers(1, 3, (24, 20, 28)), 0).astype(np.uint8)
    _, boxes = W.boxes(grid, axis=1)
    lo, hi = api.box_bounds(boxes)
    assert lo.dtype == hi.dtype == np.int32 and lo.shape == hi.shape == (len(boxes), 3)
    assert np.array_equal(lo, W.bounds(boxes)[0]) and np.array_equal(hi, W.bounds(boxes)[1])
    shapes = api.box_shapes(boxes)
    assert shapes.dtype == api.EDIT_SHAPE_DTYPE and len(shapes) == len(boxes)
    assert np.all(shapes["kind"] == L.SHAPE_BOX) and np.all(shapes["op"] == L.EDIT_PLACE) and shapes["palette"].tolist() == boxes["palette"].tolist()
    assert np.array_equal(shapes["a"], lo.astype(np.float32)) and np.array_equal(shapes["b"], (hi + 1).astype(np.float32))
    # the voxels whose centre lies inside [a, b] are the box's: painting the shapes gives the grid back
    centre = np.stack(np.meshgrid(*(np.arange(n) + 0.5 for n in grid.shape), indexing="ij"), axis=-1)
    again = np.zeros_like(grid)
    for shape in shapes:
        inside = np.all((centre >= shape["a"]) & (centre <= shape["b"]), axis=-1)
        assert not again[inside].any()
        again[inside] = shape["palette"] + 1
    assert np.array_equal(again, grid)
    painted = api.box_shapes(boxes[:4], op=L.EDIT_PAINT, palette=7)
    assert painted["palette"].tolist() == [7] * 4 and np.all(painted["op"] == L.EDIT_PAINT)
    assert len(api.box_shapes(boxes[:0])) == 0 and api.box_bounds(boxes[:0])[0].shape == (0, 3)
    full = np.array([(0, 3, 255, 255, 255)], api.BOX_DTYPE)                       # the extent 256 is stored as 255
    assert api.box_bounds(full)[1].tolist() == [[255, 255, 255]] and api.box_shapes(full)["b"].tolist() == [[256.0, 256.0, 256.0]]


def test_cpp_mirror_boxes_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "boxes_mirror.cpp"), "-o", str(tmp_path / "boxes_mirror.o")])
