"""Model columns on the host side (dust_hip_model_columns, dust_hip_model_columns_apply): the entry points are declared, exported,
bound, documented and mirrored; the three records' layouts and the constants are the same in the C header, the ctypes binding, the
numpy dtypes and the witness; the query is a surface query field for field, with the layer in its first reserved word; the calls
refuse without a device and leave the outputs alone; the header states the contract and what is out of scope; the C++ mirror
compiles. (What device_columns makes of every query, refusals included, is tests/test_column_rule.py's validation table.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import column_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_columns", "dust_hip_model_columns_apply")


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
    for record in ("DustHipColumnsQuery", "DustHipColumnsResult", "DustHipColumnCell"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.columns) and callable(api.Model.columns_apply)
    assert header.index("Model deltas:") < header.index("Model columns:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model columns:"):])       # (the comment's line breaks and margin stars out of the way)
    block = block[:block.index("dust_hip_model_columns_apply(DustHipModel")]
    for sentence in ("query.face names exactly one", "voxels outside the region do not exist for this call", "is see-through",
                     "at most 128", "row-major [v][u] with u fastest", "valid for a miss too", "among equals the lowest key",
                     "decided on the model as it stood when the call began", "whatever they hold", "snow only under open sky"):
        assert sentence in block, sentence
    for scope in ("columns across the instances of a scene in world space", "walls", "arbitrary directions", "4096^3 trees", "an asynchronous form",
                  "more than one layer per call"):                                 # what the header rules out
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "column_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "column_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipColumnsQuery", L.ColumnsQuery, None, W.QUERY_DTYPE, 48), ("DustHipColumnsResult", L.ColumnsResult, api.COLUMNS_RESULT_DTYPE, W.RESULT_DTYPE, 64),
               ("DustHipColumnCell", L.ColumnCell, api.COLUMN_CELL_DTYPE, W.CELL_DTYPE, 4))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == size and (dtype is None or dtype.itemsize == size)
        assert [f for f, _ in struct._fields_] == list(witness.names) and (dtype is None or list(dtype.names) == list(witness.names))
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            if dtype is not None:
                assert dtype.fields[field][1] == off and dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert c["DUST_HIP_COLUMNS_RUN"] == L.COLUMNS_RUN == W.RUN == 0 and c["DUST_HIP_COLUMNS_GAP"] == L.COLUMNS_GAP == W.GAP == 1
    assert c["DUST_HIP_COLUMNS_BINS"] == L.COLUMNS_BINS == W.BINS == 256
    assert c["DUST_HIP_COLUMNS_NO_KEY"] == L.COLUMNS_NO_KEY == W.NO_KEY == 0xFFFFFFFF
    for d, side in enumerate(("NEG_X", "POS_X", "NEG_Y", "POS_Y", "NEG_Z", "POS_Z")):
        assert c["DUST_HIP_FACE_" + side] == getattr(L, "FACE_" + side) == getattr(W, side) == W.FACES[d] == 1 << d


def test_the_query_is_a_surface_query_with_the_layer_in_its_first_reserved_word(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipColumnsQuery"] == c["DustHipSurfaceQuery"] == C.sizeof(L.SurfaceQuery)
    for mine, other in (("struct_size", "struct_size"), ("face", "faces"), ("flags", "flags"), ("palette", "palette"), ("lo", "lo"), ("hi", "hi"),
                        ("layer", "reserved")):
        assert getattr(L.ColumnsQuery, mine).offset == getattr(L.SurfaceQuery, other).offset == c["DustHipColumnsQuery." + mine] == c["DustHipSurfaceQuery." + other]
    assert c["DustHipColumnsQuery.reserved"] == c["DustHipSurfaceQuery.reserved"] + 4 == 44
    assert dict(L.ColumnsQuery._fields_)["palette"] is C.c_int32


def test_map_shape_follows_the_mesh_axes():
    region = ((3, 10, 20), (7, 19, 49))                                           # extents 5, 10, 30
    assert [api.Model.columns_shape(face, region) for face in W.FACES] == [(10, 30), (10, 30), (5, 30), (5, 30), (5, 10), (5, 10)]
    assert api.Model.columns_shape(L.FACE_POS_Y) == (256, 256) and api.Model.columns_shape(L.FACE_POS_Y, ((0, 0, 250), (9, 9, 300))) == (10, 6)
    assert api.Model.columns_shape(L.FACE_NEG_Z, ((5, 0, 0), (4, 9, 9))) == (0, 0)
    grid = np.zeros((8, 20, 50), np.uint8)
    for face in W.FACES:
        assert W.columns(grid, face, region=region)[1].shape == api.Model.columns_shape(face, region)


def test_calls_refuse_without_a_device_and_leave_the_outputs_alone():
    lib = L.load()

    def query(face=L.FACE_POS_Y, flags=0, palette=-1, layer=0, reserved=0, size=C.sizeof(L.ColumnsQuery)):
        q = L.ColumnsQuery(struct_size=size, face=face, flags=flags, palette=palette, layer=layer, reserved=reserved)
        q.hi[:] = [255, 255, 255]
        return q
    result = np.full(64, 0x5A, np.uint8).view(api.COLUMNS_RESULT_DTYPE)
    cells = np.full(16 * 4, 0x5A, np.uint8).view(api.COLUMN_CELL_DTYPE)
    counts = np.full(256, 0x5A5A5A5A, np.uint32)
    changed = C.c_uint32(0x5A5A5A5A)
    before = result.tobytes(), cells.tobytes(), counts.tobytes()
    rp, vp, cp = (a.ctypes.data_as(C.c_void_p) for a in (result, cells, counts))
    # every refusal of the header, through the entry points: a null model, then the query's faults one at a time
    queries = [query(), query(size=47), query(size=0), query(face=0), query(face=3), query(face=64), query(face=63), query(flags=1), query(reserved=1),
               query(palette=-2), query(palette=255), query(layer=256)]
    for q in queries:
        assert lib.dust_hip_model_columns(None, C.byref(q), rp, vp, 16, cp) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_columns_apply(None, C.byref(q), L.COLUMNS_RUN, 1, 3, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_columns(None, None, None, None, 0, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_columns_apply(None, None, 2, 0, 255, None) == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), cells.tobytes(), counts.tobytes()) == before and changed.value == 0x5A5A5A5A
    for q in queries[3:]:                                                         # ... and each of those is one the witness refuses too
        assert W.refused(q.face, q.flags, q.palette, q.layer, q.reserved)
    assert not W.refused(queries[0].face, 0, -1, 0, 0)


def test_cpp_mirror_column_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "column_mirror.cpp"), "-o", str(tmp_path / "column_mirror.o")])
