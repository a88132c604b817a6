"""Model voxelisation on the host side (dust_hip_model_edit_triangles, dust_hip_model_fill_mesh): the entry points are declared,
exported, bound, documented and mirrored; the three records' layouts and the constants are the same in the C header, the ctypes
binding, the numpy dtypes and the witness; the calls refuse without a device and leave the outputs alone; the header states the two
rules and what is out of scope; the host helpers make the records the header describes; the C++ mirror compiles. (What
device_triangle and device_fill_mesh make of every record and query, refusals included, is tests/test_triangle_rule.py's tables.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import triangle_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_edit_triangles", "dust_hip_model_fill_mesh")


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
    for record in ("DustHipTriangle", "DustHipFillMeshQuery", "DustHipFillMeshResult"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.edit_triangles) and callable(api.Model.fill_mesh) and callable(api.triangles) and callable(api.quads_to_triangles)
    assert header.index("Model settling:") < header.index("Model voxelisation:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model voxelisation:"):])  # (the comment's line breaks and stars out of the way, the products' too)
    block = block[:block.index("dust_hip_model_fill_mesh(DustHipModel")]
    for sentence in ("in units of 1 / DUST_HIP_TRIANGLE_UNIT = 1/256 voxel", "its centre (256 x + 128, 256 y + 128, 256 z + 128)", "every intermediate stays below 2^60",
                     "the normal is n = e1 x e2", "covers nothing: changed[i] = 0", "the closed triangle and the closed cube share a point",
                     "13-axis separating-axis test on integers", "e x u for the three edges e", "The inequalities are strict, so touching covers",
                     "apply in array order, as n successive calls would", "counted as edit_shapes counts it", "`changed` may be NULL",
                     "an odd number of triangles is CROSSED above its centre", "let s = sign(n.z)", "If s == 0 the triangle crosses nothing",
                     "E = d.x (py - a.y) - d.y (px - a.x)", "E == 0 and (d.y > 0, or d.y == 0 and d.x < 0)", "s dot(n, c - v0) < 0",
                     "A centre exactly on the plane is not crossed", "does not depend on the winding or on the order", "An OPEN mesh still gives a deterministic answer",
                     "clipped to the tree as dust_hip_model_columns clips it", "lo > hi on an axis is the empty region", "before the query is looked at",
                     "n == 0 is a no-op", "byte for byte what dust_hip_model_create builds", "DUST_ERR_NOT_READY"):
        assert sentence in block, sentence
    for scope in ("thin (6-separating) surfaces", "float vertices in the ABI", "count-only dry runs", "a choice of ray axis", "repairing open meshes", "4096^3 trees",
                  "asynchronous forms", "texture or colour sampling"):            # what the header rules out
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "triangle_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "triangle_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipTriangle", L.Triangle, api.TRIANGLE_DTYPE, W.TRIANGLE_DTYPE, 48),
               ("DustHipFillMeshQuery", L.FillMeshQuery, W.QUERY_DTYPE, W.QUERY_DTYPE, 48),
               ("DustHipFillMeshResult", L.FillMeshResult, api.FILL_MESH_RESULT_DTYPE, W.RESULT_DTYPE, 48))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == dtype.itemsize == size
        assert [f for f, _ in struct._fields_] == list(witness.names) == list(dtype.names)
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1] == dtype.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            assert dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert c["DustHipTriangle.op"] == 36 and c["DustHipFillMeshQuery.lo"] == 16 and c["DustHipFillMeshResult.lo"] == 16 and c["DustHipFillMeshResult.reserved"] == 40
    assert c["DUST_HIP_TRIANGLE_UNIT"] == L.TRIANGLE_UNIT == W.UNIT == 256 and c["DUST_HIP_TRIANGLE_MAX_COORD"] == L.TRIANGLE_MAX_COORD == W.MAX_COORD == 1 << 18
    assert c["DUST_HIP_MAX_EDIT_TRIANGLES"] == L.MAX_EDIT_TRIANGLES == W.MAX_EDIT_TRIANGLES == 65536
    assert c["DUST_HIP_MAX_MESH_TRIANGLES"] == L.MAX_MESH_TRIANGLES == W.MAX_MESH_TRIANGLES == 1 << 20
    ops = [c["DUST_HIP_EDIT_" + n] for n in ("CARVE", "FILL", "PAINT", "PLACE")]
    assert ops == [W.CARVE, W.FILL, W.PAINT, W.PLACE] == [L.EDIT_CARVE, L.EDIT_FILL, L.EDIT_PAINT, L.EDIT_PLACE]


def test_host_helpers_make_the_records_the_header_describes():
    t = api.triangles([[[0.5, 1.25, -3.0], [2.0, 0.001953125, 7.0], [1024.0, -1024.00390625, 0.998046875]]], L.EDIT_PAINT, 9)
    assert t.dtype == api.TRIANGLE_DTYPE and t["v"].tolist() == [[[128, 320, -768], [512, 0, 1792], [262144, -262145, 256]]]      # rint, ties to even; not clamped
    assert t["op"].tolist() == [2] and t["palette"].tolist() == [9] and t["reserved"].tolist() == [0]
    assert api.triangles(np.zeros((5, 3, 3)), [0, 1, 2, 3, 0], np.arange(5))["palette"].tolist() == [0, 1, 2, 3, 4]
    # a quad of Model.mesh -> two triangles on integer voxel corners whose normals are the face's, the pair covering the quad
    quads = np.zeros(6, api.MESH_QUAD_DTYPE)
    for face in range(6):
        quads[face] = ((10 << 16) | (20 << 8) | 30, face, 0, 3, 1)                 # du = 3, dv = 1: 4 x 2 faces
    tri = api.quads_to_triangles(quads)
    corners, normals = api.mesh_corners(quads)
    assert tri.dtype == api.TRIANGLE_DTYPE and len(tri) == 12 and (tri["v"] % 256 == 0).all() and tri["op"].tolist() == [L.EDIT_FILL] * 12
    for face in range(6):
        for half in (0, 1):
            v = W.verts(tri[2 * face + half])
            n = W.normal(v)
            assert [int(np.sign(c)) for c in n] == normals[face].tolist() and sum(abs(c) for c in n) == 8 * 256 * 256   # twice half of 4 x 2 faces
        assert {p for k in (0, 1) for p in W.verts(tri[2 * face + k])} == {tuple(int(c) * 256 for c in p) for p in corners[face]}


def test_calls_refuse_without_a_device_and_leave_the_outputs_alone():
    lib = L.load()
    tris = W.triangles([[(0, 0, 0), (256, 0, 0), (0, 256, 0)]] * 4, W.FILL, 1)
    tp = tris.ctypes.data_as(C.c_void_p)
    changed = np.full(4, 0x5A5A5A5A, np.uint32)
    result = np.full(48, 0x5A, np.uint8).view(api.FILL_MESH_RESULT_DTYPE)
    cp, rp = changed.ctypes.data_as(C.c_void_p), result.ctypes.data_as(C.c_void_p)

    def query(op=1, palette=0, flags=0, reserved=(0, 0), lo=(0, 0, 0), hi=(255, 255, 255), size=C.sizeof(L.FillMeshQuery)):
        q = L.FillMeshQuery(struct_size=size, op=op, palette=palette, flags=flags)
        q.lo[:], q.hi[:], q.reserved[:] = lo, hi, reserved
        return q
    # a null model, with every other argument right or wrong
    for n, pointer in ((4, tp), (0, None), (4, None), (L.MAX_EDIT_TRIANGLES + 1, tp)):
        assert lib.dust_hip_model_edit_triangles(None, pointer, n, cp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    queries = [query(), query(size=47), query(size=0), query(op=4), query(palette=255), query(palette=-1), query(flags=1), query(reserved=(7, 0)), query(reserved=(0, 7))]
    for q in queries:
        assert lib.dust_hip_model_fill_mesh(None, tp, 4, C.byref(q), rp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_fill_mesh(None, None, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert (changed == 0x5A5A5A5A).all() and result.tobytes() == bytes([0x5A]) * 48
    for q in queries[3:]:                                                         # ... and each of those is one the witness refuses too
        assert W.query_refused(q.op, q.palette, q.flags, tuple(q.reserved))
    assert not W.query_refused(W.CARVE, 255) and not W.query_refused(W.PLACE, 254)


def test_cpp_mirror_triangle_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "triangle_mirror.cpp"), "-o", str(tmp_path / "triangle_mirror.o")])
