"""Model meshes on the host side (dust_hip_model_mesh): the entry point is declared, exported, bound, documented and mirrored; the
three records' layouts and the constants are the same in the C header, the ctypes binding, the numpy dtypes and the witness, and the
query is a surface query field for field; the call refuses null arguments without a device and leaves the outputs alone; the header
says what the rule is not and what is out of scope; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import mesh_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_mesh"


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
    for record in ("DustHipMeshQuery", "DustHipMeshQuad", "DustHipMeshResult"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.mesh) and callable(api.mesh_corners)
    assert header.index("Model surfaces:") < header.index("Model meshes:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model meshes:"):])        # (the comment's line breaks and margin stars out of the way)
    assert "NOT the minimum-count greedy mesh" in block[:block.index("Out of scope:")]
    for scope in ("the minimum-count greedy mesh", "T-junction-free output", "seams between different materials as faces",
                  "vertex or index buffers on the device", "faces across the instances of a scene", "4096^3 trees", "an asynchronous form"):
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "mesh_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mesh_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipMeshQuery", L.MeshQuery, None, W.QUERY_DTYPE, 48), ("DustHipMeshQuad", L.MeshQuad, api.MESH_QUAD_DTYPE, W.QUAD_DTYPE, 8),
               ("DustHipMeshResult", L.MeshResult, api.MESH_RESULT_DTYPE, W.RESULT_DTYPE, 64))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == size and (dtype is None or dtype.itemsize == size)
        assert [f for f, _ in struct._fields_] == list(witness.names) and (dtype is None or list(dtype.names) == list(witness.names))
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            if dtype is not None:
                assert dtype.fields[field][1] == off and dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert c["DustHipMeshQuery"] == c["DustHipSurfaceQuery"]
    for field, _ in L.MeshQuery._fields_:                                        # field for field a surface query
        assert c[f"DustHipMeshQuery.{field}"] == c[f"DustHipSurfaceQuery.{field}"] == getattr(L.SurfaceQuery, field).offset
    assert c["DUST_HIP_MESH_WALLS"] == L.MESH_WALLS == W.WALLS == c["DUST_HIP_SURFACE_WALLS"] == 1
    assert c["DUST_HIP_MESH_ANY_PALETTE"] == L.MESH_ANY_PALETTE == W.ANY_PALETTE == 2
    assert c["DUST_HIP_FACES_ALL"] == L.FACES_ALL == W.FACES_ALL == 63
    # the device writes a quad as one 64-bit word: key | face << 32 | palette << 40 | du << 48 | dv << 56
    quad = np.array([(0x00ABCDEF, 5, 254, 7, 255)], api.MESH_QUAD_DTYPE)
    assert int(quad.view("<u8")[0]) == 0x00ABCDEF | (5 << 32) | (254 << 40) | (7 << 48) | (255 << 56)


def test_call_refuses_null_arguments_and_leaves_the_outputs_alone():
    lib = L.load()
    q = L.MeshQuery(struct_size=C.sizeof(L.MeshQuery), faces=L.FACES_ALL, palette=-1)
    q.hi[:] = [255, 255, 255]
    result = np.full(64, 0x5A, np.uint8).view(api.MESH_RESULT_DTYPE)
    quads = np.full(4 * 8, 0x5A, np.uint8).view(api.MESH_QUAD_DTYPE)
    before = result.tobytes(), quads.tobytes()
    rp, qp = (a.ctypes.data_as(C.c_void_p) for a in (result, quads))
    assert lib.dust_hip_model_mesh(None, C.byref(q), rp, qp, 4) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_mesh(None, None, None, None, 0) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_mesh(None, None, rp, qp, 4) == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), quads.tobytes()) == before


def test_cpp_mirror_mesh_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "mesh_mirror.cpp"), "-o", str(tmp_path / "mesh_mirror.o")])
