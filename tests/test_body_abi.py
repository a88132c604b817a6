"""Model bodies on the host side (dust_hip_model_bodies): the entry point is declared, exported, bound, documented and mirrored; the two
records' layouts and the constants are the same in the C header, the ctypes binding, the numpy dtype and the witness, and the query has
a surface query's layout; the call refuses null arguments without a device and leaves the outputs alone; the header states the overflow
bound and what is out of scope; the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import body_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_bodies"


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
    for record in ("DustHipBodyQuery", "DustHipBody"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.bodies) and callable(api.body_properties)
    # the block stands after "Model fracture", before "Model resampling"
    assert header.index("Model fracture:") < header.index("Model bodies:") < header.index("Model resampling:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model bodies:"):header.index("Model resampling:")])   # (line breaks and margin stars out of the way)
    assert "65535 255^2 2^24" in block and "below 2^63" in block       # (65535 * 255^2 * 2^24, its stars gone with the margin)
    for scope in ("world-space bodies over a scene's instances", "float densities", "groups named by a field's range", "an asynchronous form", "4096^3 trees"):
        assert scope in block[block.index("Out of scope:"):], scope
    # census's own sentence stays: it is still true of census
    assert "second moments (an inertia tensor)" in re.sub(r"[\s*]+", " ", header[header.index("Model censuses:"):header.index("Model surfaces:")])


def _c_layout(tmp_path):
    exe = str(tmp_path / "body_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "body_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipBodyQuery", L.BodyQuery, None, W.QUERY_DTYPE, 48), ("DustHipBody", L.Body, api.BODY_DTYPE, W.BODY_DTYPE, 96))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == size and (dtype is None or dtype.itemsize == size)
        assert [f for f, _ in struct._fields_] == list(witness.names) and (dtype is None or list(dtype.names) == list(witness.names))
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            if dtype is not None:
                assert dtype.fields[field][1] == off and dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert [c[f"DustHipBody.{f}"] for f in ("key", "voxels", "lo", "reserved0", "hi", "reserved1", "mass", "m1", "m2")] == [0, 4, 8, 11, 12, 15, 16, 24, 48]
    assert c["DustHipBodyQuery"] == c["DustHipSurfaceQuery"]
    for mine, surface in zip(L.BodyQuery._fields_, L.SurfaceQuery._fields_):     # a surface query's layout, `group` where `faces` stands
        assert c[f"DustHipBodyQuery.{mine[0]}"] == c[f"DustHipSurfaceQuery.{surface[0]}"] and mine[1] is surface[1]
        assert mine[0] == surface[0] or (mine[0], surface[0]) == ("group", "faces")
    for field in ("key", "voxels", "lo", "hi"):                                   # an island's header
        assert c[f"DustHipBody.{field}"] == c[f"DustHipIsland.{field}"]
    groups = (c["DUST_HIP_BODIES_ALL"], c["DUST_HIP_BODIES_MATERIALS"], c["DUST_HIP_BODIES_ISLANDS"], c["DUST_HIP_BODIES_CELLS"])
    assert groups == (L.BODIES_ALL, L.BODIES_MATERIALS, L.BODIES_ISLANDS, L.BODIES_CELLS) == (W.ALL, W.MATERIALS, W.ISLANDS, W.CELLS) == (0, 1, 2, 3)
    assert c["DUST_HIP_BODY_WEIGHTS"] == L.BODY_WEIGHTS == W.WEIGHTS == 255
    assert c["DUST_HIP_NO_CELL"] == W.NO_CELL == L.NO_CELL and c["DUST_HIP_NO_ISLAND"] == W.NO_ISLAND


def test_call_refuses_null_arguments_and_leaves_the_outputs_alone():
    lib = L.load()
    q = L.BodyQuery(struct_size=C.sizeof(L.BodyQuery), group=L.BODIES_ALL, palette=-1)
    q.hi[:] = [255, 255, 255]
    n = C.c_uint32(0x5A5A5A5A)
    bodies = np.full(4 * 96, 0x5A, np.uint8).view(api.BODY_DTYPE)
    weights = np.ones(255, np.uint16)
    before = bodies.tobytes()
    bp, wp = (a.ctypes.data_as(C.c_void_p) for a in (bodies, weights))
    assert lib.dust_hip_model_bodies(None, C.byref(q), wp, C.byref(n), bp, 4) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_bodies(None, None, None, None, None, 0) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_bodies(None, None, wp, C.byref(n), bp, 4) == L.ERR_INVALID_ARGUMENT
    assert bodies.tobytes() == before and n.value == 0x5A5A5A5A


def test_binding_checks_the_weight_table_before_the_call():
    model = api.Model.__new__(api.Model)                                          # (no device: the check comes first)
    for bad in (np.ones(254), np.ones(256), np.full(255, 65536), np.full(255, -1)):
        try:
            model.bodies(weights=bad)
        except ValueError:
            continue
        raise AssertionError("a weight table the call cannot take was accepted")


def test_cpp_mirror_bodies_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "body_mirror.cpp"), "-o", str(tmp_path / "body_mirror.o")])
