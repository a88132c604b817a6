"""Scene ray queries on the host side (dust_hip_scene_trace_rays / _async): the two entry points are declared, exported, bound and
documented; the records' layout is the same in the C header, the ctypes binding and the numpy dtypes; the calls refuse bad arguments
without a device; the C++ mirror's Scene::trace_rays compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_scene_trace_rays", "dust_hip_scene_trace_rays_async")


def test_entry_points_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS, name
        assert re.search(r"pub fn " + name + r"\(", doc), name
        assert getattr(lib, name) is not None
    for struct in ("DustHipRay", "DustHipRayHit"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct
    assert "pipeline/mod.rs:64-98" in doc


def _c_layout(tmp_path):
    exe = str(tmp_path / "ray_query_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ray_query_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layout_matches_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipRay"] == C.sizeof(L.Ray) == api.RAY_DTYPE.itemsize == 32
    assert c["DustHipRayHit"] == C.sizeof(L.RayHit) == api.HIT_DTYPE.itemsize == 32
    for struct, ct, dt in (("DustHipRay", L.Ray, api.RAY_DTYPE), ("DustHipRayHit", L.RayHit, api.HIT_DTYPE)):
        for field, _ in ct._fields_:
            off = c[f"{struct}.{field}"]
            assert getattr(ct, field).offset == off, (struct, field)
            assert dt.fields[field][1] == off, (struct, field)
    assert c["DUST_HIP_NO_HIT"] == L.NO_HIT
    assert c["DUST_HIP_QUERY_ANY_HIT"] == L.QUERY_ANY_HIT


def test_calls_refuse_without_a_scene():
    lib = L.load()
    rays = api.ray_records(np.zeros((4, 3)), np.ones((4, 3)))
    hits = np.zeros(4, api.HIT_DTYPE)
    rp, hp = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn(None, rp, hp, 4, 0) == L.ERR_INVALID_ARGUMENT, name
        assert fn(None, None, None, 4, 0) == L.ERR_INVALID_ARGUMENT, name
        assert fn(None, None, None, 0, 0) == L.ERR_INVALID_ARGUMENT, name   # (n == 0 with a live scene is a no-op: the GPU tests)


def test_ray_records_broadcast_and_unbounded_tmax():
    r = api.ray_records([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [1, 0, 0]], tmin=0.5, tmax=[np.inf, 7.0])
    assert r["origin"].tolist() == [[1, 2, 3], [4, 5, 6]] and r["tmin"].tolist() == [0.5, 0.5]
    assert r["tmax"][0] == np.float32(api.FLT_MAX) and r["tmax"][1] == 7.0   # the ABI reads a non-finite tmax as a degenerate ray


def test_cpp_mirror_scene_trace_rays_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "ray_query_mirror.cpp"), "-o", str(tmp_path / "ray_query_mirror.o")])
