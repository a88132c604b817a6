"""Scene box sweeps on the host side (dust_hip_scene_sweep_boxes / _async): the two entry points are declared, exported, bound and
documented; the records' layout is the same in the C header, the ctypes binding and the numpy dtypes; the calls refuse bad arguments
without a device; the box_sweeps helper; the C++ mirror's Scene::sweep_boxes compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_scene_sweep_boxes", "dust_hip_scene_sweep_boxes_async")


def test_entry_points_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS, name
        assert re.search(r"pub fn " + name + r"\(", doc), name
        assert getattr(lib, name) is not None
    for struct in ("DustHipBoxSweep", "DustHipSweepHit"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct


def _c_layout(tmp_path):
    exe = str(tmp_path / "sweep_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sweep_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layout_matches_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipBoxSweep"] == C.sizeof(L.BoxSweep) == api.BOX_SWEEP_DTYPE.itemsize == 48
    assert c["DustHipSweepHit"] == C.sizeof(L.SweepHit) == api.SWEEP_HIT_DTYPE.itemsize == 32
    for struct, ct, dt in (("DustHipBoxSweep", L.BoxSweep, api.BOX_SWEEP_DTYPE), ("DustHipSweepHit", L.SweepHit, api.SWEEP_HIT_DTYPE)):
        assert [f for f, _ in ct._fields_] == list(dt.names), struct
        for field, _ in ct._fields_:
            off = c[f"{struct}.{field}"]
            assert getattr(ct, field).offset == off, (struct, field)
            assert dt.fields[field][1] == off, (struct, field)
    # bytes 4..19 of a hit are a DustHipVoxelRef
    for field in ("instance", "block", "xyz", "palette", "voxel"):
        assert api.SWEEP_HIT_DTYPE.fields[field][1] == 4 + api.VOXEL_REF_DTYPE.fields[field][1], field
    assert c["DUST_HIP_QUERY_ANY_HIT"] == L.QUERY_ANY_HIT == 1
    assert c["DUST_HIP_SWEEP_IGNORE_START"] == L.SWEEP_IGNORE_START == 2
    assert c["DUST_HIP_NO_HIT"] == L.NO_HIT


def test_calls_refuse_without_a_scene():
    lib = L.load()
    sweeps = api.box_sweeps(np.zeros((4, 3)), np.ones((4, 3)), np.full((4, 3), 0.5))
    hits = np.zeros(4, api.SWEEP_HIT_DTYPE)
    sp, hp = (a.ctypes.data_as(C.c_void_p) for a in (sweeps, hits))
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn(None, sp, hp, 4, 0) == L.ERR_INVALID_ARGUMENT, name
        assert fn(None, None, None, 4, 0) == L.ERR_INVALID_ARGUMENT, name
        assert fn(None, None, None, 0, 0) == L.ERR_INVALID_ARGUMENT, name   # (n == 0 with a live scene is a no-op: the GPU tests)
        assert fn(None, sp, hp, 4, 3) == L.ERR_INVALID_ARGUMENT, name
        assert fn(None, sp, hp, 4, 4) == L.ERR_INVALID_ARGUMENT, name


def test_box_sweeps_helper():
    s = api.box_sweeps([[0, 0, 0], [1, 2, 3]], [[1, 1, 1], [2, 3, 4]], [[0, -1, 0], [-0.0, 5, 1e-45]])
    assert s.dtype == api.BOX_SWEEP_DTYPE and len(s) == 2
    assert s["lo"].tolist()[1] == [1, 2, 3] and s["hi"].tolist()[1] == [2, 3, 4]
    assert s["delta"][0].tolist() == [0, -1, 0] and np.signbit(s["delta"][1][0]) and s["delta"][1][2] > 0
    assert not s["reserved0"].any() and not s["reserved1"].any() and not s["reserved2"].any()
    assert len(api.box_sweeps(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))) == 0


def test_cpp_mirror_scene_sweep_boxes_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "sweep_mirror.cpp"), "-o", str(tmp_path / "sweep_mirror.o")])
