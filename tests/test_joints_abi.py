"""Model joints on the host side (dust_hip_model_joints): the entry point is declared, exported, bound, documented and mirrored; the two
records' layouts and the constants are the same in the C header, the ctypes binding, the numpy dtype and the witness, and the query has
a surface query's layout; the call refuses null arguments without a device and leaves the outputs alone; the witness refuses each
malformed query the header lists (tests/test_joint_rule.py holds device_joints, run natively, to the same table); the header states
the memory bound and what is out of scope; the C++ mirror compiles; joint_properties is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import joints_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_joints"


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
    for record in ("DustHipJointQuery", "DustHipJoint"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.joints) and callable(api.joint_properties)
    # the block stands after "Model bodies", before "Model resampling"
    assert header.index("Model bodies:") < header.index("Model joints:") < header.index("Model resampling:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model joints:"):header.index("Model resampling:")])   # (line breaks and margin stars out of the way)
    assert "2^24 slots" in block and "8 390 656 pairs" in block and "32 385 possible pairs" in block
    for scope in ("contacts with the tree's faces", "edge and corner contacts", "a palette filter", "breaking joints or solving anything on the device"):
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "joints_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "joints_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipJointQuery", L.JointQuery, None, W.QUERY_DTYPE, 48), ("DustHipJoint", L.Joint, api.JOINT_DTYPE, W.JOINT_DTYPE, 80))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == size and (dtype is None or dtype.itemsize == size)
        assert [f for f, _ in struct._fields_] == list(witness.names) and (dtype is None or list(dtype.names) == list(witness.names))
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            if dtype is not None:
                assert dtype.fields[field][1] == off and dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert [c[f"DustHipJoint.{f}"] for f in ("a", "b", "faces", "reserved0", "by_face", "lo2", "hi2", "reserved1", "sum2")] == [0, 4, 8, 12, 16, 40, 46, 52, 56]
    assert c["DustHipJointQuery"] == c["DustHipSurfaceQuery"]
    for mine, surface in zip(L.JointQuery._fields_, L.SurfaceQuery._fields_):    # a surface query's layout, `group` where `faces` stands
        assert c[f"DustHipJointQuery.{mine[0]}"] == c[f"DustHipSurfaceQuery.{surface[0]}"] and mine[1] is surface[1]
        assert mine[0] == surface[0] or (mine[0], surface[0]) == ("group", "faces")
    assert (c["DUST_HIP_JOINTS_MATERIALS"], c["DUST_HIP_JOINTS_CELLS"]) == (L.JOINTS_MATERIALS, L.JOINTS_CELLS) == (W.MATERIALS, W.CELLS) == (0, 1)
    assert c["DUST_HIP_JOINT_REST"] == L.JOINT_REST == W.REST == c["DUST_HIP_NO_CELL"] == W.NO_CELL == L.NO_CELL == 0xFFFF
    # by_face is in the order of the DUST_HIP_FACE_* bits
    faces = [c["DUST_HIP_FACE_" + n] for n in ("NEG_X", "POS_X", "NEG_Y", "POS_Y", "NEG_Z", "POS_Z")]
    assert faces == [1 << d for d in range(6)]


def test_call_refuses_null_arguments_and_leaves_the_outputs_alone():
    lib = L.load()
    q = L.JointQuery(struct_size=C.sizeof(L.JointQuery), group=L.JOINTS_MATERIALS, palette=-1)
    q.hi[:] = [255, 255, 255]
    n = C.c_uint32(0x5A5A5A5A)
    joints = np.full(4 * 80, 0x5A, np.uint8).view(api.JOINT_DTYPE)
    before = joints.tobytes()
    jp = joints.ctypes.data_as(C.c_void_p)
    assert lib.dust_hip_model_joints(None, C.byref(q), C.byref(n), jp, 4) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_joints(None, None, None, None, 0) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_joints(None, None, C.byref(n), jp, 4) == L.ERR_INVALID_ARGUMENT
    assert joints.tobytes() == before and n.value == 0x5A5A5A5A


def test_witness_refuses_what_the_header_lists():
    assert not W.refused() and not W.refused(W.CELLS)
    for bad in (dict(group=2), dict(group=0xFFFFFFFF), dict(flags=1), dict(palette=0), dict(palette=254), dict(palette=-2), dict(reserved=(1, 0)), dict(reserved=(0, 1))):
        assert W.refused(**bad), bad
    assert W.clip(((0, 0, 0), (300, 255, 1000))) == ([0, 0, 0], [255, 255, 255]) and W.clip(((256, 0, 0), (300, 255, 255))) is None
    assert W.clip(((5, 0, 0), (4, 255, 255))) is None


def test_cpp_mirror_joints_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "joints_mirror.cpp"), "-o", str(tmp_path / "joints_mirror.o")])


def test_joint_properties_are_exact():
    from fractions import Fraction
    records = np.zeros(3, api.JOINT_DTYPE)
    records[0]["faces"], records[0]["by_face"], records[0]["sum2"] = 3, (0, 2, 1, 0, 0, 0), (10, 21, 7)
    records[1]["faces"], records[1]["by_face"], records[1]["sum2"] = 1600, (0, 0, 1600, 0, 0, 0), (1600 * 46, 1600 * 32, 1600 * 46)
    area, anchor, normal = api.joint_properties(records, voxel_size=0.1)
    size = Fraction(0.1)
    assert area.tolist() == [float(3 * size * size), float(1600 * size * size), 0.0]
    assert anchor[0].tolist() == [float(Fraction(v, 6) * size) for v in (10, 21, 7)] and anchor[1].tolist() == [float(v * size) for v in (23, 16, 23)]
    assert normal[0].tolist() == [float(2 * size * size), float(-1 * size * size), 0.0] and normal[1].tolist() == [0.0, float(-1600 * size * size), 0.0]
    assert anchor[2].tolist() == normal[2].tolist() == [0.0] * 3
    area, anchor, normal = api.joint_properties(records[:1])
    assert (area[0], anchor[0].tolist(), normal[0].tolist()) == (3.0, [10 / 6, 3.5, 7 / 6], [2.0, -1.0, 0.0])
