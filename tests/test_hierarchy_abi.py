"""dust_hip_model_read_hierarchy on the host side: declared, exported, bound and documented; its three records laid out the same in the
C header, the ctypes binding, the numpy dtypes and the witness; null arguments refused without a device, outputs left alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import hierarchy_witness as HW
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_read_hierarchy"


def test_entry_point_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\b" + NAME + r"\s*\(", header) and NAME in L.SYMBOLS and re.search(r"pub fn " + NAME + r"\(", doc)
    assert getattr(L.load(), NAME) is not None and callable(api.Model.read_hierarchy)
    for struct in ("DustHipHierarchyInfo", "DustHipMidNode", "DustHipL2Cell"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct
    assert "tests/test_gpu_hierarchy.py" in header
    assert "tests/test_gpu_hierarchy.py" in open(os.path.join(ROOT, "dust_amd", "csrc", "edit.hip")).read()


def test_record_layouts_and_constants_match_the_header(tmp_path):
    exe = str(tmp_path / "hierarchy_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "hierarchy_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert c["DustHipHierarchyInfo"] == C.sizeof(L.HierarchyInfo) == 48
    for field, _ in L.HierarchyInfo._fields_:
        assert getattr(L.HierarchyInfo, field).offset == c[f"DustHipHierarchyInfo.{field}"], field
    assert len(L.HierarchyInfo._fields_) == 7
    for name, a, b in (("DustHipMidNode", api.MID_NODE_DTYPE, HW.MID_DTYPE), ("DustHipL2Cell", api.L2_CELL_DTYPE, HW.L2_CELL_DTYPE)):
        assert c[name] == a.itemsize == b.itemsize == 16 and a.names == b.names
        for field in a.names:
            assert c[f"{name}.{field}"] == a.fields[field][1] == b.fields[field][1] and a.fields[field][0] == b.fields[field][0], (name, field)
        assert sum(1 for k in c if k.startswith(name + ".")) == len(a.names)
    assert c["DUST_HIP_N16_BYTES"] == L.N16_BYTES == HW.N16_BYTES == 656
    assert c["DUST_HIP_N16_ROOT_BYTES"] == L.N16_ROOT_BYTES == HW.N16_ROOT_BYTES == 640


def test_call_refuses_without_a_model():
    lib = L.load()
    info = L.HierarchyInfo(struct_size=C.sizeof(L.HierarchyInfo), n_mid=77, n_l2=78)
    root = np.full(L.N16_BYTES, 0x5A, np.uint8)
    assert lib.dust_hip_model_read_hierarchy(None, C.byref(info), None, 0, None, 0, root.ctypes.data_as(C.c_void_p), None, None, 0, None, 0) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_read_hierarchy(None, None, None, 0, None, 0, None, None, None, 0, None, 0) == L.ERR_INVALID_ARGUMENT
    assert (info.n_mid, info.n_l2) == (77, 78) and (root == 0x5A).all()
