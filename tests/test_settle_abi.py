"""Model settling on the host side (dust_hip_model_settle, dust_hip_model_settle_apply): the entry points are declared, exported,
bound, documented and mirrored; the three records' layouts and the constants are the same in the C header, the ctypes binding, the
numpy dtypes and the witness; the calls refuse without a device and leave the outputs alone; the header states the contract, the
descent identity and what is out of scope; the C++ mirror compiles. (What device_settle makes of every query, refusals included, is
tests/test_settle_rule.py's validation table.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import settle_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_settle", "dust_hip_model_settle_apply")


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
    for record in ("DustHipSettleQuery", "DustHipSettleResult", "DustHipSettleApplied"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.settle) and callable(api.Model.settle_apply) and callable(api.loose_mask)
    assert header.index("Model neighbourhoods:") < header.index("Model settling:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model settling:"):])     # (the comment's line breaks and margin stars out of the way)
    block = block[:block.index("dust_hip_model_settle_apply(DustHipModel")]
    for sentence in ("query.toward is exactly one DUST_HIP_FACE_", "the plane axes of dust_hip_model_columns", "a coordinate >= 256 is refused", "neither consulted nor changed",
                     "is a floor, and nothing falls in from above the region", "every other solid voxel is fixed", "All 255 bits set: everything is loose",
                     "a stable compaction per stretch between fixed voxels", "keep their order and their palette indices",
                     "the voxel above p is empty or outside the region and p + d and p + d + g are both inside the region and empty",
                     "A destination has one possible source, and sources and destinations are disjoint", "d = +u, -u, +v, -v for k mod 4 = 0, 1, 2, 3, then a fall",
                     "ask first, apply after", "0 is a plain vertical settle", "1 + the index of the last generation that moved a voxel",
                     "the initial fall is not in fell", "the rows after a fixed point are 0", "s(before) - s(after) == fall_sum + slid",
                     "four consecutive generations", "how often it looks does not show in any output", "only when a grid byte is needed, that is when loose is not all-ones",
                     "rebuilds ONCE", "even when nothing moved", "loose bit 255", "generations above 256", "before the query is looked at"):
        assert sentence in block, sentence
    for scope in ("angles of repose other than 45 degrees", "liquids", "settling across the instances of a scene", "4096^3 trees", "an asynchronous form",
                  "a brick worklist between generations"):                        # what the header rules out
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "settle_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "settle_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipSettleQuery", L.SettleQuery, api.SETTLE_QUERY_DTYPE, W.QUERY_DTYPE, 72),
               ("DustHipSettleResult", L.SettleResult, api.SETTLE_RESULT_DTYPE, W.RESULT_DTYPE, 64),
               ("DustHipSettleApplied", L.SettleApplied, api.SETTLE_APPLIED_DTYPE, W.APPLIED_DTYPE, 64))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == dtype.itemsize == size
        assert [f for f, _ in struct._fields_] == list(witness.names) == list(dtype.names)
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1] == dtype.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            assert dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert c["DustHipSettleQuery.loose"] == 40 and c["DustHipSettleResult.fall_sum"] == 24 and c["DustHipSettleResult.changed_columns"] == 40
    assert c["DustHipSettleApplied.slid"] == 16 and c["DustHipSettleApplied.fell"] == 24 and c["DustHipSettleApplied.fall_sum"] == 32
    assert dict(L.SettleApplied._fields_)["slid"] is C.c_uint64 and dict(L.SettleResult._fields_)["fall_sum"] is C.c_uint64
    assert c["DUST_HIP_SETTLE_MAX_GENERATIONS"] == L.SETTLE_MAX_GENERATIONS == W.MAX_GENERATIONS == 256
    faces = [c["DUST_HIP_FACE_" + n] for n in ("NEG_X", "POS_X", "NEG_Y", "POS_Y", "NEG_Z", "POS_Z")]
    assert faces == list(W.FACES) == [L.FACE_NEG_X, L.FACE_POS_X, L.FACE_NEG_Y, L.FACE_POS_Y, L.FACE_NEG_Z, L.FACE_POS_Z]


def test_loose_mask():
    assert api.loose_mask() == W.ALL_LOOSE == (0xFFFFFFFF,) * 7 + (0x7FFFFFFF,)
    assert api.loose_mask([]) == (0,) * 8 and api.loose_mask([0, 33, (62, 65), np.int64(254)]) == W.loose_mask([0, 33, (62, 65), 254]) == (1, 2 | (3 << 30), 3, 0, 0, 0, 0, 1 << 30)
    assert api.loose_mask([(0, 254)]) == W.ALL_LOOSE


def test_calls_refuse_without_a_device_and_leave_the_outputs_alone():
    lib = L.load()

    def query(toward=4, flags=0, reserved=0, lo=(0, 0, 0), hi=(255, 255, 255), loose=W.ALL_LOOSE, size=C.sizeof(L.SettleQuery)):
        q = L.SettleQuery(struct_size=size, toward=toward, flags=flags, reserved=reserved)
        q.lo[:], q.hi[:], q.loose[:] = lo, hi, loose
        return q
    result = np.full(64, 0x5A, np.uint8).view(api.SETTLE_RESULT_DTYPE)
    applied = np.full(64, 0x5A, np.uint8).view(api.SETTLE_APPLIED_DTYPE)
    rows = np.full(512, 0x5A5A5A5A, np.uint32)
    before = result.tobytes(), applied.tobytes(), rows.tobytes()
    rp, ap, gp = (a.ctypes.data_as(C.c_void_p) for a in (result, applied, rows))
    # every refusal of the header, through the entry points: a null model, then the query's faults one at a time
    queries = [query(), query(size=71), query(size=0), query(toward=0), query(toward=3), query(toward=64), query(flags=1), query(reserved=7), query(lo=(256, 0, 0)),
               query(hi=(255, 256, 255)), query(loose=(0,) * 7 + (1 << 31,)), query(loose=(0xFFFFFFFF,) * 8)]
    for q in queries:
        assert lib.dust_hip_model_settle(None, C.byref(q), rp) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_settle_apply(None, C.byref(q), 1, ap, gp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_settle(None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_settle_apply(None, None, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), applied.tobytes(), rows.tobytes()) == before
    for q in queries[3:]:                                                         # ... and each of those is one the witness refuses too
        assert W.refused(q.toward, q.flags, q.reserved, tuple(q.lo), tuple(q.hi), tuple(q.loose))
    assert not W.refused(32, 0, 0, (255, 255, 255), (0, 0, 0), W.loose_mask([]), 256) and W.refused(32, 0, 0, (0,) * 3, (0,) * 3, W.ALL_LOOSE, 257)


def test_cpp_mirror_settle_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "settle_mirror.cpp"), "-o", str(tmp_path / "settle_mirror.o")])
