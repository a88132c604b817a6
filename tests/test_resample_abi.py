"""Model resampling on the host side (dust_hip_model_resample): the entry point is declared, exported, bound, documented and mirrored; the
two records' layouts and the constants are the same in the C header, the ctypes binding, the numpy dtypes and the witness; the call
refuses without a device and leaves the counts alone; the header states the rules and what is out of scope; the host helpers make the
records the header describes; the C++ mirror compiles. (What resample_op_refusal, resample_map_refusal and device_resample make of a record is
tests/test_resample_rule.py's tables.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resample_witness as W
import stamp_witness as S
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_resample"


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
    for record in ("DustHipResample", "DustHipResampleCount"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert all(callable(f) for f in (api.Model.resample, api.resamples, api.rotation_about))
    assert header.index("Model fracture:") < header.index("Model resampling:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model resampling:"):])     # (the comment's line breaks and stars out of the way, the products' too)
    block = block[:block.index("dust_hip_model_resample(DustHipModel")]
    for sentence in ("1 / DUST_HIP_RESAMPLE_ONE = 1 / 65536 voxel", "point sampling at the destination voxel's centre",
                     "Q[k] = m[k][0] (2x + 1) + m[k][1] (2y + 1) + m[k][2] (2z + 1) + 2 t[k], s[k] = floor(Q[k] / 131072)",
                     "Q[k] = -1 gives s[k] = -1, not 0", "|m[k][r]| <= 8 65536 and |t[k]| <= 2^28", "1 340 604 416 < 2^31", "the device computes in 32 bits",
                     "it keeps its value under every op, REPLACE included", "A singular m is legal", "dst_lo > dst_hi on some axis", "src_lo > src_hi on some axis",
                     "wholly outside the tree", "with the same values and the same table", "the records apply in array order", "also when src == dst",
                     "byte for byte what dust_hip_model_create builds", "invalidated exactly as by a stamp", "is not made editable", "nothing is written",
                     "independently of the others", "blocked == 0 means the piece fits", "exactly as cast does", "flag bits other than DRY_RUN",
                     "an m or t beyond its limit", "a palette_map entry above 254", "exactly where stamp returns it", "before the records are looked at",
                     "defined by the integer record"):
        assert sentence in block, sentence
    for scope in ("filtered sampling", "dust_hip_model_reduce is the tool for whole levels", "float matrices in the ABI", "perspective maps", "4096^3 trees",
                  "an asynchronous form", "a rotating cast"):                     # what the header rules out
        assert scope in block[block.index("Out of scope:"):], scope
    assert "defined by the integer record" in api.Model.resample.__doc__ and "defined by that integer record" in re.sub(r"\s+", " ", api.resamples.__doc__)


def _c_layout(tmp_path):
    exe = str(tmp_path / "resample_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "resample_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipResample", L.Resample, api.RESAMPLE_DTYPE, W.RESAMPLE_DTYPE, 96),
               ("DustHipResampleCount", L.ResampleCount, api.RESAMPLE_COUNT_DTYPE, W.COUNT_DTYPE, 16))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == dtype.itemsize == size
        assert [f for f, _ in struct._fields_] == list(witness.names) == list(dtype.names)
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1] == dtype.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            assert dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert [c["DustHipResample." + f] for f in ("m", "t", "dst_lo", "dst_hi", "src_lo", "src_hi", "op", "reserved")] == [0, 36, 48, 60, 72, 76, 80, 84]
    assert c["DUST_HIP_RESAMPLE_ONE"] == L.RESAMPLE_ONE == W.ONE == 65536
    assert c["DUST_HIP_RESAMPLE_MAX_M"] == L.RESAMPLE_MAX_M == W.MAX_M == 8 * 65536 and c["DUST_HIP_RESAMPLE_MAX_T"] == L.RESAMPLE_MAX_T == W.MAX_T == 2 ** 28
    assert c["DUST_HIP_RESAMPLE_DRY_RUN"] == L.RESAMPLE_DRY_RUN == W.DRY_RUN == 1 and c["DUST_HIP_MAX_RESAMPLES"] == L.MAX_RESAMPLES == W.MAX_RESAMPLES == 65536
    ops = ("PLACE", "OVERWRITE", "REPLACE", "CARVE", "PAINT")
    assert [c["DUST_HIP_STAMP_" + o] for o in ops] == [getattr(L, "STAMP_" + o) for o in ops] == [getattr(W, o) for o in ops] == [0, 1, 2, 3, 4]
    # the header's bound on |Q|
    assert 3 * W.MAX_M * 511 + 2 * W.MAX_T == 1340604416 < 2 ** 31


def test_host_helpers_make_the_records_the_header_describes():
    # a signed axis permutation at an integer offset: the record is exact, and it is the stamp's geometry
    for word in S.all_orientations()[::5]:
        p, g = S.orient_fields(word)
        lo, hi, offset = (3, 9, 14), (7, 14, 20), (13, 29, 45)
        f = np.zeros((3, 4))
        for r in range(3):
            f[r, p[r]] = -1.0 if g[r] else 1.0
            f[r, 3] = offset[r] + (hi[p[r]] + 1 if g[r] else -lo[p[r]])
        rec = api.resamples(f, L.STAMP_REPLACE, lo, hi)[0]
        assert rec["op"] == L.STAMP_REPLACE and rec["src_lo"].tolist() == list(lo) and rec["src_hi"].tolist() == list(hi) and not rec["reserved"].any()
        extent = [hi[p[r]] - lo[p[r]] for r in range(3)]
        assert rec["dst_lo"].tolist() == [o - 1 for o in offset] and rec["dst_hi"].tolist() == [o + e + 1 for o, e in zip(offset, extent)]
        assert set(np.abs(rec["m"]).reshape(-1).tolist()) == {0, W.ONE}
        inside, s = W.image_of(rec, [int(v) for v in rec["dst_lo"]], [int(v) for v in rec["dst_hi"]])
        assert inside[1:-1, 1:-1, 1:-1].all() and inside.sum() == np.prod([e + 1 for e in extent])
        for r in range(3):
            u = np.arange(extent[r] + 1)
            want = hi[p[r]] - u if g[r] else lo[p[r]] + u
            got = np.moveaxis(s[p[r]][1:-1, 1:-1, 1:-1], r, 0)[:, 0, 0]
            assert got.tolist() == want.tolist()
    # a rotation about an axis: the pivots correspond, the inverse is rounded to 1 / 65536, the box holds the image
    f = api.rotation_about("z", 30.0, (10.0, 20.0, 30.0), (100.0, 110.0, 120.0), scale=1.5)
    assert np.allclose(f[:, :3] @ np.array([10.0, 20.0, 30.0]) + f[:, 3], [100.0, 110.0, 120.0])
    assert np.allclose(f[:, :3] @ f[:, :3].T, 2.25 * np.eye(3)) and np.allclose(f[2, :3], [0, 0, 1.5])
    assert np.allclose(api.rotation_about(2, 30.0, (0, 0, 0), (0, 0, 0)), api.rotation_about((0, 0, 5), 30.0, (0, 0, 0), (0, 0, 0)))
    assert np.allclose(api.rotation_about("x", 90.0, (0, 0, 0), (0, 0, 0))[:, :3] @ [0, 1, 0], [0, 0, 1])
    rec = api.resamples(f, L.STAMP_PLACE, (5, 15, 25), (14, 24, 34))[0]
    inv = np.linalg.inv(f[:, :3])
    assert rec["m"].tolist() == np.rint(inv * 65536).astype(int).tolist() and rec["t"].tolist() == np.rint(-(inv @ f[:, 3]) * 65536).astype(int).tolist()
    whole = W.records([rec["m"]], [rec["t"]], (0, 0, 0), (255, 255, 255), src_lo=(5, 15, 25), src_hi=(14, 24, 34))[0]
    inside, _ = W.image_of(whole, [0, 0, 0], [255, 255, 255])
    where = np.argwhere(inside)
    assert len(where) > 1000 and (where.min(axis=0) > rec["dst_lo"]).all() and (where.max(axis=0) < rec["dst_hi"]).all()
    # refusals of the helper: singular, and beyond the limits
    with pytest.raises(ValueError):
        api.resamples(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        api.resamples(np.hstack([np.eye(3) / 8.001, np.zeros((3, 1))]))
    with pytest.raises(ValueError):
        api.resamples(np.hstack([np.eye(3), np.full((3, 1), 4097.0)]))
    assert len(api.resamples(np.hstack([np.eye(3) / 8.0, np.full((3, 1), 512.0)]))) == 1
    assert len(api.resamples(np.zeros((0, 3, 4)))) == 0


def test_call_refuses_without_a_device_and_leaves_the_counts_alone():
    lib = L.load()
    good = W.records([np.eye(3) * W.ONE], [(0, 0, 0)], (0, 0, 0), (9, 9, 9))
    counts = np.full(32, 0x5A, np.uint8).view(api.RESAMPLE_COUNT_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    palette_map = np.arange(255, dtype=np.uint8)
    for records, n in ((good, 1), (None, 0), (None, 1), (good, L.MAX_RESAMPLES + 1)):
        for flags in (0, L.RESAMPLE_DRY_RUN, 2):
            for pm in (None, palette_map):
                assert lib.dust_hip_model_resample(None, None, None if records is None else ptr(records), n, None if pm is None else ptr(pm), flags,
                                                   ptr(counts)) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert counts.tobytes() == bytes([0x5A]) * 32


def test_cpp_mirror_resample_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "resample_mirror.cpp"), "-o", str(tmp_path / "resample_mirror.o")])
