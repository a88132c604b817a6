"""The witness of the model stamps (tests/stamp_witness.py) against the header's formula read voxel by voxel, and the host side of
dust_hip_model_stamp: declared, bound, and refusing a null model without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stamp_witness as S
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def naive(dst, src, stamp, palette_map=None):
    """include/dust_hip.h, the Geometry and Values paragraphs, one destination voxel at a time"""
    out = dst.copy()
    offset = [int(v) for v in stamp["offset"]]
    lo = [int(v) for v in stamp["src_lo"]]
    hi = [int(v) for v in stamp["src_hi"]]
    orient, op = int(stamp["orient"]), int(stamp["op"])
    p = [(orient >> (2 * r)) & 3 for r in range(3)]
    g = [(orient >> (6 + r)) & 1 for r in range(3)]
    if any(lo[k] > hi[k] for k in range(3)):
        return out, 0
    e = [hi[k] - lo[k] for k in range(3)]
    changed = 0
    box = [range(max(offset[r], 0), min(offset[r] + e[p[r]], 255) + 1) for r in range(3)]
    for dx in box[0]:
        for dy in box[1]:
            for dz in box[2]:
                d = (dx, dy, dz)
                s = [0, 0, 0]
                for r in range(3):
                    u = d[r] - offset[r]
                    s[p[r]] = lo[p[r]] + u if g[r] == 0 else hi[p[r]] - u
                byte = int(src[tuple(s)])
                v = 0 if byte == 0 else (byte if palette_map is None else int(palette_map[byte - 1]) + 1)
                w = int(dst[d])
                if op == S.PLACE:
                    to = v if v and not w else w
                elif op == S.OVERWRITE:
                    to = v if v else w
                elif op == S.REPLACE:
                    to = v
                elif op == S.CARVE:
                    to = 0 if v else w
                else:
                    to = v if v and w else w
                changed += to != w
                out[d] = to
    return out, changed


def small_source(seed=5):
    """a 3 x 4 x 5 box at (250, 3, 100) of a 256^3 grid: distinct materials, a third of the voxels empty"""
    rng = np.random.default_rng(seed)
    src = np.zeros((256,) * 3, np.uint8)
    box = (1 + np.arange(60, dtype=np.uint8)).reshape(3, 4, 5)
    box[rng.random((3, 4, 5)) < 1 / 3] = 0
    src[250:253, 3:7, 100:105] = box
    return src, (250, 3, 100), (252, 6, 104)


def test_the_48_orientations_are_distinct_and_valid():
    words = S.all_orientations()
    assert len(set(words)) == 48 and S.IDENTITY in words and api.ORIENT_IDENTITY == S.IDENTITY
    assert all(S.orient_fields(w) is not None for w in words)
    assert sum(S.orient_fields(w) is not None for w in range(1024)) == 48
    for perm in ((0, 1, 2), (2, 0, 1), (1, 0, 2)):
        for flips in ((0, 0, 0), (1, 0, 1)):
            assert api.orientation(perm, flips) == S.orient_word(perm, flips)


@pytest.mark.parametrize("op", [S.PLACE, S.OVERWRITE, S.REPLACE, S.CARVE, S.PAINT])
def test_witness_agrees_with_the_header_formula_voxel_by_voxel(op):
    src, lo, hi = small_source()
    rng = np.random.default_rng(6)
    dst = np.zeros((256,) * 3, np.uint8)
    dst[:12, 250:, 120:134] = np.where(rng.random((12, 6, 14)) < 0.5, rng.integers(100, 256, (12, 6, 14)), 0)
    pm = rng.permutation(255).astype(np.uint8)
    for k, orient in enumerate(S.all_orientations()):
        # half of the images hang over the tree's edge on two axes
        offset = (-2, 253, 125) if k % 2 else (4, 250, 122)
        stamp = S.records([offset], orient, op, lo, hi)[0]
        for palette_map in (None, pm):
            got = dst.copy()
            n = S.stamp_one(got, src, stamp, palette_map)
            want, want_n = naive(dst, src, stamp, palette_map)
            assert np.array_equal(got, want) and n == want_n, (orient, op)
            assert op in (S.CARVE, S.PAINT) or n > 0


def test_an_orientation_and_its_inverse_give_the_source_back():
    src, lo, hi = small_source(7)
    for orient in S.all_orientations():
        p, _ = S.orient_fields(orient)
        there, n = S.stamp(np.zeros_like(src), src, S.records([(10, 20, 30)], orient, S.REPLACE, lo, hi))
        assert n[0] == np.count_nonzero(src)
        image_hi = [10 + hi[p[0]] - lo[p[0]], 20 + hi[p[1]] - lo[p[1]], 30 + hi[p[2]] - lo[p[2]]]
        back, _ = S.stamp(np.zeros_like(src), there, S.records([lo], S.inverse(orient), S.REPLACE, (10, 20, 30), image_hi))
        assert np.array_equal(back, src), orient
        assert S.inverse(S.inverse(orient)) == orient


def test_offsets_at_the_int32_limits_and_empty_boxes_change_nothing():
    src, lo, hi = small_source()
    dst = np.full((256,) * 3, 9, np.uint8)
    for offset in ((-2 ** 31, 0, 0), (2 ** 31 - 1, 0, 0), (0, 256, 0), (0, 0, -5)):
        out, n = S.stamp(dst, src, S.records([offset], S.IDENTITY, S.REPLACE, lo, hi))
        assert n.tolist() == [0] and np.array_equal(out, dst)
    out, n = S.stamp(dst, src, S.records([(0, 0, 0)], S.IDENTITY, S.REPLACE, (5, 0, 0), (4, 255, 255)))
    assert n.tolist() == [0] and np.array_equal(out, dst)


def test_snapshot_when_a_grid_is_stamped_onto_itself():
    grid = np.zeros((256,) * 3, np.uint8)
    grid[10:14, 0, 0] = [1, 2, 3, 4]
    out, n = S.stamp(grid, grid, S.records([(11, 0, 0)], S.IDENTITY, S.REPLACE, (10, 0, 0), (13, 0, 0)))
    assert out[10:15, 0, 0].tolist() == [1, 1, 2, 3, 4] and n.tolist() == [4]


def test_entry_point_is_bound_and_refuses_a_null_model_without_a_device():
    assert "dust_hip_model_stamp" in L.SYMBOLS
    assert C.sizeof(L.Stamp) == api.STAMP_DTYPE.itemsize == S.STAMP_DTYPE.itemsize == 32
    assert [f for f, _ in L.Stamp._fields_] == list(api.STAMP_DTYPE.names) == list(S.STAMP_DTYPE.names)
    for field, _ in L.Stamp._fields_:
        assert getattr(L.Stamp, field).offset == api.STAMP_DTYPE.fields[field][1] == S.STAMP_DTYPE.fields[field][1], field
    assert (L.STAMP_PLACE, L.STAMP_OVERWRITE, L.STAMP_REPLACE, L.STAMP_CARVE, L.STAMP_PAINT) == (S.PLACE, S.OVERWRITE, S.REPLACE, S.CARVE, S.PAINT)
    assert L.MAX_STAMPS == S.MAX_STAMPS == 65536
    lib = L.load()
    stamps = api.stamps([(0, 0, 0)])
    changed = np.full(1, 77, np.uint32)
    sp, cp = stamps.ctypes.data_as(C.c_void_p), changed.ctypes.data_as(C.c_void_p)
    assert lib.dust_hip_model_stamp(None, None, sp, 1, None, cp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_stamp(None, None, None, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert changed.tolist() == [77]
    assert callable(api.Model.stamp)


def test_record_layout_and_constants_match_the_header(tmp_path):
    exe = str(tmp_path / "stamp_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stamp_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert c["DustHipStamp"] == C.sizeof(L.Stamp) == 32
    for field, _ in L.Stamp._fields_:
        assert getattr(L.Stamp, field).offset == c[f"DustHipStamp.{field}"] == api.STAMP_DTYPE.fields[field][1], field
    assert (c["DUST_HIP_STAMP_PLACE"], c["DUST_HIP_STAMP_OVERWRITE"], c["DUST_HIP_STAMP_REPLACE"], c["DUST_HIP_STAMP_CARVE"], c["DUST_HIP_STAMP_PAINT"]) == \
        (L.STAMP_PLACE, L.STAMP_OVERWRITE, L.STAMP_REPLACE, L.STAMP_CARVE, L.STAMP_PAINT)
    assert c["DUST_HIP_MAX_STAMPS"] == L.MAX_STAMPS


def test_cpp_mirror_stamp_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "stamp_mirror.cpp"), "-o", str(tmp_path / "stamp_mirror.o")])


# ---- the device path's arithmetic, ported line by line (dust_amd/csrc/stamp.hip k_stamp, model_records.hpp device_stamp): no device runs
# here, but the per-axis scatter, the affine maps, the clipping and the op tables are plain integer code that Python can follow
def _leaf_address(x, y, z):
    """edit.hpp leaf_code(x >> 2, y >> 2, z >> 2) * 64 + the voxel bit: where a voxel's byte lies in the brick-major grid"""
    bx, by, bz = x >> 2, y >> 2, z >> 2
    code = ((((bx >> 2) << 8) | ((by >> 2) << 4) | (bz >> 2)) << 6) | ((bx & 3) << 4) | ((by & 3) << 2) | (bz & 3)
    return code * 64 + (((x & 3) << 4) | ((y & 3) << 2) | (z & 3))


def _scatter(c, axis):
    c &= 0xFFFFFFFF
    return (((c >> 4) << (20 - 4 * axis)) | (((c >> 2) & 3) << (10 - 2 * axis)) | ((c & 3) << (4 - 2 * axis))) & 0xFFFFFFFF


def _device_stamp(s):
    lo, hi = [int(v) for v in s["src_lo"]], [int(v) for v in s["src_hi"]]
    if any(a > b for a, b in zip(lo, hi)):
        return None
    orient = int(s["orient"])
    d = {"base": [], "lo": [], "hi": [], "orient": orient}
    for r in range(3):
        p, flip, off = (orient >> (2 * r)) & 3, (orient >> (6 + r)) & 1, int(s["offset"][r])
        first, last = max(off, 0), min(off + hi[p] - lo[p], 255)
        if first > last:
            return None
        d["lo"].append(first)
        d["hi"].append(last)
        d["base"].append(hi[p] + off if flip else lo[p] - off)
        assert -(1 << 31) <= d["base"][-1] < 1 << 31
    keep, take, clear = 0, 1, 2
    table = lambda ee, es, se, ss: ee | es << 2 | se << 4 | ss << 6  # noqa: E731
    d["table"] = {S.PLACE: table(keep, keep, take, keep), S.OVERWRITE: table(keep, keep, take, take), S.REPLACE: table(take, take, take, take),
                  S.CARVE: table(keep, keep, keep, clear), S.PAINT: table(keep, keep, keep, take)}[int(s["op"])]
    return d


def _kernel(dst_bytes, src_bytes, d, byte_map):
    n, orient = 0, d["orient"]
    p = [(orient >> (2 * r)) & 3 for r in range(3)]
    g = [(orient >> (6 + r)) & 1 for r in range(3)]
    for x in range(d["lo"][0], d["hi"][0] + 1):
        ax = _scatter(d["base"][0] + (-x if g[0] else x), p[0])
        for y in range(d["lo"][1], d["hi"][1] + 1):
            ay = _scatter(d["base"][1] + (-y if g[1] else y), p[1])
            for z in range(d["lo"][2], d["hi"][2] + 1):
                address = ax + ay + _scatter(d["base"][2] + (-z if g[2] else z), p[2])
                assert 0 <= address < 1 << 24        # every load the kernel issues lies inside the 16 MiB grid
                v = int(byte_map[src_bytes[address]])
                at = _leaf_address(x, y, z)
                w = int(dst_bytes[at])
                act = (d["table"] >> (((2 if v else 0) | (1 if w else 0)) * 2)) & 3
                to = w if act == 0 else v if act == 1 else 0
                if to != w:
                    n += 1
                    dst_bytes[at] = to
    return n


def test_the_kernels_address_arithmetic_agrees_with_the_witness():
    rng = np.random.default_rng(1)
    src = np.zeros((256,) * 3, np.uint8)
    src[240:256, 0:20, 100:120] = np.where(rng.random((16, 20, 20)) < 0.6, rng.integers(1, 256, (16, 20, 20)), 0)
    dst = np.zeros((256,) * 3, np.uint8)
    dst[0:40, 236:256, 0:40] = np.where(rng.random((40, 20, 40)) < 0.5, rng.integers(1, 256, (40, 20, 40)), 0)
    palette_map = rng.integers(0, 255, 255).astype(np.uint8)
    byte_map = np.concatenate([[0], palette_map.astype(np.int64) + 1]).astype(np.uint8)
    address = _leaf_address(*np.indices((256,) * 3))
    assert len(np.unique(address)) == 1 << 24
    src_bytes, dst_bytes = np.zeros(1 << 24, np.uint8), np.zeros(1 << 24, np.uint8)
    src_bytes[address.reshape(-1)] = src.reshape(-1)
    dst_bytes[address.reshape(-1)] = dst.reshape(-1)
    window = (slice(0, 48), slice(200, 256), slice(0, 48))      # every image lands in here
    covered = 0
    for k, orient in enumerate(S.all_orientations()):
        offset = (int(rng.integers(-5, 30)), int(rng.integers(230, 258)), int(rng.integers(-8, 30)))
        hi = (241 + int(rng.integers(0, 9)), 2 + int(rng.integers(0, 9)), 101 + int(rng.integers(0, 9)))
        stamp = S.records([offset], orient, k % 5, (241, 2, 101), hi)
        want, counts = S.stamp(dst, src, stamp, palette_map)
        got = dst_bytes.copy()
        d = _device_stamp(stamp[0])
        n = _kernel(got, src_bytes, d, byte_map) if d else 0
        assert n == counts[0] and np.array_equal(got[address[window]], want[window]), (k, orient)
        covered += d is not None
    assert covered >= 24        # (an image whose offset lies past an edge by more than its extent covers nothing)
