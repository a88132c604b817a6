"""dust_amd/csrc/model_records.hpp, the device-free half of the model calls, run as native code on a CPU: tests/cpp/model_records_test.cpp
compiled with g++ under AddressSanitizer and UBSan (no HIP compiler, not linked against the library) reads caller records from a file
and writes the device records, the chunk ends, the cell lists, the cast work items and the decoded cast hits to another. They are held
to the Python ports that are themselves held to the witnesses (device_cast of tests/test_cast_walk_port.py, _device_stamp of
tests/test_stamp_witness.py), to tests/shape_edit_witness.py, to a brute-force binning and to tests/cast_witness.py."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cast_witness as CW
import shape_edit_witness as SW
import stamp_witness as TW
from test_cast_walk_port import OFFSET_LIMIT, WALLS_BIT, device_cast
from test_stamp_witness import _device_stamp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "model_records_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "model_records_test")

DEV_SHAPE = np.dtype([("a", "<f4", 3), ("kind", "<u4"), ("b", "<f4", 3), ("radius", "<f4"), ("solid_to", "<u4"), ("empty_to", "<u4"), ("lo", "<u4"), ("hi", "<u4")])
DEV_STAMP = np.dtype([("base", "<i4", 3), ("lo", "<u4"), ("hi", "<u4"), ("orient", "<u4"), ("table", "<u4"), ("pad", "<u4")])
DEV_CAST = np.dtype([("off", "<i4", 3), ("orient", "<u4"), ("step", "<i4", 3), ("max_steps", "<u4"), ("k_lo", "<u4"), ("k_hi", "<u4"), ("lo", "<u4"), ("hi", "<u4")])
ITEM = np.dtype([("cast", "<u4"), ("cell", "<u4")])
DECODE = np.dtype([("cast", CW.CAST_DTYPE), ("best", "<u8"), ("contacts", "<u4"), ("voxels", "<u4"), ("wall", "<u4"), ("pad", "<u4")])
assert (DEV_SHAPE.itemsize, DEV_STAMP.itemsize, DEV_CAST.itemsize, DECODE.itemsize) == (48, 32, 48, 72)
NO_HIT = (1 << 64) - 1
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SPECIAL = [I32_MIN, I32_MIN + 1, -256, -1, 0, 255, 256, I32_MAX - 1, I32_MAX]


@pytest.fixture(scope="module")
def exe():
    """built once, again when the program or a header it includes is newer (as tests/test_cpp_mirror.py caches its binary)"""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "dust_hip.h")] + [os.path.join(CSRC, h) for h in ("model_records.hpp", "cast.hpp", "stamp.hpp", "edit.hpp", "grid.hpp", "dust_dev.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                               "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE])
    return EXE


class Out:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, dtype, n=1):
        a = np.frombuffer(self.data, dtype, n, self.at)
        self.at += a.nbytes
        return a


def run(exe, tmp_path, shapes=(), stamps=(), casts=(), bounds=(), configs=(), decode=()):
    """one run of the program (which must end clean under both sanitizers) -> what it wrote, parsed"""
    shapes, stamps, casts, decode = (np.zeros(0, dt) if len(a) == 0 else np.asarray(a, dt).reshape(-1)
                                     for a, dt in ((shapes, SW.SHAPE_DTYPE), (stamps, TW.STAMP_DTYPE), (casts, CW.CAST_DTYPE), (decode, DECODE)))
    bounds, configs = np.asarray(bounds, "<u4").reshape(-1, 2), np.asarray(configs, "<u4").reshape(-1, 2)
    head = np.array([len(shapes), len(stamps), len(casts), len(bounds), len(configs), len(decode)], "<u4")
    (tmp_path / "in.bin").write_bytes(b"".join(a.tobytes() for a in (head, shapes, stamps, casts, bounds, configs, decode)))
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    o = Out((tmp_path / "out.bin").read_bytes())
    r = {}
    for name, n, dev in (("shapes", len(shapes), DEV_SHAPE), ("stamps", len(stamps), DEV_STAMP), ("casts", len(casts), DEV_CAST)):
        r[name] = o.take(np.dtype([("live", "<u4"), ("d", dev)]), n)
    r["index"] = o.take("<u4", int(o.take("<u4")[0]))
    r["chunks"] = []
    for _ in configs:
        chunks = []
        for _ in range(int(o.take("<u4")[0])):
            c1, n_cells, n_ids, n_items = (int(v) for v in o.take("<u4", 4))
            chunks.append(dict(c1=c1, cells=o.take("<u4", n_cells), starts=o.take("<u4", n_cells + 1), ids=o.take("<u2", n_ids), items=o.take(ITEM, n_items)))
        r["chunks"].append(chunks)
    r["hits"] = o.take(CW.HIT_DTYPE, len(decode))
    r["shape_limit_end"], r["cast_limit_end"] = (int(v) for v in o.take("<u4", 2))
    r["offset_limit"] = int(o.take("<i4")[0])
    assert o.at == len(o.data)
    return r


def pack(v):
    return int(v[0]) | int(v[1]) << 8 | int(v[2]) << 16


def offsets(rng, n):
    """per component: one of the int32 edge values, or a value from a small range around the tree"""
    near = rng.integers(-300, 560, (n, 3))
    return np.where(rng.random((n, 3)) < 0.5, rng.choice(SPECIAL, (n, 3)), near)


def sub_boxes(rng, n):
    """(lo, hi): boxes of every size from a voxel to the tree, one in eight empty on some axis (lo > hi)"""
    lo = rng.integers(0, 256, (n, 3))
    hi = np.minimum(lo + rng.choice([0, 1, 3, 15, 16, 100, 255], (n, 3)), 255)
    empty = rng.random(n) < 0.125
    axis = rng.integers(0, 3, n)
    lo[empty, axis[empty]] = np.maximum(lo[empty, axis[empty]], 1)
    hi[empty, axis[empty]] = lo[empty, axis[empty]] - rng.integers(1, 3, n)[empty].clip(None, lo[empty, axis[empty]])
    return lo, hi


def test_device_cast_is_the_port(exe, tmp_path):
    rng = np.random.default_rng(41)
    words = TW.all_orientations()
    combos = [(w, (x, y, z), walls, ms) for w in words for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) for walls in (0, 1) for ms in (0, 1, 65535)]
    n = len(combos)
    assert n == 48 * 27 * 2 * 3
    lo, hi = sub_boxes(rng, n)
    casts = CW.records(offsets(rng, n), [c[1] for c in combos], [c[3] for c in combos], [c[0] for c in combos], [c[2] for c in combos], lo, hi)
    casts[:9]["offset"] = [(v, v, v) for v in SPECIAL]      # (every edge value on every axis at least once, with a sub-box)
    casts[:9]["src_lo"], casts[:9]["src_hi"] = (3, 4, 5), (30, 20, 10)
    r = run(exe, tmp_path, casts=casts)
    assert r["offset_limit"] == OFFSET_LIMIT
    live = []
    for i, (c, got) in enumerate(zip(casts, r["casts"])):
        want = device_cast(c)
        assert bool(got["live"]) == (want is not None), (i, c)
        if want is None:
            continue
        live.append(i)
        d = got["d"]
        assert d["off"].tolist() == want["off"] and d["step"].tolist() == want["step"], (i, c, d, want)
        assert (int(d["orient"]), int(d["max_steps"]), int(d["k_lo"]), int(d["k_hi"])) == (want["orient"], want["max_steps"], want["k_lo"], want["k_hi"]), (i, c, d, want)
        assert (int(d["lo"]), int(d["hi"])) == (pack(want["lo"]), pack(want["hi"])), (i, c, d, want)
        assert bool(d["orient"] & WALLS_BIT) == bool(c["flags"] & 1)
        assert d["k_lo"] <= 65535 + 1 and d["k_hi"] <= 65535 + 1 and np.abs(d["off"].astype(np.int64)).max() <= OFFSET_LIMIT
    assert r["index"].tolist() == live and 0.5 * n < len(live) < n
    walked = r["casts"]["d"][live]
    assert np.count_nonzero(walked["k_lo"] <= walked["k_hi"]) > n // 20 and np.count_nonzero(walked["k_lo"] > walked["k_hi"]) > n // 20


def test_device_stamp_is_the_port(exe, tmp_path):
    rng = np.random.default_rng(42)
    words = TW.all_orientations()
    combos = [(w, op) for w in words for op in (TW.PLACE, TW.OVERWRITE, TW.REPLACE, TW.CARVE, TW.PAINT)] * 12
    n = len(combos)
    lo, hi = sub_boxes(rng, n)
    off = offsets(rng, n)
    off[n // 2:] = rng.integers(-120, 256, (n - n // 2, 3))     # (half of them close enough to land)
    stamps = TW.records(off, [c[0] for c in combos], [c[1] for c in combos], lo, hi)
    r = run(exe, tmp_path, stamps=stamps)
    n_live = 0
    for i, (s, got) in enumerate(zip(stamps, r["stamps"])):
        want = _device_stamp(s)
        assert bool(got["live"]) == (want is not None), (i, s)
        if want is None:
            continue
        n_live += 1
        d = got["d"]
        assert all(I32_MIN <= b <= I32_MAX for b in want["base"])
        assert d["base"].tolist() == want["base"] and (int(d["lo"]), int(d["hi"])) == (pack(want["lo"]), pack(want["hi"])), (i, s, d, want)
        assert (int(d["orient"]), int(d["table"]), int(d["pad"])) == (want["orient"], want["table"], 0), (i, s, d, want)
    assert n // 8 < n_live < n
    assert {int(s["op"]) for s, got in zip(stamps, r["stamps"]) if got["live"]} == {0, 1, 2, 3, 4}


def edge_shapes():
    B, S, C = SW.BOX, SW.SPHERE, SW.CAPSULE
    nan, inf = float("nan"), float("inf")
    return SW.shapes(
        SW.shape(B, (300.0, 10.0, 10.0), (310.0, 20.0, 20.0), op=SW.FILL, palette=1),            # entirely outside the tree
        SW.shape(B, (-40.0, -40.0, -40.0), (-2.0, 300.0, 300.0), op=SW.FILL, palette=1),
        SW.shape(S, (128.0, -30.0, 128.0), radius=8.0, op=SW.FILL, palette=2),
        SW.shape(C, (270.0, 270.0, 270.0), (290.0, 280.0, 275.0), radius=3.0, op=SW.PAINT, palette=3),
        SW.shape(S, (40.5, 50.5, 60.5), radius=0.0, op=SW.FILL, palette=4),                       # radius 0 on a centre: one voxel
        SW.shape(S, (40.25, 50.5, 60.5), radius=0.0, op=SW.FILL, palette=4),                      # ... off it: none
        SW.shape(C, (10.5, 10.5, 10.5), (14.5, 10.5, 10.5), radius=0.0, op=SW.PLACE, palette=5),
        SW.shape(B, (nan, 1.0, 1.0), (5.0, 5.0, 5.0), op=SW.CARVE), SW.shape(B, (1.0, 1.0, 1.0), (5.0, nan, 5.0), op=SW.CARVE),
        SW.shape(B, (-inf, 1.0, 1.0), (5.0, 5.0, 5.0), op=SW.CARVE), SW.shape(B, (1.0, 1.0, 1.0), (5.0, 5.0, inf), op=SW.CARVE),
        SW.shape(S, (inf, 5.0, 5.0), radius=2.0, op=SW.CARVE), SW.shape(S, (5.0, 5.0, 5.0), radius=nan, op=SW.CARVE),
        SW.shape(S, (5.0, 5.0, 5.0), radius=inf, op=SW.CARVE), SW.shape(C, (5.0, 5.0, 5.0), (9.0, -inf, 5.0), radius=1.0, op=SW.CARVE),
        SW.shape(S, (5.5, 5.5, 5.5), (nan, inf, -inf), radius=1.0, op=SW.CARVE),                  # a sphere ignores b
        SW.shape(B, (1.0, 1.0, 1.0), (5.0, 5.0, 5.0), radius=nan, op=SW.PAINT, palette=6),        # a box ignores its radius
        SW.shape(B, (10.5, 20.5, 30.5), (12.5, 22.5, 30.5), op=SW.FILL, palette=7),               # extent exactly on voxel centres
        SW.shape(B, (0.5, 0.5, 0.5), (255.5, 255.5, 255.5), op=SW.PAINT, palette=8),
        SW.shape(S, (100.5, 100.5, 100.5), radius=5.0, op=SW.FILL, palette=9),                    # voxels at distance exactly 5
        SW.shape(C, (20.5, 30.5, 40.5), (20.5, 38.5, 40.5), radius=2.0, op=SW.FILL, palette=10),
        SW.shape(B, (255.5, 255.5, 255.5), (255.5, 255.5, 255.5), op=SW.FILL, palette=11),
        SW.shape(B, (-0.5, 0.0, 0.0), (0.5, 0.5, 0.5), op=SW.FILL, palette=254),
        SW.shape(B, (-1e30,) * 3, (1e30,) * 3, op=SW.CARVE), SW.shape(B, (254.5, 254.5, 254.5), (1e30, 300.0, 256.0), op=SW.FILL, palette=22),
        SW.shape(S, (65536.0, 30.5, 30.5), radius=65281.0, op=SW.PLACE, palette=29),              # the coordinate limit: a disc on the x = 255 layer
        SW.shape(S, (65537.0, 30.5, 30.5), radius=65281.0, op=SW.PLACE, palette=29), SW.shape(S, (65.0, 65.0, 65.0), radius=65537.0, op=SW.CARVE),
        SW.shape(S, (65.0, 65.0, 65.0), radius=-1.0, op=SW.CARVE), SW.shape(B, (65.0, 60.0, 60.0), (64.0, 70.0, 70.0), op=SW.CARVE),
        SW.shape(C, (-20.0, 100.3, 30.1), (280.0, 110.2, 31.7), radius=1.7, op=SW.PLACE, palette=27),   # through two faces
        SW.shape(C, (80.5, 200.5, 80.5), (80.5 + 1e-20, 200.5, 80.5), radius=3.0, op=SW.FILL, palette=18))


def random_shapes(rng, n, lo, hi, size):
    a = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    kind = rng.integers(0, 3, n)
    b = a + np.where((kind == SW.BOX)[:, None], rng.uniform(0.0, size, (n, 3)), rng.uniform(-size, size, (n, 3))).astype(np.float32)
    return SW.shapes(*[SW.shape(int(k), p, q, radius=float(r), op=int(op), palette=int(pal)) for k, p, q, r, op, pal in
                       zip(kind, a, b, rng.uniform(0.0, size / 2, n), rng.integers(0, 4, n), rng.integers(0, 255, n))])


def test_device_shape_bounds_hold_the_witness_coverage(exe, tmp_path):
    rng = np.random.default_rng(43)
    shapes = np.concatenate([edge_shapes(), random_shapes(rng, 600, -30.0, 286.0, 20.0), random_shapes(rng, 60, 100.0, 156.0, 120.0)])
    r = run(exe, tmp_path, shapes=shapes)
    n_live = n_covering = 0
    for i, (s, got) in enumerate(zip(shapes, r["shapes"])):
        reg, m = SW.coverage(s)
        if not got["live"]:
            assert not m.any(), (i, s)
            continue
        n_live += 1
        d = got["d"]
        lo, hi = [(int(d["lo"]) >> (8 * k)) & 255 for k in range(3)], [(int(d["hi"]) >> (8 * k)) & 255 for k in range(3)]
        assert d["lo"] < 1 << 24 and d["hi"] < 1 << 24 and all(l <= h for l, h in zip(lo, hi)), (i, s, d)
        if m.any():
            n_covering += 1
            for k in range(3):
                along = np.nonzero(m.any(axis=tuple(a for a in range(3) if a != k)))[0] + reg[k].start
                assert lo[k] <= along.min() and along.max() <= hi[k], (i, s, d, k)
        # the operation as the two grid bytes (include/dust_hip.h: CARVE solid -> None; FILL every voxel -> palette; PAINT solid ->
        # palette, empty stays empty; PLACE empty -> palette, solid keeps its material -- 256 on the device)
        byte, op, kind = int(s["palette"]) + 1, int(s["op"]), int(s["kind"])
        want = {SW.CARVE: (0, 0), SW.FILL: (byte, byte), SW.PAINT: (byte, 0), SW.PLACE: (256, byte)}[op]
        assert (int(d["solid_to"]), int(d["empty_to"])) == want, (i, s, d)
        assert int(d["kind"]) == kind and d["a"].tobytes() == s["a"].tobytes()
        assert d["b"].tobytes() == (s["a"] if kind == SW.SPHERE else s["b"]).tobytes()
        assert d["radius"].tobytes() == (np.float32(0) if kind == SW.BOX else s["radius"]).tobytes()
    assert n_covering > 300 and len(shapes) - n_live > 30
    assert r["shapes"]["live"][:32].tolist() == [0, 0, 0, 0, 1, 1, 1] + [0] * 8 + [1] * 8 + [1, 1, 1, 0, 0, 0, 0, 1, 1]


def brute_force(bounds, c0, c1):
    """per root cell, ascending: the records c0..c1 whose bounds reach it (relative to c0, ascending); and the work items in record order"""
    per_cell, items = {}, []
    for i in range(c0, c1):
        lo, hi = [(int(bounds[i][0]) >> (8 * k)) & 255 for k in range(3)], [(int(bounds[i][1]) >> (8 * k)) & 255 for k in range(3)]
        for x in range(lo[0] >> 4, (hi[0] >> 4) + 1):
            for y in range(lo[1] >> 4, (hi[1] >> 4) + 1):
                for z in range(lo[2] >> 4, (hi[2] >> 4) + 1):
                    cell = x << 8 | y << 4 | z
                    per_cell.setdefault(cell, []).append(i - c0)
                    items.append((i - c0, cell))
    return per_cell, items


def test_chunks_cell_lists_and_work_items(exe, tmp_path):
    rng = np.random.default_rng(44)
    n = 150
    lo = rng.integers(0, 256, (n, 3))
    hi = np.minimum(lo + rng.choice([0, 3, 15, 16, 17, 40, 90], (n, 3)), 255)
    lo[5], hi[5] = (0, 0, 0), (255, 255, 255)           # one record alone is above every small limit
    lo[70:76], hi[70:76] = (16, 32, 48), (31, 47, 63)   # the same single cell six times
    bounds = np.stack([lo[:, 0] | lo[:, 1] << 8 | lo[:, 2] << 16, hi[:, 0] | hi[:, 1] << 8 | hi[:, 2] << 16], axis=1)
    configs = [(64, 65536), (64, 3), (1, 65536), (1000, 7), (1 << 21, 65536)]
    r = run(exe, tmp_path, bounds=bounds, configs=configs)
    cells_of = [len(brute_force(bounds, i, i + 1)[1]) for i in range(n)]
    assert cells_of[5] == 4096 and min(cells_of) == 1
    for (max_entries, max_records), chunks in zip(configs, r["chunks"]):
        c0 = 0
        for ch in chunks:
            c1 = ch["c1"]
            assert c0 < c1 <= n and c1 - c0 <= max_records
            assert sum(cells_of[c0:c1]) <= max_entries or c1 == c0 + 1
            if c1 < n and c1 - c0 < max_records:      # greedy: the next record would not have fitted
                assert sum(cells_of[c0:c1 + 1]) > max_entries
            per_cell, items = brute_force(bounds, c0, c1)
            assert ch["cells"].tolist() == sorted(per_cell)
            assert ch["starts"][0] == 0 and ch["starts"][-1] == len(ch["ids"]) == sum(cells_of[c0:c1])
            for k, cell in enumerate(ch["cells"].tolist()):
                assert ch["ids"][ch["starts"][k]:ch["starts"][k + 1]].tolist() == per_cell[cell], (c0, c1, cell)
            assert [tuple(int(v) for v in it) for it in ch["items"]] == items
            c0 = c1
        assert c0 == n
    assert [len(c) for c in r["chunks"]][-1] == 1 and len(r["chunks"][0]) > 5 and len(r["chunks"][2]) == n
    # the real limits: 512 whole-tree shapes fill 2^21 u16 entries, 256 whole-tree casts 2^20 work items
    assert r["shape_limit_end"] == 512 and r["cast_limit_end"] == 256


@functools.lru_cache(maxsize=None)
def decode_cases():
    """casts over two small random grids, the witness's hits, and per cast the device's result (best, acc) that those hits stand for"""
    rng = np.random.default_rng(45)
    src = np.zeros((256,) * 3, np.uint8)
    src[10:23, 12:21, 14:20] = rng.random((13, 9, 6)) < 0.4
    dst = np.zeros((256,) * 3, np.uint8)
    dst[0:64, 0:64, 0:64] = rng.random((64, 64, 64)) < 0.03
    dst[200:256, 200:256, 200:256] = rng.random((56, 56, 56)) < 0.03
    words = TW.all_orientations()
    steps = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
    n = 54
    base = rng.integers(-20, 70, (n, 3))
    base[n // 2:] += 190
    lo = rng.integers(9, 14, (n, 3))
    casts = CW.records(base, [steps[i % 27] for i in range(n)], rng.choice([0, 3, 60, 400, CW.MAX_STEPS], n), [words[(7 * i) % 48] for i in range(n)],
                       rng.integers(0, 2, n), lo, lo + rng.integers(-1, 11, (n, 3)))
    flip_x = TW.orient_word((0, 1, 2), (1, 0, 0))
    wrap = CW.records([(I32_MAX - 2, 5, 5), (I32_MAX, I32_MAX, 5), (I32_MIN, 5, 5), (I32_MAX - 70000, 5, 5)], [(0, 0, 0), (1, 1, 0), (-1, 0, 0), (1, 0, 0)],
                      [9, 9, 9, CW.MAX_STEPS], [flip_x, flip_x, TW.IDENTITY, flip_x], CW.WALLS, (10, 12, 14), (22, 20, 19))
    casts = np.concatenate([casts, wrap])
    hits = CW.cast(dst, src, casts)
    cases = np.zeros(len(casts), DECODE)
    cases["cast"], cases["voxels"], cases["contacts"] = casts, hits["voxels"], hits["contacts"]
    cases["wall"] = (hits["flags"] & CW.HIT_WALL) != 0
    k = np.where(hits["flags"] & CW.OVERLAP, np.uint64(0), hits["steps"].astype(np.uint64) + np.uint64(1))
    cases["best"] = np.where(hits["flags"] & CW.HIT, (k << np.uint64(24)) | hits["src_key"].astype(np.uint64), np.uint64(NO_HIT))
    return cases, hits


def test_cast_hits_are_the_witness_records(exe, tmp_path):
    cases, want = decode_cases()
    got = run(exe, tmp_path, decode=cases)["hits"]
    for i in range(len(cases)):
        assert got[i].tobytes() == want[i].tobytes(), (i, cases[i], got[i], want[i])
    flags = want["flags"]
    assert np.count_nonzero(flags == 0) > 5 and np.count_nonzero(flags & CW.OVERLAP) > 5 and np.count_nonzero(flags & (CW.HIT | CW.OVERLAP) == CW.HIT) > 5
    assert np.count_nonzero(want["voxels"] == 0) > 0 and np.count_nonzero(flags & CW.HIT_WALL) > 3
    # a contact past the int32 range comes back as its low 32 bits: INT32_MAX - 2 + (22 - 10) wraps to INT32_MIN + 9
    assert want["contact"][54][0] == I32_MIN + 9 and want["contact"][55][0] < 0 and want["contact"][56][0] == I32_MIN
