"""dust_amd/csrc/boxes_rule.hpp (the functions the kernels of boxes.hip run) and the boxes records of dust_amd/csrc/model_records.hpp
(device_boxes, boxes_result) run as native code on a CPU: tests/cpp/boxes_rule_test.cpp compiled with g++ under AddressSanitizer and
UBSan into a program of its own, fed bit planes on stdin and held to the witness (tests/boxes_witness.py): a pair of slices is handed
to the witness as a two-voxel-thick slab stacked along x, where v is y and u is z."""
import os
import subprocess

import numpy as np
import pytest

import boxes_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "boxes_rule_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("boxes_rule") / "boxes_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr)
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def words(bits):
    """rows of 256 flags -> rows of eight 32-bit words, bit u & 31 of word u >> 5"""
    return np.packbits(np.asarray(bits, bool), axis=-1, bitorder="little").view("<u4")


def planes(slab, any_palette):
    """F, J, K of a slab[v, u] of bytes (0: the voxel is not in S), from their definitions"""
    f = slab != 0
    j, k = np.zeros_like(f), np.zeros_like(f)
    j[:, 1:] = f[:, 1:] & f[:, :-1] & (any_palette | (slab[:, 1:] == slab[:, :-1]))
    k[1:] = f[1:] & f[:-1] & (any_palette | (slab[1:] == slab[:-1]))
    return f, j, k


def pair_lines(before, slab, any_palette, stride):
    same = np.ones(slab.shape, bool) if any_palette else slab == before
    rows = np.concatenate([words(p) for p in planes(slab, any_palette) + planes(before, any_palette) + (same,)], axis=1)
    return [f"pair {len(slab)} {stride}"] + [" ".join(str(v) for v in row) for row in rows]


def witness_rects(before, slab, any_palette):
    """[v0, u0, u1, v1, d] per rect of the second slice, row by row: d, the rect is the second slice of a box"""
    grid = np.zeros((2, 256, 256), np.uint8)
    grid[0, :len(before)], grid[1, :len(slab)] = before, slab
    _, rects, boxes = W.decompose(grid, axis=0, any_palette=any_palette)
    stacked = {(v0, u0) for s0, s1, v0, u0 in zip(*(boxes[k].tolist() for k in ("s0", "s1", "v0", "u0"))) if (s0, s1) == (0, 1)}
    mine = [(v0, u0, u1, v1) for s, v0, u0, u1, v1 in zip(*(rects[k].tolist() for k in ("s", "v0", "u0", "u1", "v1"))) if s == 1]
    return [[v0, u0, u1, v1, int((v0, u0) in stacked)] for v0, u0, u1, v1 in sorted(mine)]


def check_pair(exe, before, slab, any_palette, stride=8):
    want = witness_rects(before, slab, any_palette)
    got = run(exe, pair_lines(before, slab, any_palette, stride))
    assert got[-1] == [len(want), sum(r[4] for r in want)], (got[-1], len(want))
    assert got[:-1] == want, [(g, w) for g, w in zip(got[:-1], want) if g != w][:3]
    return want


@pytest.mark.parametrize("density", [0.5, 0.9, 0.97])
def test_random_slice_pairs_against_the_witness(exe, density):
    rng = np.random.default_rng(int(density * 100) + 1)
    stacked = single = 0
    for materials, rows, stride in ((1, 256, 8), (3, 256, 9), (2, 37, 8)):
        slab = np.where(rng.random((rows, 256)) < density, rng.integers(1, materials + 1, (rows, 256)), 0).astype(np.uint8)
        # the slice before: the same slice with a voxel in 300 drawn again, so that most rects continue and some do not
        again = rng.random(slab.shape) < 1 / 300
        before = np.where(again, np.where(rng.random(slab.shape) < density, rng.integers(1, materials + 1, slab.shape), 0), slab).astype(np.uint8)
        unrelated = np.where(rng.random((rows, 256)) < density, rng.integers(1, materials + 1, (rows, 256)), 0).astype(np.uint8)
        for any_palette in (False, True):
            want = check_pair(exe, before, slab, any_palette, stride)
            stacked += sum(r[4] for r in want)
            single += sum(1 - r[4] for r in want)
            check_pair(exe, unrelated, slab, any_palette, stride)
            check_pair(exe, np.zeros_like(slab), slab, any_palette, stride)         # nothing before: D is clear
    assert stacked > 100 and single > 100


def test_d_word_at_word_edges_and_first_and_last_rows(exe):
    slab = np.zeros((256, 256), np.uint8)
    slab[0, 0:32] = 1                                                            # row 0, ends at bit 31
    slab[2, 31:33] = 1                                                           # starts at 31, crosses 31 | 32
    slab[4:6, 32:64] = 1                                                         # starts at bit 0 of a word, ends at 63
    slab[8, 20:32], slab[10, 20:32], slab[12:14, 20:32] = 1, 1, 1                # (their partners differ below)
    slab[16:18, 100:110] = 2
    slab[20:23, 60:70] = 1
    slab[255, 224:256] = 3                                                       # the last row, the last word
    slab[254, 0] = 1
    slab[30, :] = 1                                                              # a whole row
    before = slab.copy()
    before[8, 20:33] = 1                                                         # a longer u1 over the same corner
    before[10:12, 20:32] = 1                                                     # a taller v1
    before[12, 20:32] = 0                                                        # the same u0 and u1 one row down: another v0
    before[16:18, 100:110] = 3                                                   # another material
    before[21, 65] = 0                                                           # the middle row lacks a voxel
    want = check_pair(exe, before, slab, False)
    for rect in ([0, 0, 31, 0, 1], [2, 31, 32, 2, 1], [4, 32, 63, 5, 1], [8, 20, 31, 8, 0], [10, 20, 31, 10, 0], [12, 20, 31, 13, 0], [16, 100, 109, 17, 0],
                 [20, 60, 69, 22, 0], [255, 224, 255, 255, 1], [254, 0, 0, 254, 1], [30, 0, 255, 30, 1]):
        assert rect in want, rect
    merged = check_pair(exe, before, slab, True, stride=9)
    assert [16, 100, 109, 17, 1] in merged and [8, 20, 31, 8, 0] in merged and [20, 60, 69, 22, 0] in merged
    # all ones over all ones: one rect, continued; over a plane of another material: not
    ones = np.ones((256, 256), np.uint8)
    assert check_pair(exe, ones, ones, False) == [[0, 0, 255, 255, 1]]
    assert check_pair(exe, ones * 2, ones, False, stride=9) == [[0, 0, 255, 255, 0]]
    assert check_pair(exe, ones * 2, ones, True) == [[0, 0, 255, 255, 1]]
    stripes = np.tile(np.array([1, 2], np.uint8), (256, 128))                    # every run one bit long, every rect 256 high
    assert check_pair(exe, stripes, stripes, False) == [[0, u, u, 255, 1] for u in range(256)]
    shifted = np.roll(stripes, 1, axis=1)
    assert check_pair(exe, shifted, stripes, False) == [[0, u, u, 255, 0] for u in range(256)]


@pytest.mark.parametrize("any_palette", [False, True])
def test_whole_stacks_against_the_witness(exe, any_palette):
    """the two passes in the kernels' order over several slices: D of every slice, then the box starts with their depths"""
    rng = np.random.default_rng(12 + any_palette)
    rows = 48
    block = np.zeros((9, rows, 256), np.uint8)
    layer = np.where(rng.random((rows, 256)) < 0.9, rng.integers(1, 3, (rows, 256)), 0).astype(np.uint8)
    for s in range(9):
        if s != 4:                                                               # slice 4 stays empty: its D plane must still be written
            again = rng.random(layer.shape) < 1 / 400
            layer = np.where(again, np.where(rng.random(layer.shape) < 0.9, rng.integers(1, 3, layer.shape), 0), layer).astype(np.uint8)
            block[s] = layer
    lines = [f"stack {len(block)} {rows}"]
    for s in range(len(block)):
        same = np.ones(block[s].shape, bool) if any_palette or s == 0 else block[s] == block[s - 1]
        planes_ = np.concatenate([words(p) for p in planes(block[s], any_palette) + (same,)], axis=1)
        lines += [" ".join(str(v) for v in row) for row in planes_]
    got = run(exe, lines)
    grid = np.zeros((len(block), 256, 256), np.uint8)
    grid[:, :rows] = block
    _, _, boxes = W.decompose(grid, axis=0, any_palette=any_palette)
    want = [list(b) for b in zip(*(boxes[k].tolist() for k in ("s0", "v0", "u0", "u1", "v1")), (boxes["s1"] - boxes["s0"] + 1).tolist())]
    assert got[-1] == [len(want)] and got[:-1] == want, [(g, w) for g, w in zip(got[:-1], want) if g != w][:3]
    depths = [b[5] for b in want]
    assert max(depths) == 4 and sum(d > 1 for d in depths) > 100 and not any(b[0] <= 4 < b[0] + b[5] for b in want)     # nothing crosses the empty slice


def test_depth_walk_over_a_hand_made_volume(exe):
    def depth(last, s, v0, u0, bits):
        return f"depth {last} {s} {v0} {u0} {len(bits)} " + " ".join(f"{t} {v} {u}" for t, v, u in bits)
    column = [(t, 7, 33) for t in range(256)]
    cases = [(depth(255, 0, 7, 33, []), 1),                                       # nothing continues
             (depth(255, 0, 7, 33, column), 256),                                 # the whole axis
             (depth(100, 0, 7, 33, column[:101]), 101),                                 # the region's last slice stops the walk (the volume ends there)
             (depth(100, 100, 7, 33, column[:101]), 1),                                # a start in the last slice reads no plane
             (depth(255, 3, 7, 33, [(4, 7, 33), (5, 7, 33), (7, 7, 33)]), 3),     # a gap stops it
             (depth(255, 3, 7, 33, [(4, 7, 32), (4, 7, 34), (4, 6, 33), (4, 8, 33), (3, 7, 33)]), 1),   # the neighbours' bits and its own slice's are not its
             (depth(255, 10, 0, 0, [(11, 0, 0), (12, 0, 0)]), 3), (depth(255, 10, 255, 255, [(11, 255, 255)]), 2),
             (depth(255, 10, 0, 31, [(11, 0, 31), (12, 0, 32)]), 2), (depth(255, 10, 0, 32, [(11, 0, 32), (12, 0, 31)]), 2),
             (depth(0, 0, 5, 5, []), 1)]
    got = run(exe, [line for line, _ in cases])
    assert [row[0] for row in got] == [want for _, want in cases]


def test_records_for_all_three_axes(exe):
    boxes = np.zeros(5, W.BOX_DTYPE)
    # n, s, u0, u1, v0, v1, depth, palette: n = x: u = z, v = y; n = y: u = z, v = x; n = z: u = y, v = x
    boxes[0] = ((7 << 16) | (200 << 8) | 100, 254, 9, 55, 155)
    boxes[1] = ((200 << 16) | (7 << 8) | 100, 0, 55, 9, 155)
    boxes[2] = ((200 << 16) | (100 << 8) | 7, 3, 55, 155, 9)
    boxes[3] = (0, 17, 255, 255, 255)
    boxes[4] = ((255 << 16) | (255 << 8) | 255, 1, 0, 0, 0)
    got = run(exe, ["c 0 7 100 255 200 255 10 254", "c 1 7 100 255 200 255 10 0", "c 2 7 100 255 200 255 10 3", "c 1 0 0 255 0 255 256 17", "c 2 255 255 255 255 255 1 1"])
    assert [row[0] for row in got] == boxes.view("<u8").tolist()
    # the witness writes the same records: a box 10 x 56 x 156 at (7, 200, 100), seen along every axis
    grid = np.zeros((256, 256, 256), np.uint8)
    grid[7:17, 200:256, 100:256] = 255
    for axis in range(3):
        assert W.boxes(grid, axis=axis)[1].tobytes() == boxes[:1].tobytes()


def test_query_validation_table_and_clipping(exe):
    queries = [(axis, flags, palette, lo, hi)
               for axis in (0, 1, 2, 3, 63, 0xFFFFFFFF) for flags in (0, 1, 2, 3, 4, 1 << 31) for palette in (-2, -1, 0, 254, 255)
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((17, 3, 250), (40, 3, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 4000)))]
    got = run(exe, ["m " + " ".join(str(v) for v in (axis, flags, palette) + lo + hi) for axis, flags, palette, lo, hi in queries])
    accepted = 0
    for (axis, flags, palette, lo, hi), row in zip(queries, got):
        if W.refused(axis, flags, palette, lo, hi):
            assert row == [0], (axis, flags, palette, lo, hi)
            continue
        accepted += 1
        empty = any(l > h for l, h in zip(lo, hi))
        assert row[:5] == [1, int(empty), axis, palette + 1, flags & 1]
        assert row[5:] == ([] if empty else list(lo) + list(hi))
    assert 0 < accepted < len(queries)


def test_result_record(exe):
    acc = [50, 20, 7000, 255 - 3, 255 - 0, 255 - 250, 9, 255, 251]
    got = run(exe, ["r", "r " + " ".join(str(v) for v in acc), "r 0 0 0 0 0 0 0 0 0"])
    zero = W.zero_result()
    assert got[0] == [0, 0, 0, 255, 255, 255, 0, 0, 0, 0, 0] + [0] * 11 == got[2]   # nothing looked at, or nothing found: bounds 255 / 0
    assert zero.tobytes() == np.array([tuple(got[0][:3]) + (got[0][3:6], 0, got[0][7:10], 0, [0] * 11)], W.RESULT_DTYPE).tobytes()
    assert got[1] == [30, 50, 7000, 3, 0, 250, 0, 9, 255, 251, 0] + [0] * 11
