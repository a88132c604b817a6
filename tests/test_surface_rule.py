"""dust_amd/csrc/surface_rule.hpp (surface_exposure, surface_region_mask) and the surface records of dust_amd/csrc/model_records.hpp
(device_surface, surface_result) run as native code on a CPU: tests/cpp/surface_rule_test.cpp compiled with g++ under AddressSanitizer
and UBSan into a program of its own, fed brick words on stdin and held to the witness (tests/surface_witness.py) on random 12^3 blocks
-- three bricks per axis, so the centre brick has all six neighbours and every other one some face off the block, with and without
WALLS --, on the all-ones and all-zero words, on regions that cut through bricks and on the query validation table."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import surface_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "surface_rule_test.cpp")
ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("surface_rule") / "surface_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def brick_word(flags):
    """a 4^3 boolean cube -> its word: bit x << 4 | y << 2 | z"""
    return sum(1 << ((x << 4) | (y << 2) | z) for x, y, z in np.argwhere(flags).tolist())


def words_of(block):
    """a 12^3 array of flags -> {(bx, by, bz): word}"""
    return {b: brick_word(block[4 * b[0]:4 * b[0] + 4, 4 * b[1]:4 * b[1] + 4, 4 * b[2]:4 * b[2] + 4]) for b in itertools.product(range(3), repeat=3)}


def exposure_lines(words, walls):
    off = ONES if walls else 0
    return [f"e {words[b]} " + " ".join(str(words.get((b[0] + sx, b[1] + sy, b[2] + sz), off)) for sx, sy, sz in W.STEPS) for b in sorted(words)]


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_random_blocks_against_the_witness(exe, density):
    rng = np.random.default_rng(int(density * 100))
    for walls in (False, True):
        grid = np.where(rng.random((12,) * 3) < density, rng.integers(1, 4, (12,) * 3), 0).astype(np.uint8)
        words = words_of(grid != 0)
        got = run(exe, exposure_lines(words, walls))
        exposed = W.exposure(grid, walls)
        for b, row in zip(sorted(words), got):
            cube = exposed[4 * b[0]:4 * b[0] + 4, 4 * b[1]:4 * b[1] + 4, 4 * b[2]:4 * b[2] + 4]
            assert row == [brick_word((cube >> d) & 1 == 1) for d in range(6)], (b, walls)
        assert any(any(row) for row in got)


def test_all_ones_and_all_zero_words(exe):
    planes = [brick_word(np.indices((4, 4, 4))[axis] == at) for axis, at in ((0, 0), (0, 3), (1, 0), (1, 3), (2, 0), (2, 3))]
    lines = ["e 0 0 0 0 0 0 0", f"e 0 {ONES} {ONES} {ONES} {ONES} {ONES} {ONES}",        # an empty brick shows nothing, whatever is around it
             f"e {ONES} 0 0 0 0 0 0",                                                      # a full brick alone: its six boundary planes
             f"e {ONES} {ONES} {ONES} {ONES} {ONES} {ONES} {ONES}",                          # ... buried (or at a corner of the tree under WALLS)
             f"e {ONES} {ONES} 0 {ONES} 0 {ONES} 0"]                                        # ... with the three positive neighbours missing
    got = run(exe, lines)
    assert got[0] == got[1] == got[3] == [0] * 6
    assert got[2] == planes and got[4] == [0, planes[1], 0, planes[3], 0, planes[5]]
    assert [bin(p).count("1") for p in planes] == [16] * 6
    # a neighbour's voxel hides exactly the one voxel it touches: each boundary voxel against its mirror in the neighbour
    for d, (sx, sy, sz) in enumerate(W.STEPS):
        cases = []
        for x, y, z in itertools.product(range(4), repeat=3):
            if not all(0 <= c < 4 for c in (x + sx, y + sy, z + sz)):
                cases.append(((x << 4) | (y << 2) | z, ((x + sx) % 4 << 4) | ((y + sy) % 4 << 2) | (z + sz) % 4))
        assert len(cases) == 16
        rows = run(exe, ["e " + " ".join([str(ONES)] + [str(1 << theirs if k == d else 0) for k in range(6)]) for _, theirs in cases])
        for (mine, _), row in zip(cases, rows):
            assert row[d] == planes[d] & ~(1 << mine)


def test_region_masks_cut_through_bricks(exe):
    rng = np.random.default_rng(92)
    cases = [((0, 0, 0), (0, 0, 0), (255, 255, 255)), ((63, 63, 63), (255, 255, 255), (255, 255, 255)), ((1, 2, 3), (5, 9, 14), (6, 11, 14)),
             ((1, 2, 3), (8, 0, 0), (255, 255, 255)), ((1, 2, 3), (0, 0, 0), (3, 255, 255))]
    for _ in range(60):
        lo = rng.integers(0, 40, 3)
        hi = lo + rng.integers(0, 12, 3)
        cases.append((tuple(int(v) for v in rng.integers(0, 12, 3)), tuple(int(v) for v in lo), tuple(int(v) for v in hi)))
    got = run(exe, ["m " + " ".join(str(v) for v in b + lo + hi) for b, lo, hi in cases])
    seen = set()
    for (b, lo, hi), (mask,) in zip(cases, got):
        inside = np.zeros((4, 4, 4), bool)
        for x, y, z in itertools.product(range(4), repeat=3):
            inside[x, y, z] = all(lo[r] <= 4 * b[r] + c <= hi[r] for r, c in enumerate((x, y, z)))
        assert mask == brick_word(inside), (b, lo, hi)
        seen.add(0 if mask == 0 else 2 if mask == ONES else 1)
    assert seen == {0, 1, 2}


def test_query_validation_table_and_clipping(exe):
    queries = [(faces, flags, palette, lo, hi)
               for faces in (0, 1, 8, 63, 64, 0xFFFFFFFF) for flags in (0, 1, 2, 1 << 31) for palette in (-2, -1, 0, 254, 255)
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((17, 3, 250), (40, 3, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 4000)))]
    got = run(exe, ["q " + " ".join(str(v) for v in (faces, flags, palette) + lo + hi) for faces, flags, palette, lo, hi in queries])
    accepted = 0
    for (faces, flags, palette, lo, hi), row in zip(queries, got):
        if W.refused(faces, flags, palette, lo, hi):
            assert row == [0], (faces, flags, palette, lo, hi)
            continue
        accepted += 1
        empty = any(l > h for l, h in zip(lo, hi))
        assert row[:5] == [1, int(empty), faces, flags & 1, palette + 1]
        if empty:
            assert len(row) == 5
        else:
            assert row[5:] == list(lo) + list(hi) + [v >> 4 for v in lo] + [v >> 4 for v in hi]
    assert 0 < accepted < len(queries)


def test_result_record(exe):
    acc = [10, 1, 2, 3, 4, 5, 6, 77, 255 - 3, 255 - 0, 255 - 200, 9, 255, 201]
    got = run(exe, ["r", "r " + " ".join(str(v) for v in acc), "r " + " ".join(["0"] * 7 + ["5"] + ["0"] * 6)])
    zero = W.zero_result()
    assert got[0] == [0, 0] + [0] * 6 + [0] + zero["lo"].tolist() + zero["hi"].tolist() + [0]
    assert got[1] == [10, 21, 1, 2, 3, 4, 5, 6, 77, 3, 0, 200, 9, 255, 201, 0]
    assert got[2] == [0, 0] + [0] * 6 + [5, 255, 255, 255, 0, 0, 0, 0]      # solid voxels, none listed: the bounds of the zero result
