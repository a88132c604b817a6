"""dust_amd/csrc/neighbour_rule.hpp (neighbour_plane, neighbour_count, neighbour_change, with surface_rule.hpp's region mask) and the
neighbours records of dust_amd/csrc/model_records.hpp (device_neighbours, neighbours_apply_arguments, neighbours_result,
neighbours_applied) run as native code on a CPU: tests/cpp/neighbour_rule_test.cpp compiled with g++ under AddressSanitizer and UBSan
into a program of its own, fed bricks on stdin and held to the witness (tests/neighbour_witness.py), which sees the same 27 words as a
12^3 grid with the brick in its middle: one set bit in each of the 27 words in turn, at the eight brick corners and an interior bit
(every offset across every face, edge and corner of a brick), all words full, a full brick alone and inside walls, random words at
three densities, regions that cut the brick on each axis, the three neighbourhoods throughout, and the validation table."""
import os
import subprocess

import numpy as np
import pytest

import neighbour_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "neighbour_rule_test.cpp")
FULL = (1 << 64) - 1
CAVE = {W.FACES: (W.count_mask(1, (4, 6)), W.count_mask((2, 6))), W.EDGES: (W.count_mask((7, 18)), W.count_mask((5, 18))),
        W.CORNERS: (W.count_mask((14, 26)), W.count_mask((13, 26)))}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("neighbour_rule") / "neighbour_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def grid_of(words):
    """27 words, index (dx + 1) * 9 + (dy + 1) * 3 + dz + 1 -> the 12^3 boolean grid they are the bricks of"""
    grid = np.zeros((12, 12, 12), np.uint8)
    for i, word in enumerate(words):
        bits = np.array([(word >> b) & 1 for b in range(64)], np.uint8).reshape(4, 4, 4)         # bit x << 4 | y << 2 | z
        bx, by, bz = i // 9, (i // 3) % 3, i % 3
        grid[4 * bx:4 * bx + 4, 4 * by:4 * by + 4, 4 * bz:4 * bz + 4] = bits
    return grid


def word_of(mask):
    """a (4, 4, 4) boolean array -> the brick word"""
    return sum(1 << b for b in np.flatnonzero(mask.reshape(64)).tolist())


def check(exe, cases):
    """cases: (words, neighbourhood, birth, survive, lo, hi) with lo / hi relative to the 12^3 grid, the brick at (1, 1, 1); each held
    to the witness on that grid. Returns the counts seen, per case a (4, 4, 4) array"""
    got = run(exe, ["c " + " ".join(str(v) for v in (nb, birth, survive) + tuple(lo) + tuple(hi) + (1, 1, 1) + tuple(words)) for words, nb, birth, survive, lo, hi in cases])
    seen = []
    for (words, nb, birth, survive, lo, hi), row in zip(cases, got):
        grid = grid_of(words)
        planes, born, died, region = row[:5], row[5], row[6], row[7]
        n = np.array([sum(((planes[k] >> b) & 1) << k for k in range(5)) for b in range(64)]).reshape(4, 4, 4)
        assert np.array_equal(n, W.counts_in(grid, nb, (4, 4, 4), (7, 7, 7))), (nb, words)
        inside = np.zeros((12, 12, 12), bool)
        inside[tuple(slice(l, h + 1) for l, h in zip(lo, hi))] = True
        assert region == word_of(inside[4:8, 4:8, 4:8]), (lo, hi)
        cut = tuple(max(l, 4) for l in lo), tuple(min(h, 7) for h in hi)                          # the region inside the brick
        after = W.step(grid, nb, birth, survive, region=cut)[0] if all(l <= h for l, h in zip(*cut)) else grid
        assert born == word_of(((after != 0) & (grid == 0))[4:8, 4:8, 4:8]) and died == word_of(((after == 0) & (grid != 0))[4:8, 4:8, 4:8]), (nb, lo, hi)
        assert not ((after != 0) ^ (grid != 0))[~inside].any()
        seen.append(n)
    return seen


def test_one_bit_in_each_word_crosses_every_face_edge_and_corner(exe):
    bits = [(x << 4) | (y << 2) | z for x in (0, 3) for y in (0, 3) for z in (0, 3)] + [(1 << 4) | (2 << 2) | 1]
    for nb in W.NEIGHBOURHOODS:
        cases = []
        for i in range(27):
            for bit in bits:
                words = [0] * 27
                words[i] = 1 << bit
                cases.append((words, nb, *CAVE[nb], (0, 0, 0), (11, 11, 11)))
        seen = check(exe, cases)
        total = np.sum(seen, axis=0)
        # a brick corner voxel of the brick itself is seen by its 7 (3, 6) neighbours inside the brick; the interior bit by all of its own
        assert int(np.sum([n.sum() for n in seen[13 * 9:13 * 9 + 8]])) == 8 * {W.FACES: 3, W.EDGES: 6, W.CORNERS: 7}[nb]
        assert int(seen[13 * 9 + 8].sum()) == nb and total.max() > 0
        # every offset across every face, edge and corner of the brick: each neighbour brick's facing corner bit reaches the brick
        reached = [int(np.sum([n.sum() for n in seen[i * 9:i * 9 + 8]])) for i in range(27)]
        order = [sum(c != 1 for c in (i // 9, (i // 3) % 3, i % 3)) for i in range(27)]
        for i in range(27):
            if i != 13:
                assert (reached[i] > 0) == (order[i] <= {W.FACES: 1, W.EDGES: 2, W.CORNERS: 3}[nb]), (nb, i)


def test_full_words_and_walls(exe):
    for nb in W.NEIGHBOURHOODS:
        everything = check(exe, [([FULL] * 27, nb, *CAVE[nb], (0, 0, 0), (11, 11, 11))])[0]
        assert np.all(everything == nb)
        alone = [0] * 27
        alone[13] = FULL
        n = check(exe, [(alone, nb, *CAVE[nb], (0, 0, 0), (11, 11, 11))])[0]
        corner, inner = {W.FACES: (3, 6), W.EDGES: (6, 18), W.CORNERS: (7, 26)}[nb]
        assert n[0, 0, 0] == n[3, 3, 3] == n[0, 3, 0] == corner and n[1, 2, 1] == inner
        # the all-ones substitution of WALLS is the first case again: the witness sees a 4^3 tree inside walls
        walled = W.counts_in(grid_of(alone)[4:8, 4:8, 4:8], nb, (0, 0, 0), (3, 3, 3), walls=True)
        assert np.array_equal(walled, everything)
        empty_in_walls = [FULL] * 27
        empty_in_walls[13] = 0
        n = check(exe, [(empty_in_walls, nb, *CAVE[nb], (0, 0, 0), (11, 11, 11))])[0]
        assert np.array_equal(n, W.counts_in(np.zeros((4, 4, 4), np.uint8), nb, (0, 0, 0), (3, 3, 3), walls=True)) and n[1, 1, 1] == 0 and n[0, 0, 0] == nb - corner


@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
def test_random_words_and_regions(exe, density):
    rng = np.random.default_rng(int(density * 100))
    regions = [((0, 0, 0), (11, 11, 11)), ((5, 0, 0), (6, 11, 11)), ((0, 4, 0), (11, 4, 11)), ((0, 0, 6), (11, 11, 7)), ((5, 6, 7), (5, 6, 7)), ((6, 5, 4), (11, 6, 6)),
               ((0, 0, 0), (3, 11, 11)), ((8, 8, 8), (11, 11, 11)), ((4, 4, 4), (7, 7, 7))]
    changed = 0
    for nb in W.NEIGHBOURHOODS:
        cases = []
        for k in range(40):
            words = [word_of(rng.random((4, 4, 4)) < density) for _ in range(27)]
            birth, survive = CAVE[nb] if k % 2 else (int(rng.integers(0, 2 << nb)), int(rng.integers(0, 2 << nb)))
            cases.append((words, nb, birth, survive, *regions[k % len(regions)]))
        check(exe, cases)
        rows = run(exe, ["c " + " ".join(str(v) for v in (nb, b, s) + tuple(lo) + tuple(hi) + (1, 1, 1) + tuple(w)) for w, nb, b, s, lo, hi in cases])
        changed += sum(bin(r[5]).count("1") + bin(r[6]).count("1") for r in rows)
    assert changed > 100


def test_query_validation_table_and_clipping(exe):
    queries = [(nb, flags, palette, birth, survive, lo, hi)
               for nb in (0, 5, 6, 7, 18, 26, 27, 0xFFFFFFFF) for flags in (0, 1, 2, 3, 4, 1 << 31) for palette in (-1, 0, 254, 255)
               for birth, survive in ((0, 0), (0x7F, 0x7F), (0x80, 0), (0, 1 << 18), (1 << 19, 0), (0, (1 << 27) - 1), (1 << 27, 0))
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((17, 3, 250), (40, 3, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 255, 1)), ((3, 2, 1), (30, 20, 256)))]
    got = run(exe, ["q " + " ".join(str(v) for v in (nb, flags, palette, birth, survive) + lo + hi) for nb, flags, palette, birth, survive, lo, hi in queries])
    accepted = 0
    for (nb, flags, palette, birth, survive, lo, hi), row in zip(queries, got):
        if W.refused(nb, flags, palette, birth, survive, lo, hi):
            assert row == [0], (nb, flags, palette, birth, survive, lo, hi)
            continue
        accepted += 1
        empty = any(l > h for l, h in zip(lo, hi))
        assert row[:8] == [1, int(empty), nb, flags & 1, birth, survive, palette + 1, (flags >> 1) & 1]
        if empty:
            assert len(row) == 8
        else:
            assert row[8:] == list(lo) + list(hi) + [c >> 4 for c in lo] + [c >> 4 for c in hi]
    assert accepted == (2 + 4 + 6) * 4 * 2 * 3        # per neighbourhood the mask pairs it takes; flags 0..3; two palettes; three regions
    got = run(exe, [f"a {g}" for g in (0, 1, 8, 256, 257, 0xFFFFFFFF)])
    assert [row[0] for row in got] == [0, 1, 1, 1, 0, 0] == [int(not W.refused(6, generations=g)) for g in (0, 1, 8, 256, 257, 0xFFFFFFFF)]


def test_result_records(exe):
    acc = [4096, 1000, 30, 40, 255 - 3, 255 - 0, 255 - 200, 9, 255, 201]
    got = run(exe, ["r", "r " + " ".join(str(v) for v in acc), "r 64 5 0 0 0 0 0 0 0 0"])
    zero = W.zero_result()
    assert got[0] == [0, 0, 0, 0] + zero["lo"].tolist() + zero["hi"].tolist() + [0]
    assert got[1] == [4096, 1000, 30, 40, 3, 0, 200, 9, 255, 201, 0]
    assert got[2] == [64, 5, 0, 0, 255, 255, 255, 0, 0, 0, 0]                     # voxels, nothing would change: the zero result's bounds
    # an apply: three generations that change something, then a fixed point; the rows after it are 0
    slots = [5, 1, 255 - 10, 255 - 20, 255 - 30, 12, 22, 32] + [0, 2, 255 - 9, 255 - 25, 255 - 30, 9, 25, 30] + [1, 0, 255 - 40, 255 - 1, 255 - 31, 40, 1, 31] + [0] * 16
    got = run(exe, ["p 5", "p 5 100 " + " ".join(str(v) for v in slots), "p 2 7 " + " ".join(["0"] * 16),
                    "p 256 0 " + " ".join(" ".join(str(v) for v in [1 << 24, 1 << 24, 255, 255, 255, 255, 255, 255]) for _ in range(256))])
    zero = W.zero_applied()
    assert got[0] == [0, 0, 0, 0, 0] + zero["lo"].tolist() + zero["hi"].tolist() + [0] + [0] * 10
    assert got[1] == [3, 100, 103, 6, 3, 9, 1, 30, 40, 25, 32, 0] + [5, 1, 0, 2, 1, 0, 0, 0, 0, 0]
    assert got[2] == [0, 7, 7, 0, 0, 255, 255, 255, 0, 0, 0, 0, 0, 0, 0, 0]
    assert got[3][:12] == [256, 0, 0, 1 << 32, 1 << 32, 0, 0, 0, 255, 255, 255, 0] and got[3][12:] == [1 << 24] * 512      # sums past 32 bits
