"""dust_amd/csrc/delta_rule.hpp (delta_words, delta_listed) and the delta records of dust_amd/csrc/model_records.hpp (device_delta,
delta_result, delta_apply_records) run as native code on a CPU: tests/cpp/delta_rule_test.cpp compiled with g++ under AddressSanitizer
and UBSan into a program of its own, fed brick-word pairs on stdin and held to the witness (tests/delta_witness.py) on random 12^3
blocks, on the all-ones and all-zero words, on regions that cut through bricks, on every `kinds` value 1..7 and on the validation table."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import delta_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "delta_rule_test.cpp")
ONES = (1 << 64) - 1
BRICKS = list(itertools.product(range(3), repeat=3))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("delta_rule") / "delta_rule_test")
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


def cube(block, b):
    return block[4 * b[0]:4 * b[0] + 4, 4 * b[1]:4 * b[1] + 4, 4 * b[2]:4 * b[2] + 4]


def pair(seed, density):
    rng = np.random.default_rng(seed)
    before = np.where(rng.random((12,) * 3) < density, rng.integers(1, 4, (12,) * 3), 0).astype(np.uint8)
    fresh = np.where(rng.random((12,) * 3) < density, rng.integers(1, 4, (12,) * 3), 0).astype(np.uint8)
    return before, np.where(rng.random((12,) * 3) < 0.5, fresh, before).astype(np.uint8)


def brick_lines(before, after, kinds, palette, lo, hi):
    """one request per brick of a 12^3 pair: the two words, and the two ballots the kernel takes from the grid bytes"""
    lines = []
    for b in BRICKS:
        a, c = cube(before, b), cube(after, b)
        keep = np.ones((4,) * 3, bool) if palette < 0 else (a == palette + 1) | (c == palette + 1)
        lines.append(f"w {brick_word(a != 0)} {brick_word(c != 0)} " + " ".join(str(v) for v in b + lo + hi) + f" {kinds} {brick_word(a != c)} {brick_word(keep)}")
    return lines


def check_pair(exe, before, after, kinds, palette, region):
    """the rule's words, brick by brick, against the witness's list of the same pair"""
    lo, hi = region
    rows = run(exe, brick_lines(before, after, kinds, palette, lo, hi))
    result, voxels, _ = W.delta(before, after, kinds, palette, region)
    key = voxels["key"].astype(np.int64)
    x, y, z = key >> 16, (key >> 8) & 255, key & 255
    box = tuple(slice(l, min(h, 11) + 1) for l, h in zip(lo, hi))
    inside = np.zeros((12,) * 3, bool)
    inside[box] = True
    total = 0
    for b, (solid_before, solid_after, added, removed, candidates, l_added, l_removed, l_repainted, listed) in zip(BRICKS, rows):
        mine = (x // 4 == b[0]) & (y // 4 == b[1]) & (z // 4 == b[2])
        bits = ((x[mine] % 4) << 4) | ((y[mine] % 4) << 2) | (z[mine] % 4)
        for word, bit in ((l_added, W.ADDED), (l_removed, W.REMOVED), (l_repainted, W.REPAINTED)):
            assert word == sum(1 << int(v) for v in bits[voxels["kind"][mine] == bit]), (b, bit)
        assert listed == l_added | l_removed | l_repainted and l_added & l_removed == l_added & l_repainted == l_removed & l_repainted == 0
        assert np.all(np.diff(bits) > 0)                                         # the witness's order inside a brick is the ascending bit
        a, c, here = cube(before, b), cube(after, b), cube(inside, b)
        assert solid_before == brick_word((a != 0) & here) and solid_after == brick_word((c != 0) & here)
        assert added == (brick_word((a == 0) & (c != 0) & here) if kinds & W.ADDED else 0)
        assert removed == (brick_word((a != 0) & (c == 0) & here) if kinds & W.REMOVED else 0)
        assert candidates == (brick_word((a != 0) & (c != 0) & here) if kinds & W.REPAINTED else 0)
        total += bin(listed).count("1")
    assert total == int(result["voxels"])
    assert sum(bin(r[0]).count("1") for r in rows) == int(result["solid_before"]) and sum(bin(r[1]).count("1") for r in rows) == int(result["solid_after"])
    return total


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_random_pairs_every_kinds_value(exe, density):
    before, after = pair(int(density * 100), density)
    whole = ((0, 0, 0), (255, 255, 255))
    totals = [check_pair(exe, before, after, kinds, -1, whole) for kinds in range(1, 8)]
    assert totals[6] == totals[0] + totals[1] + totals[3] and min(totals[0], totals[1], totals[3]) > 0
    for palette in (0, 1, 2, 9):
        check_pair(exe, before, after, W.ALL, palette, whole)
    check_pair(exe, before, after, W.ADDED | W.REPAINTED, 1, whole)


def test_regions_that_cut_through_bricks(exe):
    before, after = pair(17, 0.6)
    rng = np.random.default_rng(18)
    regions = [((0, 0, 0), (0, 0, 0)), ((11, 11, 11), (255, 255, 255)), ((1, 2, 3), (5, 9, 10)), ((4, 4, 4), (7, 7, 7)), ((3, 0, 0), (4, 255, 255)),
               ((0, 5, 0), (255, 5, 255)), ((12, 0, 0), (20, 5, 5))]
    for _ in range(12):
        lo = rng.integers(0, 10, 3)
        regions.append((tuple(int(v) for v in lo), tuple(int(v) for v in lo + rng.integers(0, 8, 3))))
    listed = [check_pair(exe, before, after, (7, 1, 2, 4, 6)[k % 5], (-1, -1, 1)[k % 3], region) for k, region in enumerate(regions)]
    assert sum(listed) > 100 and sum(1 for n in listed if n) > 10 and listed[6] == 0      # (not vacuous: most regions list something)


def test_all_ones_and_all_zero_words(exe):
    whole = "0 0 0 0 0 0 255 255 255"
    lines = [f"w 0 0 {whole} 7 {ONES} {ONES}",          # nothing in either: nothing, whatever the ballots say
             f"w 0 {ONES} {whole} 7 {ONES} {ONES}",     # a brick solid only after
             f"w {ONES} 0 {whole} 7 {ONES} {ONES}",     # ... only before
             f"w {ONES} {ONES} {whole} 7 {ONES} {ONES}",  # a whole brick repainted: the words are equal, only the bytes show it
             f"w {ONES} {ONES} {whole} 7 0 {ONES}",     # a whole brick identical in both
             f"w {ONES} {ONES} {whole} 3 {ONES} {ONES}",  # repainted, but not asked for
             f"w 0 {ONES} {whole} 7 {ONES} 0",          # added, but nothing passes the filter
             f"w 0 {ONES} 0 0 0 1 2 3 255 255 255 1 {ONES} {ONES}"]   # ... behind a region that cuts the brick
    got = run(exe, lines)
    assert got[0] == [0] * 9
    assert got[1] == [0, ONES, ONES, 0, 0, ONES, 0, 0, ONES]
    assert got[2] == [ONES, 0, 0, ONES, 0, 0, ONES, 0, ONES]
    assert got[3] == [ONES, ONES, 0, 0, ONES, 0, 0, ONES, ONES]
    assert got[4] == [ONES, ONES, 0, 0, ONES, 0, 0, 0, 0]
    assert got[5] == [ONES, ONES, 0, 0, 0, 0, 0, 0, 0]
    assert got[6] == [0, ONES, ONES, 0, 0, 0, 0, 0, 0]
    cut = brick_word(np.indices((4, 4, 4))[0] >= 1) & brick_word(np.indices((4, 4, 4))[1] >= 2) & brick_word(np.indices((4, 4, 4))[2] >= 3)
    assert got[7] == [0, cut, cut, 0, 0, cut, 0, 0, cut] and bin(cut).count("1") == 3 * 2 * 1


def test_query_validation_table_and_clipping(exe):
    queries = [(kinds, flags, palette, lo, hi)
               for kinds in (0, 1, 2, 3, 4, 5, 6, 7, 8, 0xFFFFFFFF) for flags in (0, 1, 2, 1 << 31) for palette in (-2, -1, 0, 254, 255)
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((17, 3, 250), (40, 3, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 4000)))]
    got = run(exe, ["q " + " ".join(str(v) for v in (kinds, flags, palette) + lo + hi) for kinds, flags, palette, lo, hi in queries])
    accepted = 0
    for (kinds, flags, palette, lo, hi), row in zip(queries, got):
        if W.refused(kinds, flags, palette, lo, hi):
            assert row == [0], (kinds, flags, palette, lo, hi)
            continue
        accepted += 1
        empty = any(l > h for l, h in zip(lo, hi))
        assert row[:4] == [1, int(empty), kinds, palette + 1]
        if empty:
            assert len(row) == 4
        else:
            assert row[4:] == list(lo) + list(hi) + [v >> 4 for v in lo] + [v >> 4 for v in hi]
    assert accepted == 7 * 1 * 3 * 3


def test_result_record(exe):
    acc = [10, 20, 30, 77, 88, 255 - 3, 255 - 0, 255 - 200, 9, 255, 201]
    got = run(exe, ["r", "r " + " ".join(str(v) for v in acc), "r " + " ".join(["0"] * 3 + ["5", "6"] + ["0"] * 6)])
    zero = W.zero_result()
    assert got[0] == [0] * 6 + zero["lo"].tolist() + zero["hi"].tolist() + [0]
    assert got[1] == [60, 10, 20, 30, 77, 88, 3, 0, 200, 9, 255, 201, 0]
    assert got[2] == [0, 0, 0, 0, 5, 6, 255, 255, 255, 0, 0, 0, 0]      # solid voxels, none listed: the bounds of the zero result


def test_apply_records_keep_the_last_of_a_key(exe):
    rng = np.random.default_rng(19)
    records = np.zeros(600, W.VOXEL_DTYPE)
    records["key"] = rng.integers(0, 200, 600)                                   # every key about three times
    records["key"][:3] = [0, (1 << 24) - 1, (255 << 16) | 255]
    records["kind"], records["before"], records["after"] = rng.integers(0, 256, 600), rng.integers(0, 256, 600), rng.integers(0, 256, 600)

    def line(r):
        return f"a {len(r)} " + " ".join(f"{k} {kind} {b} {a}" for k, kind, b, a, _ in r.tolist())
    got = run(exe, [line(records), line(records[:0]), line(records[:1])])
    kept = W.survivors(records)
    assert got[0][0] == 1 and got[0][1] == len(kept) < 300
    words = {w & 0xFFFFFFFF: w for w in got[0][2:]}
    assert len(words) == len(kept)                                                # no key twice
    for key, kind, b, a, _ in kept.tolist():
        assert words[key] == key | (kind << 32) | (b << 40) | (a << 48)
    assert got[1] == [1, 0] and got[2][:2] == [1, 1]
    # a key of 2^24 or above is refused, wherever it stands
    for at in (0, 299, 599):
        bad = records.copy()
        bad["key"][at] = 1 << 24
        assert run(exe, [line(bad)]) == [[0]]
    bad["key"][5] = 0xFFFFFFFF
    assert run(exe, [line(bad)]) == [[0]]
