"""dust_amd/csrc/fracture_rule.hpp (the text k_fracture_label of fracture.hip runs) and the fracture records of
dust_amd/csrc/model_records.hpp (device_fracture, fracture_seeds, fracture_apply_arguments, fracture_selection, fracture_result) run as
native code on a CPU: tests/cpp/fracture_rule_test.cpp compiled with g++ under AddressSanitizer and UBSan into a program of its own, fed
boxes and seed sets on stdin. The program checks min_d2 / max_d2 against loops over the box and that the pruned candidates hold every
voxel's brute-force winner; here its labels are held to the witness (tests/fracture_witness.py). UBSan is the overflow check: the seed
sets include -1024 and 1279 under scale 16."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import fracture_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "fracture_rule_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fracture_rule") / "fracture_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def boxes(rng):
    """single voxels, 4^3 bricks, 16^3 cells and region-clipped slivers, at the tree's faces too"""
    out = []
    for _ in range(6):
        p = [int(c) for c in rng.integers(0, 256, 3)]
        out.append((p, p))
    for _ in range(6):
        b = [int(c) * 4 for c in rng.integers(0, 64, 3)]
        out.append((b, [c + 3 for c in b]))
    for cell in ((0, 0, 0), (15, 15, 15), (3, 9, 15), (7, 0, 12)):
        out.append(([c * 16 for c in cell], [c * 16 + 15 for c in cell]))
    for _ in range(6):                                 # a cell's box clipped by a region: thin in one or two axes
        cell = [int(c) * 16 for c in rng.integers(0, 16, 3)]
        lo = [c + int(rng.integers(0, 16)) for c in cell]
        hi = [min(l + int(rng.integers(0, 3)) if rng.random() < 0.6 else c + 15, c + 15) for l, c in zip(lo, cell)]
        out.append((lo, hi))
    return out


def seed_sets(rng, lo, hi):
    near = rng.integers(np.array(lo) - 6, np.array(hi) + 7, (9, 3))
    wide = rng.integers(W.SEED_MIN, W.SEED_MAX + 1, (12, 3))
    corners = np.array(list(itertools.product((W.SEED_MIN, W.SEED_MAX), repeat=3)))
    lattice = np.array(list(itertools.product(range(lo[0] - 2, lo[0] + 7, 4), range(lo[1] - 2, lo[1] + 7, 4), range(lo[2] - 2, lo[2] + 7, 4))))  # even spacing: ties
    dup = np.concatenate([near[:3], near[:3], near[:3]])
    return [np.clip(s, W.SEED_MIN, W.SEED_MAX) for s in (near, wide, corners, np.concatenate([wide, near]), lattice, dup, near[:1], corners[-1:])]


def test_boxes_candidates_and_winners(exe):
    rng = np.random.default_rng(11)
    cases = []
    for lo, hi in boxes(rng):
        for k, seeds in enumerate(seed_sets(rng, lo, hi)):
            scale = [(1, 1, 1), (16, 16, 16), (1, 16, 3), (7, 2, 16)][k % 4]
            volume = int(np.prod([h - l + 1 for l, h in zip(lo, hi)]))
            for limit in (W.NO_LIMIT, 0, int(rng.integers(1, 400)) * max(scale)):
                if volume > 512 and limit != W.NO_LIMIT and k % 3:
                    continue                            # (the large boxes: fewer cases, the loops are in a sanitised program)
                cases.append((scale, limit, lo, hi, seeds))
    lines = [f"b {s[0]} {s[1]} {s[2]} {limit} {lo[0]} {lo[1]} {lo[2]} {hi[0]} {hi[1]} {hi[2]} {len(seeds)} " + " ".join(str(int(c)) for c in seeds.reshape(-1))
             for s, limit, lo, hi, seeds in cases]
    got = run(exe, lines)
    assert len(got) == len(cases)
    pruned = labelled = 0
    for (scale, limit, lo, hi, seeds), row in zip(cases, got):
        n = len(seeds)
        xyz = np.stack(np.meshgrid(*[np.arange(l, h + 1) for l, h in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)
        best, index = W.nearest(xyz, seeds, scale)
        want = np.where((limit == W.NO_LIMIT) | (best <= limit), index, W.NO_CELL)
        assert row[2:2 + len(xyz)] == want.tolist(), (scale, limit, lo, hi)
        d = np.stack([xyz[:, None, r] - seeds[None, :, r] for r in range(3)], axis=2).astype(np.int64)
        d2 = (d * d * np.array(scale)).sum(axis=2)
        assert row[2 + len(xyz):2 + len(xyz) + n] == d2.min(axis=0).tolist() and row[2 + len(xyz) + n:] == d2.max(axis=0).tolist()
        assert row[1] == d2.max(axis=0).min() and 0 <= row[0] <= n and (row[0] >= 1 or limit != W.NO_LIMIT)
        assert d2.max() < 1 << 27
        pruned += n - row[0]
        labelled += int(np.count_nonzero(want != W.NO_CELL))
    assert pruned > 500 and labelled > 20000


def test_a_full_list_of_duplicates_survives(exe):
    """4096 seeds on 8 positions: every duplicate of a winner is a candidate (its min_d2 is the winner's), the lowest index wins"""
    rng = np.random.default_rng(12)
    positions = np.array([(x, y, z) for x in (18, 29) for y in (18, 29) for z in (18, 29)])
    seeds = positions[rng.integers(0, 8, 4096)]
    lo, hi = (16, 16, 16), (31, 31, 31)
    row = run(exe, [f"b 1 1 1 {W.NO_LIMIT} {lo[0]} {lo[1]} {lo[2]} {hi[0]} {hi[1]} {hi[2]} 4096 " + " ".join(str(int(c)) for c in seeds.reshape(-1))])[0]
    assert row[0] == 4096
    labels = set(row[2:2 + 4096])
    firsts = {int(np.flatnonzero((seeds == p).all(axis=1))[0]) for p in positions}
    assert labels == firsts and len(labels) == 8


def test_query_table_against_the_witness(exe):
    queries = [(palette, scale, flags, r0, r, limit, lo, hi)
               for palette in (-2, -1, 0, 254, 255) for scale in ((1, 1, 1), (16, 1, 3), (0, 1, 1), (1, 17, 1), (1, 1, 255))
               for flags, r0, r in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 7)) for limit in (W.NO_LIMIT, 0, 576)
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((11, 119, 250), (40, 130, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 300, 1)), ((0, 0, 0), (1, 1, 4000)))]
    got = run(exe, ["q " + " ".join(str(v) for v in (palette,) + scale + (flags, r0, r, limit) + lo + hi) for palette, scale, flags, r0, r, limit, lo, hi in queries])
    accepted = 0
    for (palette, scale, flags, r0, r, limit, lo, hi), row in zip(queries, got):
        if W.refused(palette, scale, flags, r0, r):
            assert row == [0]
            continue
        accepted += 1
        box = W.clip((lo, hi))
        assert row[:7] == [1, int(box is None), palette + 1, limit] + list(scale)
        assert row[7:] ==([] if box is None else box[0] + box[1] + [l >> 4 for l in box[0]] + [h >> 4 for h in box[1]])
    assert 0 < accepted < len(queries)
    seeds = [(0, 0, 0, 0), (-1024, 1279, -1024, 0), (-1025, 0, 0, 0), (0, 1280, 0, 0), (0, 0, -2000000000, 0), (5, 5, 5, 1), (2147483647, 0, 0, 0)]
    got = run(exe, [f"s {x} {y} {z} {r}" for x, y, z, r in seeds])
    assert [row[0] for row in got] == [int(not W.refused(seeds=[(x, y, z)], seed_reserved=r)) for x, y, z, r in seeds] == [1, 1, 0, 0, 0, 0, 0]
    applies = [(0, -1), (1, 254), (2, 0), (0, 255), (1, -2), (0xFFFFFFFF, 0), (0, 0)]
    got = run(exe, [f"a {w} {v}" for w, v in applies])
    assert [row[0] for row in got] == [int(not W.apply_refused(w, v)) for w, v in applies] == [1, 1, 0, 0, 0, 0, 1]


def test_selection_and_result_records(exe):
    got = run(exe, ["d 10 4 0 9 9 3", "d 10 1 10", "d 4096 2 4095 64", "d 0 1 0", "d 5 0"])
    assert got[0] == [1, (1 << 0) | (1 << 9) | (1 << 3)] + [0] * 63 and got[1] == [0] and got[3] == [0] and got[4] == [1] + [0] * 64
    assert got[2] == [1, 0, 1] + [0] * 61 + [1 << 63]
    acc = [0] * 16
    acc[0], acc[1], acc[2], acc[3] = 900, 700, 55, 12345
    acc[4:7], acc[7:10] = [255 - 9, 255 - 118, 255 - 201], [56, 165, 248]
    acc[10], acc[12], acc[13] = 6, 0xFFFFFFFF - 4, 300
    none = list(acc)
    none[1] = none[10] = 0
    got = run(exe, ["r", "r " + " ".join(str(v) for v in acc), "r " + " ".join(str(v) for v in none), "e"])
    assert got[0] == [0, 0, 0, 0xFFFFFFFF, 0, 0, 0, 255, 255, 255, 0, 0, 0, 0]
    assert got[1] == [900, 700, 6, 4, 300, 55, 12345, 9, 118, 201, 56, 165, 248, 0]
    assert got[2] == [900, 0, 0, 0xFFFFFFFF, 0, 55, 0, 255, 255, 255, 0, 0, 0, 0]
    assert got[3] == [0, 0, 255, 255, 255, 0, 0, 0, 0, 0, 0, 0]
    zero = W.result(np.zeros((4, 4, 4), np.uint8), np.full((4, 4, 4), W.NO_CELL, np.uint16), np.zeros((4, 4, 4), np.int64))
    assert got[0][:13] == [int(c) for f in ("solid", "labelled", "cells", "largest_cell", "largest_voxels", "cut_faces", "max_d2", "lo", "hi") for c in np.atleast_1d(zero[f])]
