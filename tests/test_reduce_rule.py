"""dust_amd/csrc/reduce_rule.hpp (reduce_vote, device_reduce, reduce_result) run as native code on a CPU:
tests/cpp/reduce_rule_test.cpp compiled with g++ under AddressSanitizer and UBSan into a program of its own, held to the witness
(tests/reduce_witness.py) on every combination of eight children over {None, 0, 1}, every threshold, random cells over all 256 byte
values and the query validation table; and the plan of the levels device_reduce makes, replayed on numpy grids full of stale bytes."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import reduce_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "reduce_rule_test.cpp")
SOURCE, MODEL, SCRATCH = 0, 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("reduce_rule") / "reduce_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-I", CSRC, SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def votes(exe, cells, min_solid):
    """cells (n, 8) uint8 -> the program's coarse bytes"""
    packed = (cells.astype(np.uint64) << (np.arange(8, dtype=np.uint64) * np.uint64(8))).sum(axis=1, dtype=np.uint64)
    return np.array(run(exe, [f"v {int(p)} {min_solid}" for p in packed]), np.uint8).reshape(-1)


def witness(cells, min_solid):
    """cells (n, 8) -> the witness's coarse bytes: the cells stacked along x, each a 2^3 cube (the vote does not depend on the order)"""
    return W.level(cells.reshape(-1, 2, 2), min_solid).reshape(-1)


def embed(cube):
    """a cube at the origin of an otherwise empty 256^3 grid"""
    out = np.zeros((256,) * 3, np.uint8)
    n = cube.shape[0]
    out[:n, :n, :n] = cube
    return out


def test_every_combination_of_none_and_two_materials_under_every_threshold(exe):
    cells = np.array(list(itertools.product((0, 1, 2), repeat=8)), np.uint8)      # grid bytes: None, palette 0, palette 1
    assert len(cells) == 3 ** 8
    for min_solid in range(1, 9):
        assert np.array_equal(votes(exe, cells, min_solid), witness(cells, min_solid)), min_solid


def test_random_cells_over_all_byte_values(exe):
    rng = np.random.default_rng(11)
    cells = rng.integers(0, 256, (10000, 8)).astype(np.uint8)
    few = rng.integers(0, 4, (10000, 8))                   # few distinct values per cell, so that counts above 1 and ties are common
    cells = np.where(rng.random((10000, 1)) < 0.5, cells, np.take_along_axis(cells, few, axis=1))
    cells[rng.random(cells.shape) < 0.2] = 0
    cells[:50, :] = np.where(rng.random((50, 8)) < 0.5, 255, 254)      # palette 254 (byte 255) against its neighbour
    thresholds = rng.integers(1, 9, 10000)
    want = np.zeros(10000, np.uint8)
    got = np.zeros(10000, np.uint8)
    for min_solid in range(1, 9):
        pick = thresholds == min_solid
        want[pick] = witness(cells[pick], min_solid)
        got[pick] = votes(exe, cells[pick], min_solid)
    assert np.array_equal(got, want)
    assert 255 in set(want.tolist()) and 0 in set(want.tolist())


def test_query_validation_table_and_result_record(exe):
    queries = [(lv, ms, fl) for lv in (0, 1, 2, 7, 8, 9, 0xFFFFFFFF) for ms in (0, 1, 4, 8, 9, 0xFFFFFFFF) for fl in (0, 1, 1 << 31)]
    got = run(exe, [f"q {lv} {ms} {fl}" for lv, ms, fl in queries])
    for (lv, ms, fl), row in zip(queries, got):
        assert row[0] == int(W.valid(lv, ms, fl)), (lv, ms, fl)
        if row[0]:
            assert row[1:3] == [lv, 256 >> lv] and len(row) == 3 + 7 * lv
    assert run(exe, ["r 3 1000 17", "r 8 5 1"]) == [[1000, 17, 32, 0], [5, 1, 1, 0]]


@pytest.mark.parametrize("levels", [1, 2, 3, 8])
def test_plan_replayed_on_stale_grids_leaves_the_witness_grid(exe, levels):
    """what the kernel does with a level of the plan, in numpy: read [0, 2 * extent)^3 of `from`, write whole bricks of [0, cover)^3 of
    `to` -- the vote inside [0, extent)^3, zero outside --, and under `fresh` nothing where a brick comes out empty. The new model's
    grid starts zero, the scratch full of another call's bytes; afterwards the model's grid is the witness's, zero padding included."""
    rng = np.random.default_rng(13)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[:48, :48, :48] = np.where(rng.random((48,) * 3) < 0.5, rng.integers(1, 5, (48,) * 3), 0)
    grid[224:, 96:128, 250:] = 9
    row = run(exe, [f"q {levels} 1 0"])[0]
    assert row[:2] == [1, levels]
    plan = [row[3 + 7 * k: 10 + 7 * k] for k in range(levels)]
    bufs = {SOURCE: grid, MODEL: np.zeros((256,) * 3, np.uint8), SCRATCH: rng.integers(1, 256, (256,) * 3).astype(np.uint8)}
    before = grid.copy()
    for k, (src, dst, extent, cover, fresh, count_src, count_dst) in enumerate(plan):
        assert src != dst and dst != SOURCE and extent == 256 >> (k + 1) and cover >= extent
        assert (count_src, count_dst) == (int(k == 0), int(k == levels - 1))
        side = max(cover, 4)
        out = np.zeros((side,) * 3, np.uint8)
        out[:extent, :extent, :extent] = W.reduce(embed(bufs[src][:2 * extent, :2 * extent, :2 * extent]), 1, 1)[:extent, :extent, :extent]
        if fresh:
            assert not bufs[dst][:side, :side, :side].any()      # skipping the empty bricks is only right over zeros
        bufs[dst][:side, :side, :side] = out
    assert plan[-1][1] == MODEL and np.array_equal(grid, before)
    assert np.array_equal(bufs[MODEL], W.reduce(grid, levels, 1))
