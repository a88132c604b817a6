"""The witness of the model floods (tests/flood_witness.py) against hand-computed cases and against an independent queue search on small
grids; and the shared scenes are what the device tests take them for."""
import collections

import numpy as np
import pytest

import flood_witness as W


def queue_search(grid, seeds, medium, palette, max_steps, region):
    """a textbook breadth-first search, a voxel at a time: shares nothing with the witness but the definition of `passable`"""
    grid = np.asarray(grid)
    box = W.clip(region, grid.shape)

    def ok(p):
        if box is None or any(c < 0 or c >= n for c, n in zip(p, grid.shape)):
            return False
        if any(c < lo or c > hi for c, lo, hi in zip(p, *box)):
            return False
        g = int(grid[p])
        return g == 0 if medium == W.EMPTY else g != 0 if medium == W.SOLID else g == palette + 1

    out = np.full(grid.shape, W.UNREACHED, np.uint16)
    todo = collections.deque()
    for s in seeds:
        s = tuple(int(v) for v in s)
        if ok(s) and out[s] == W.UNREACHED:
            out[s] = 0
            todo.append(s)
    while todo:
        p = todo.popleft()
        if out[p] == max_steps:
            continue
        for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
            if ok(q) and out[q] == W.UNREACHED:
                out[q] = out[p] + 1
                todo.append(q)
    return out


def test_hand_computed_line_and_wall():
    grid = np.zeros((7, 3, 1), np.uint8)
    grid[3, :2, 0] = 5            # a wall across the strip with a gap at y = 2
    f = W.steps(grid, [(0, 0, 0)])
    assert f[:, :, 0].T.tolist() == [[0, 1, 2, W.UNREACHED, 8, 9, 10], [1, 2, 3, W.UNREACHED, 7, 8, 9], [2, 3, 4, 5, 6, 7, 8]]
    r = W.result(f)
    assert (int(r["reached"]), int(r["farthest"]), int(r["seeds_used"])) == (19, 10, 1)
    assert r["lo"].tolist() == [0, 0, 0] and r["hi"].tolist() == [6, 2, 0] and int(r["boundary"]) == 19     # one layer thick: every voxel is on a face
    f = W.steps(grid, [(0, 0, 0)], max_steps=4)
    assert np.count_nonzero(f != W.UNREACHED) == 9 and f.max() == W.UNREACHED and f[f != W.UNREACHED].max() == 4
    f = W.steps(grid, [(0, 0, 0)], max_steps=0)
    assert np.count_nonzero(f != W.UNREACHED) == 1
    f = W.steps(grid, [(3, 0, 0), (3, 0, 0), (0, 0, 0)], medium=W.SOLID)         # the wall itself: the empty seed is ignored
    assert f[3, :, 0].tolist() == [0, 1, W.UNREACHED] and int(W.result(f)["seeds_used"]) == 1
    assert not (W.steps(grid, [(3, 0, 0)], medium=W.MATERIAL, palette=3) != W.UNREACHED).any()
    assert np.count_nonzero(W.steps(grid, [(3, 0, 0)], medium=W.MATERIAL, palette=4) != W.UNREACHED) == 2
    f = W.steps(grid, [(0, 0, 0), (6, 2, 0)], region=((0, 0, 0), (2, 9, 9)))     # the second seed is outside the region
    assert np.count_nonzero(f != W.UNREACHED) == 9 and int(W.result(f, ((0, 0, 0), (2, 9, 9)))["boundary"]) == 9
    assert not (W.steps(grid, [(0, 0, 0)], region=((2, 0, 0), (1, 2, 0))) != W.UNREACHED).any()
    empty = W.result(W.steps(grid, []))
    assert empty.tobytes() == bytes(32)


def test_hand_computed_paths_and_apply():
    grid = np.zeros((3, 3, 1), np.uint8)
    f = W.steps(grid, [(0, 0, 0)])
    keys = np.full((3, 4), 77, np.uint32)
    lengths, keys = W.paths(f, [(2, 2, 0), (0, 0, 0), (1, 1, 0)], 4, keys)
    # ties go to -x first: from (2, 2) the way runs along -x to x = 0, then along -y
    assert lengths.tolist() == [5, 1, 3]
    assert keys.tolist() == [[0x020200, 0x010200, 0x000200, 0x000100], [0, 77, 77, 77], [0x010100, 0x000100, 0, 77]]
    grid[1, 1, 0] = 9
    f = W.steps(grid, [(0, 0, 0)])
    lengths, keys = W.paths(f, [(1, 1, 0), (2, 1, 0)], 2)
    assert lengths.tolist() == [0, 4] and keys.tolist() == [[0, 0], [0x020100, 0x020000]]
    after, changed = W.apply(grid, f, 3, max_steps=2)
    assert changed == 5 and np.count_nonzero(after == 4) == 5 and after[1, 1, 0] == 9 and after[2, 2, 0] == 0
    after, changed = W.apply(after, f, 3)
    assert changed == 3
    after, changed = W.apply(after, W.steps(after, [(1, 1, 0)], medium=W.SOLID), -1)
    assert changed == 9 and not after.any()


@pytest.mark.parametrize("seed", range(6))
def test_matches_a_queue_search_on_small_grids(seed):
    rng = np.random.default_rng(100 + seed)
    shape = tuple(rng.integers(3, 11, 3))
    grid = np.where(rng.random(shape) < 0.45, rng.integers(1, 4, shape), 0).astype(np.uint8)
    seeds = rng.integers(0, 10, (4, 3)) % np.array(shape)
    for medium in (W.EMPTY, W.SOLID, W.MATERIAL):
        for max_steps, region in ((W.MAX_STEPS, None), (3, None), (W.MAX_STEPS, ((1, 0, 2), (6, 255, 5))), (5, ((0, 1, 0), (255, 4, 255)))):
            want = queue_search(grid, seeds, medium, 1, max_steps, region)
            got = W.steps(grid, seeds, medium, 1, max_steps, region)
            assert np.array_equal(got, want), (medium, max_steps, region)
            lengths, _ = W.paths(got, np.argwhere(np.ones(shape, bool)), 1)
            assert np.array_equal(lengths, np.where(got == W.UNREACHED, 0, got.astype(np.uint32) + 1).reshape(-1))


def adjacent(a, b):
    return int(np.abs(np.asarray(a) - np.asarray(b)).sum()) == 1


def assert_snake(path):
    """consecutive voxels share a face, no others do"""
    path = [tuple(int(v) for v in p) for p in path]
    assert len(set(path)) == len(path)
    for i, p in enumerate(path):
        for j in range(i + 1, len(path)):
            assert adjacent(p, path[j]) == (j == i + 1), (i, j)


def crossings(path):
    return int(np.count_nonzero(np.any(np.diff(np.asarray(path) >> 2, axis=0) != 0, axis=1)))


def test_shared_scenes_are_what_they_claim():
    grid, path = W.brick_snake()
    assert_snake(path)
    assert len(path) == 22 and len({tuple(p) for p in path >> 2}) == 1 and not (path[0] & 3).any()      # inside one brick
    f = W.steps(grid, [path[0]], medium=W.SOLID)
    assert W.at(f, path).tolist() == list(range(22))
    grid, seed, target, detour, shortcut = W.late_shortcut()
    assert_snake(detour) and assert_snake(shortcut)
    assert tuple(detour[0]) == tuple(shortcut[0]) == tuple(seed) and tuple(detour[-1]) == tuple(shortcut[-1]) == tuple(target)
    assert len(detour) == 40 and len(shortcut) == 24 and crossings(detour) == 3 and crossings(shortcut) == 5
    f = W.steps(grid, [seed], medium=W.SOLID)
    assert int(f[tuple(target)]) == 23 and int(f[tuple(detour[-2])]) == 24       # the end of the detour is reached from the target
    grid, empty, solid = W.corridors()
    for runs, medium in ((empty, W.EMPTY), (solid, W.SOLID)):
        f = W.steps(grid, [r[0] for r in runs], medium=medium)
        for r in runs:
            assert W.at(f, r).tolist() == list(range(31))
            assert len(np.unique(r >> 4, axis=0)) == 3 and len(np.unique(r >> 2, axis=0)) >= 8      # root cells and bricks along it
        assert int(W.result(f)["reached"]) == 93


def test_random_fill_has_the_recorded_figures():
    grid, region, seeds = W.random_fill()
    o = W.RANDOM_ORIGIN
    assert any(v % 4 for v in o)
    block = grid[o[0]:o[0] + 64, o[1]:o[1] + 64, o[2]:o[2] + 64]
    assert np.count_nonzero(block == 0) == 89144 and np.count_nonzero(grid) == np.count_nonzero(block)
    r = W.result(W.steps(grid, seeds[W.EMPTY], region=region), region)
    assert (int(r["reached"]), int(r["farthest"]), int(r["seeds_used"])) == (52376, 270, 3)
