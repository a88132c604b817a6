"""The witness of the model reductions (tests/reduce_witness.py) against the header's rule spelled out cell by cell with
collections.Counter, and the properties the header states: levels = n is the one-level rule applied n times, levels = 8 is one voxel,
and the vote of votes is not one vote over 8^n voxels."""
import collections

import numpy as np
import pytest

import reduce_witness as W


def cell_by_cell(grid, min_solid):
    """the header's one-level rule, one coarse voxel at a time"""
    n = grid.shape[0] // 2
    out = np.zeros((n, n, n), np.uint8)
    for x in range(n):
        for y in range(n):
            for z in range(n):
                kids = [int(grid[2 * x + i, 2 * y + j, 2 * z + k]) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
                votes = collections.Counter(b for b in kids if b)
                if sum(votes.values()) >= min_solid and votes:
                    top = max(votes.values())
                    out[x, y, z] = min(b for b, c in votes.items() if c == top)
    return out


def embed(region):
    grid = np.zeros((256,) * 3, np.uint8)
    n = region.shape[0]
    grid[:n, :n, :n] = region
    return grid


@pytest.fixture(scope="module")
def region():
    rng = np.random.default_rng(5)
    return np.where(rng.random((24, 24, 24)) < 0.6, rng.integers(1, 4, (24, 24, 24)), 0).astype(np.uint8)


@pytest.mark.parametrize("min_solid", range(1, 9))
def test_witness_is_the_rule_cell_by_cell(region, min_solid):
    want = region
    for levels in (1, 2, 3):
        want = cell_by_cell(want, min_solid)
        got = W.reduce(embed(region), levels, min_solid)
        n = 24 >> levels
        assert np.array_equal(got[:n, :n, :n], want), (levels, min_solid)
        assert np.count_nonzero(got) == np.count_nonzero(want)          # zero padding everywhere else
        assert np.array_equal(W.level(region, min_solid), cell_by_cell(region, min_solid))


def test_ties_go_to_the_lowest_index_and_byte_255_votes():
    cell = np.array([5, 9, 9, 5, 0, 0, 255, 255], np.uint8).reshape(2, 2, 2)
    assert W.level(cell, 1).tolist() == [[[5]]] and W.level(cell, 6).tolist() == [[[5]]] and W.level(cell, 7).tolist() == [[[0]]]
    cell = np.array([255, 0, 0, 0, 0, 0, 0, 0], np.uint8).reshape(2, 2, 2)
    assert W.level(cell, 1).tolist() == [[[255]]] and W.level(cell, 2).tolist() == [[[0]]]


def test_two_levels_are_one_level_twice(region):
    grid = embed(region)
    grid[200:256, 130:140, 255] = 7
    for min_solid in (1, 3, 4, 8):
        assert np.array_equal(W.reduce(grid, 2, min_solid), W.reduce(W.reduce(grid, 1, min_solid), 1, min_solid))
        assert np.array_equal(W.reduce(grid, 5, min_solid), W.reduce(W.reduce(grid, 2, min_solid), 3, min_solid))


def test_eight_levels_are_one_voxel(region):
    grid = embed(region)
    one = W.reduce(grid, 8, 1)
    assert np.count_nonzero(one) == 1 and one[0, 0, 0] != 0
    assert np.count_nonzero(W.reduce(grid, 8, 8)) == 0
    assert np.count_nonzero(W.reduce(np.full((256,) * 3, 9, np.uint8), 8, 8)) == 1
    r = W.result(grid, one, 8)
    assert (int(r["src_voxels"]), int(r["voxels"]), int(r["extent"])) == (np.count_nonzero(region), 1, 1)


def test_the_vote_of_votes_is_not_one_big_vote():
    """a 4^3 cell: material 1 in 5 voxels of each of three children (15 voxels), material 2 in all 8 voxels of two others (16 voxels).
    Level by level the children vote 1, 1, 1, 2, 2 and the cell takes 1; one vote over the 64 voxels would give 2."""
    cell = np.zeros((4, 4, 4), np.uint8)
    for corner in ((0, 0, 0), (2, 0, 0), (0, 2, 0)):
        child = np.zeros(8, np.uint8)
        child[:5] = 2            # grid byte = palette index + 1
        cell[tuple(slice(c, c + 2) for c in corner)] = child.reshape(2, 2, 2)
    for corner in ((0, 0, 2), (2, 2, 2)):
        cell[tuple(slice(c, c + 2) for c in corner)] = 3
    assert np.count_nonzero(cell == 2) == 15 and np.count_nonzero(cell == 3) == 16
    assert collections.Counter(cell[cell != 0].tolist()).most_common(1)[0][0] == 3
    got = W.reduce(embed(cell), 2, 1)
    assert got[0, 0, 0] == 2 and np.count_nonzero(got) == 1
