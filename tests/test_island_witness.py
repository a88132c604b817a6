"""The numpy witness of the model islands (tests/island_witness.py) against answers written out by hand and, where scipy is installed,
against scipy.ndimage.label: the witness is what the GPU tests hold dust_hip_model_find_islands, island_of and detach_islands to."""
import numpy as np
import pytest

import island_witness as W


def key(x, y, z):
    return x << 16 | y << 8 | z


def grid_of(*voxels, shape=(8, 8, 8)):
    g = np.zeros(shape, np.uint8)
    for i, v in enumerate(voxels):
        g[v] = i + 1
    return g


def test_connectivity_by_hand():
    # a face pair, an edge pair and a corner pair, far from each other
    g = grid_of((0, 0, 0), (1, 0, 0), (4, 0, 0), (5, 1, 0), (0, 4, 4), (1, 5, 5))
    faces = W.records(W.label(g, W.FACES))
    assert faces["key"].tolist() == [key(0, 0, 0), key(0, 4, 4), key(1, 5, 5), key(4, 0, 0), key(5, 1, 0)]
    assert faces["voxels"].tolist() == [2, 1, 1, 1, 1]
    corners = W.records(W.label(g, W.CORNERS))
    assert corners["key"].tolist() == [key(0, 0, 0), key(0, 4, 4), key(4, 0, 0)]
    assert corners["voxels"].tolist() == [2, 2, 2]
    assert corners["lo"].tolist() == [[0, 0, 0], [0, 4, 4], [4, 0, 0]] and corners["hi"].tolist() == [[1, 0, 0], [1, 5, 5], [5, 1, 0]]
    assert corners["sum"].tolist() == [[1, 0, 0], [1, 9, 9], [9, 1, 0]]
    assert not corners["flags"].any() and not corners["reserved"].any()


def test_the_key_is_the_smallest_x_then_y_then_z():
    # an L whose smallest key is not where a z-fastest or a brick-order scan would start
    g = grid_of((3, 0, 7), (3, 1, 7), (3, 1, 6), (2, 1, 6), (2, 2, 6), shape=(4, 4, 8))
    lab = W.label(g, W.FACES)
    assert set(lab[g != 0].tolist()) == {key(2, 1, 6)} and (lab[g == 0] == W.NO_ISLAND).all()
    rec = W.records(lab)[0]
    assert (rec["key"], rec["voxels"], rec["lo"].tolist(), rec["hi"].tolist(), rec["sum"].tolist()) == (key(2, 1, 6), 5, [2, 0, 6], [3, 2, 7], [13, 5, 32])


def test_anchor_box_island_of_and_detach_by_hand():
    g = W.full(grid_of((0, 0, 0), (0, 1, 0), (0, 3, 0), (0, 4, 0), (6, 6, 6)))
    lab = W.label(g, W.FACES)
    rec = W.records(lab, anchor=((0, 0, 0), (255, 0, 255)))
    assert rec["key"].tolist() == [key(0, 0, 0), key(0, 3, 0), key(6, 6, 6)] and rec["flags"].tolist() == [W.ANCHORED, 0, 0]
    assert W.records(lab, anchor=((0, 4, 0), (1000, 1000, 1000)))["flags"].tolist() == [0, W.ANCHORED, W.ANCHORED]    # clipped to the tree
    assert W.records(lab, anchor=((1, 0, 0), (0, 255, 255)))["flags"].tolist() == [0, 0, 0]                           # lo > hi: nothing
    assert W.island_of(lab, [[0, 4, 0], [0, 2, 0], [6, 6, 6]]).tolist() == [key(0, 3, 0), W.NO_ISLAND, key(6, 6, 6)]
    piece, rest = W.detach(g, lab, [key(0, 3, 0), key(6, 6, 6), key(0, 3, 0)])
    assert W.voxels(piece)[0].tolist() == [[0, 3, 0], [0, 4, 0], [6, 6, 6]] and W.voxels(piece)[1].tolist() == [2, 3, 4]
    assert W.voxels(rest)[0].tolist() == [[0, 0, 0], [0, 1, 0]] and W.voxels(rest)[1].tolist() == [0, 1]
    for bad in (key(0, 4, 0), key(0, 2, 0), 1 << 24):     # not the smallest voxel; empty; outside
        with pytest.raises(AssertionError):
            W.detach(g, lab, [bad])


def test_empty_full_and_checkerboard():
    assert len(W.records(W.label(np.zeros((256,) * 3, np.uint8)))) == 0
    rec = W.records(W.label(np.ones((8, 8, 8), np.uint8), W.FACES))
    assert rec["voxels"].tolist() == [512] and rec["sum"].tolist() == [[512 * 7 // 2] * 3]
    board = W.checkerboard(16)
    assert len(W.records(W.label(board, W.FACES))) == 16 ** 3 // 2
    assert W.records(W.label(board, W.CORNERS))["voxels"].tolist() == [16 ** 3 // 2]


def test_the_shared_scenes_are_what_they_claim():
    pairs, grid = W.cube_pairs()
    assert len(pairs) == 24
    for connectivity, column in ((W.FACES, 3), (W.CORNERS, 4)):
        lab = W.label(grid, connectivity)
        assert len(W.records(lab)) == sum(p[column] for p in pairs)
        for p in pairs:
            assert (lab[p[1]] == lab[p[2]]) == (p[column] == 1), p[0]
    for name, a, b, _, _ in pairs:    # cube A ends at the boundary on every axis, cube B lies across it on at least one
        m = 4 if "brick" in name else 16
        assert all((c + 2) % m == 0 for c in a) and ("root" in name or all((c + 2) % 16 == 8 for c in a))
        assert any(cb >= ca + 2 for ca, cb in zip(a, b))
    grid, path = W.snake()
    assert len({tuple(c) for c in (path >> 4).tolist()}) >= 8 and len({tuple(c) for c in (path >> 2).tolist()}) > 500
    assert set(np.abs(np.diff(path, axis=0)).sum(axis=1).tolist()) == {1}
    for connectivity in (W.FACES, W.CORNERS):
        rec = W.records(W.label(grid, connectivity))
        assert rec["voxels"].tolist() == [len(path)] and rec["sum"].tolist() == [path.sum(axis=0).tolist()]
        assert rec["lo"].tolist() == [path.min(axis=0).tolist()] and rec["hi"].tolist() == [path.max(axis=0).tolist()]
    grid, top = W.terrain()
    rec = W.records(W.label(grid, W.FACES), anchor=((0, 0, 0), (255, 0, 255)))
    assert rec["key"].tolist() == [0, key(*top)] and rec["flags"].tolist() == [W.ANCHORED, 0]
    assert rec["voxels"].tolist() == [256 * 128 * 256 + 20 * 22 * 20, 20 * 46 * 20]


@pytest.mark.parametrize("scene", ["sparse", "dense", "snake"])
def test_witness_equals_scipy(scene):
    ndimage = pytest.importorskip("scipy.ndimage")
    grid = {"sparse": lambda: W.random_fill(41, 0.05), "dense": lambda: W.random_fill(42, 0.30), "snake": lambda: W.snake()[0]}[scene]()
    for connectivity, structure in ((W.FACES, None), (W.CORNERS, np.ones((3, 3, 3)))):
        lab = W.label(grid, connectivity)
        theirs, n = ndimage.label(grid != 0, structure=structure)
        assert ((lab == W.NO_ISLAND) == (theirs == 0)).all()
        rec = W.records(lab)
        assert len(rec) == n
        # the two partitions are the same: every one of their labels maps to one key and back
        solid = grid != 0
        pairs = np.unique(np.stack([theirs[solid].astype(np.int64), lab[solid].astype(np.int64)]), axis=1)
        assert pairs.shape[1] == n and len(np.unique(pairs[0])) == n and len(np.unique(pairs[1])) == n
        # ... and a key is its island's smallest voxel
        xyz = np.argwhere(solid)
        keys = (xyz[:, 0] << 16) | (xyz[:, 1] << 8) | xyz[:, 2]
        smallest = np.full(n + 1, 1 << 30, np.int64)
        np.minimum.at(smallest, theirs[solid], keys)
        assert np.array_equal(np.sort(smallest[1:]), rec["key"].astype(np.int64))
        assert np.array_equal(ndimage.sum_labels(np.ones_like(theirs), theirs, np.arange(1, n + 1))[np.argsort(smallest[1:])].astype(np.int64),
                              rec["voxels"].astype(np.int64))
