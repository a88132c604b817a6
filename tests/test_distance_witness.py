"""tests/distance_witness.py held to the header's definition: an all-pairs brute force on small trees, and where scipy is installed its
exact Euclidean and chessboard transforms, capped; both metrics, R in {1, 3, 20}, with and without WALLS (for scipy: the input padded
with a shell of targets)."""
import numpy as np
import pytest

import distance_witness as W

RADII = (1, 3, 20)


def brute(grid, target, metric, max_radius, walls, palette=0):
    """the definition: every voxel against every target (and, under WALLS, against every voxel at coordinate -1 or n on some axis: a
    voxel further out has one of these between itself and the tree, nearer on every axis)"""
    t = W.targets(grid, target, palette)
    pad = 1 if walls else 0
    if walls:
        t = np.pad(t, pad, constant_values=True)
    tx = np.argwhere(t) - pad
    vx = np.argwhere(np.ones(grid.shape, bool))
    out = np.full(len(vx), W.FAR, np.int64)
    limit = W.limit_of(metric, max_radius)
    if len(tx):
        for s in range(0, len(vx), 256):
            d = np.abs(vx[s:s + 256, None, :] - tx[None, :, :])
            m = ((d * d).sum(axis=-1) if metric == W.EUCLIDEAN else d.max(axis=-1)).min(axis=1)
            out[s:s + 256] = np.where(m <= limit, m, W.FAR)
    return out.reshape(grid.shape).astype(np.uint16)


def small_grids():
    rng = np.random.default_rng(17)
    sparse = np.where(rng.random((11, 9, 12)) < 0.03, rng.integers(1, 4, (11, 9, 12)), 0).astype(np.uint8)
    yield "sparse", sparse
    dense = np.where(rng.random((10, 12, 9)) < 0.9, rng.integers(1, 4, (10, 12, 9)), 0).astype(np.uint8)
    yield "dense", dense
    one = np.zeros((12, 7, 10), np.uint8)
    one[0, 6, 3] = 2
    yield "one voxel", one
    yield "empty", np.zeros((6, 7, 8), np.uint8)
    yield "full", np.full((7, 6, 8), 2, np.uint8)


@pytest.mark.parametrize("walls", (False, True))
@pytest.mark.parametrize("metric", (W.EUCLIDEAN, W.CHEBYSHEV))
@pytest.mark.parametrize("name, grid", list(small_grids()), ids=lambda v: v if isinstance(v, str) else "")
def test_witness_is_the_definition(name, grid, metric, walls):
    for radius in RADII:
        for target in (W.TO_SOLID, W.TO_EMPTY, W.TO_MATERIAL):
            got = W.field(grid, target, metric, radius, walls, palette=1)
            assert np.array_equal(got, brute(grid, target, metric, radius, walls, palette=1)), (radius, target)


def test_both_ways_through_an_axis_agree():
    """the witness walks an axis slab by slab or shift by shift, by the number of slabs that hold something: the same field either way"""
    rng = np.random.default_rng(18)
    grid = np.zeros((70, 24, 24), np.uint8)
    grid[:, 4:20, 4:20] = rng.random((70, 16, 16)) < 0.05          # 70 slabs along x (shifts), 16 along y and z (slabs)
    for metric in (W.EUCLIDEAN, W.CHEBYSHEV):
        for radius in (3, 20):
            got = W.field(grid, W.TO_SOLID, metric, radius)
            swapped = W.field(np.ascontiguousarray(grid.transpose(1, 0, 2)), W.TO_SOLID, metric, radius).transpose(1, 0, 2)
            assert np.array_equal(got, swapped)
            crop = (slice(20, 44), slice(0, 24), slice(0, 24))
            inner = brute(grid, W.TO_SOLID, metric, radius, False)[crop]
            assert np.array_equal(got[crop], inner)


@pytest.mark.parametrize("walls", (False, True))
@pytest.mark.parametrize("radius", RADII)
def test_witness_against_scipy(radius, walls):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(19)
    grid = np.where(rng.random((40, 33, 36)) < 0.01, 3, 0).astype(np.uint8)
    for target in (W.TO_SOLID, W.TO_EMPTY):
        t = W.targets(grid, target)
        if walls:
            t = np.pad(t, 1, constant_values=True)
        inner = tuple(slice(1, -1) for _ in range(3)) if walls else tuple(slice(None) for _ in range(3))
        if not t.any():
            continue
        edt = np.rint(ndimage.distance_transform_edt(~t) ** 2).astype(np.int64)[inner]
        cdt = ndimage.distance_transform_cdt(~t, metric="chessboard").astype(np.int64)[inner]
        assert np.array_equal(W.field(grid, target, W.EUCLIDEAN, radius, walls), np.where(edt <= radius * radius, edt, W.FAR))
        assert np.array_equal(W.field(grid, target, W.CHEBYSHEV, radius, walls), np.where(cdt <= radius, cdt, W.FAR))


def test_result_at_and_apply():
    grid = np.zeros((8, 8, 8), np.uint8)
    grid[2, 3, 4] = 5
    values = W.field(grid, W.TO_SOLID, W.EUCLIDEAN, 2)
    r = W.result(values)
    assert (int(r["targets"]), int(r["near"]), int(r["far"])) == (1, 32, 512 - 33)          # the 33 voxels within distance 2 of a voxel
    assert int(r["largest"]) == 4 and int(r["largest_key"]) == W.key(0, 3, 4)             # (0, 3, 4), (2, 1, 4), ... all hold 4: the lowest key
    assert W.at(values, [(2, 3, 4), (3, 4, 4), (2, 3, 7)]).tolist() == [0, 2, W.FAR]
    grown, changed = W.apply(grid, values, 7, 1, 4)
    assert changed == 32 and np.count_nonzero(grown == 8) == 32 and grown[2, 3, 4] == 5
    assert W.apply(grid, values, 7, 5, 4)[1] == 0 and W.apply(grid, values, -1, 0, 0)[1] == 1
    none = W.result(W.field(np.zeros((4, 4, 4), np.uint8)))
    assert (int(none["targets"]), int(none["near"]), int(none["far"]), int(none["largest"]), int(none["largest_key"])) == (0, 0, 64, 0, W.NO_KEY)
    assert W.RESULT_DTYPE.itemsize == 32 and W.QUERY_DTYPE.itemsize == 32
