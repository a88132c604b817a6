"""tests/settle_witness.py, the vectorised numpy witness of the model settling, held to a plain per-voxel loop written from the header
text (include/dust_hip.h) on grids of at most 24^3, for all six sides; the conservation of every material's count; the descent identity
s(before) - s(after) == fall_sum + slid; and the three inputs whose outcome the feature's description gives."""
import itertools

import numpy as np
import pytest

import settle_witness as W


def loop_is_loose(byte, loose):
    return byte != 0 and (loose[(byte - 1) >> 5] >> ((byte - 1) & 31)) & 1 == 1


def region_of(grid, region):
    lo, hi = ((0, 0, 0), tuple(n - 1 for n in grid.shape)) if region is None else region
    return lo, hi


def loop_fall(grid, toward, loose, region):
    """one fall, voxel by voxel: a column is walked from the toward end, a fixed voxel raises the floor, a loose one lands on the pile"""
    out = grid.copy()
    lo, hi = region_of(grid, region)
    axis, high = W.side(toward)
    others = [r for r in range(3) if r != axis]
    moved = fall_sum = fall_max = 0
    for a in range(lo[others[0]], hi[others[0]] + 1):
        for b in range(lo[others[1]], hi[others[1]] + 1):
            coords = range(hi[axis], lo[axis] - 1, -1) if high else range(lo[axis], hi[axis] + 1)
            cells = []
            for c in coords:
                p = [0, 0, 0]
                p[axis], p[others[0]], p[others[1]] = c, a, b
                cells.append(tuple(p))
            top = 0                                                                  # the position the next loose voxel comes to rest at
            for i, p in enumerate(cells):
                byte = int(grid[p])
                if byte == 0:
                    continue
                if not loop_is_loose(byte, loose):
                    top = i + 1
                    continue
                if top != i:
                    out[p] = 0
                    out[cells[top]] = byte
                    moved += 1
                    fall_sum += i - top
                    fall_max = max(fall_max, i - top)
                top += 1
    return out, moved, fall_sum, fall_max


def loop_slide(grid, toward, d, loose, region):
    """one slide, voxel by voxel, decided on `grid` and written into a copy"""
    out = grid.copy()
    lo, hi = region_of(grid, region)
    g = W.step(toward)

    def inside(p):
        return all(l <= c <= h for c, l, h in zip(p, lo, hi))

    def add(p, q):
        return tuple(a + b for a, b in zip(p, q))
    slid = 0
    for p in itertools.product(*(range(l, h + 1) for l, h in zip(lo, hi))):
        byte = int(grid[p])
        if not loop_is_loose(byte, loose):
            continue
        above, beside = add(p, tuple(-c for c in g)), add(p, d)
        below = add(beside, g)
        if inside(above) and grid[above] != 0:
            continue
        if not inside(beside) or not inside(below) or grid[beside] != 0 or grid[below] != 0:
            continue
        assert out[below] == 0                                                   # one possible source per destination
        out[below] = byte
        out[p] = 0
        slid += 1
    return out, slid


def random_grid(seed, shape, density, materials=5):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, materials + 1, shape), 0).astype(np.uint8)


REGIONS = (None, ((2, 3, 1), (17, 12, 20)), ((0, 0, 0), (0, 18, 22)), ((5, 5, 5), (5, 5, 5)))


@pytest.mark.parametrize("toward", W.FACES)
def test_fall_against_the_loop(toward):
    moved_any = 0
    for seed, density, loose in ((1, 0.3, W.loose_mask([0, 2, 4])), (2, 0.7, W.loose_mask([1])), (3, 0.5, W.ALL_LOOSE), (4, 0.4, W.loose_mask([]))):
        grid = random_grid(seed, (20, 19, 24), density)
        for region in REGIONS:
            box = W.clip(grid, region)
            got, record = W.fall(grid, toward, loose, box)
            want, moved, fall_sum, fall_max = loop_fall(grid, toward, loose, region)
            assert np.array_equal(got, want), (toward, seed, region)
            assert (record["moved"], record["fall_sum"], record["fall_max"]) == (moved, fall_sum, fall_max)
            assert record["changed"] == np.count_nonzero((grid != 0) != (want != 0))
            assert record["loose"] == np.count_nonzero(W.is_loose(grid[box], loose)) and record["loose"] + record["fixed"] == np.count_nonzero(grid[box])
            assert W.height_sum(grid, toward, loose, box) - W.height_sum(got, toward, loose, box) == fall_sum
            again, record = W.fall(got, toward, loose, box)                          # a fall leaves nothing to fall
            assert np.array_equal(again, got) and record["moved"] == 0 == record["changed"]
            result = W.settle(grid, toward, loose, region)
            assert int(result["moved"]) == moved and int(result["fall_sum"]) == fall_sum and int(result["fall_max"]) == fall_max
            moved_any += moved
    assert moved_any > 1000


@pytest.mark.parametrize("toward", W.FACES)
def test_slide_against_the_loop(toward):
    slid_any = 0
    for seed, density, loose in ((5, 0.15, W.loose_mask([0, 2, 4])), (6, 0.4, W.ALL_LOOSE), (7, 0.6, W.loose_mask([(0, 3)]))):
        grid = random_grid(seed, (13, 12, 14), density)
        for region in (None, ((1, 2, 1), (11, 9, 12)), ((0, 0, 0), (0, 11, 13))):
            for k in range(4):
                d = W.lateral(toward, k)
                got, slid, turned = W.slide(grid, toward, d, loose, W.clip(grid, region))
                want, want_slid = loop_slide(grid, toward, d, loose, region)
                assert np.array_equal(got, want) and slid == want_slid, (toward, seed, region, k)
                assert np.count_nonzero(turned) == 2 * slid
                slid_any += slid
    assert slid_any > 300
    axis, _ = W.side(toward)                                                         # +u, -u, +v, -v
    assert [W.lateral(toward, k) for k in range(4)] == [tuple((1 if k % 2 == 0 else -1) * (r == (W.U_AXIS, W.V_AXIS)[k // 2][axis]) for r in range(3)) for k in range(4)]


@pytest.mark.parametrize("toward", W.FACES)
def test_conservation_and_descent(toward):
    grid = random_grid(8, (14, 15, 16), 0.3, materials=6)
    loose = W.loose_mask([0, 1, 3, 5])
    for region in (None, ((1, 1, 1), (12, 13, 13))):
        box = W.clip(grid, region)
        after, applied, rows = W.apply(grid, toward, loose, 64, region, rest_within=64)
        assert np.array_equal(np.bincount(after.reshape(-1), minlength=8), np.bincount(grid.reshape(-1), minlength=8))
        fixed = (grid != 0) & ~W.is_loose(grid, loose)
        assert np.array_equal(np.where(fixed, grid, 0), np.where(fixed, after, 0))    # no fixed voxel moved, none was overwritten
        assert W.height_sum(grid, toward, loose, box) - W.height_sum(after, toward, loose, box) == int(applied["fall_sum"]) + int(applied["slid"])
        assert int(applied["slid"]) == int(rows[:, 0].sum()) > 0 and int(applied["fell"]) == int(rows[:, 1].sum())
        assert not rows[int(applied["generations"]):].any() and rows[int(applied["generations"]) - 1].any()
        # generation by generation, held to the loops; every material's count is conserved in every generation
        at, *_ = loop_fall(grid, toward, loose, region)
        for k in range(int(applied["generations"])):
            at, slid = loop_slide(at, toward, W.lateral(toward, k), loose, region)
            at, moved, _, _ = loop_fall(at, toward, loose, region)
            assert (slid, moved) == tuple(rows[k])
            assert np.array_equal(np.bincount(at.reshape(-1), minlength=8), np.bincount(grid.reshape(-1), minlength=8))
        assert np.array_equal(at, after)
        same, again, none = W.apply(after, toward, loose, 8, region)                  # at rest: a second apply moves nothing
        assert np.array_equal(same, after) and int(again["generations"]) == 0 and not none.any() and again["lo"].tolist() == [255] * 3
        shorter, record, _ = W.apply(grid, toward, loose, int(applied["generations"]), region)
        assert np.array_equal(shorter, after) and record.tobytes() == applied.tobytes()
        outside = np.ones(grid.shape, bool)                                          # outside the region nothing was changed
        outside[box] = False
        assert np.array_equal(after[outside], grid[outside])


def test_described_outcomes():
    """the tower of 12 is at rest after generation 13, the 4 x 8 x 4 block is a stepped pyramid after generation 30"""
    floor = np.zeros((40, 24, 40), np.uint8)
    floor[:, 0, :] = 1
    tower, block = floor.copy(), floor.copy()
    tower[20, 1:13, 20] = 2
    block[18:22, 1:9, 18:22] = 2
    loose = W.loose_mask([1])
    after, applied, _ = W.apply(tower, W.NEG_Y, loose, 64, rest_within=64)
    assert int(applied["generations"]) == 13 and int(applied["first_moved"]) == 0
    after, applied, _ = W.apply(block, W.NEG_Y, loose, 64, rest_within=64)
    assert int(applied["generations"]) == 30
    layers = (after[:, 1:, :] == 2).sum(axis=(0, 2))
    assert layers[:5].tolist() == [64, 40, 20, 4, 0] and all(a >= b for a, b in zip(layers, layers[1:]))
    rng = np.random.default_rng(9)
    fill = np.where(rng.random((12, 19, 12)) < 0.3, 2, 0).astype(np.uint8)
    after, applied, _ = W.apply(fill, W.NEG_Y, W.ALL_LOOSE, 64, rest_within=64)
    assert np.count_nonzero(after) == np.count_nonzero(fill)
    # at rest: no loose voxel has an empty voxel below it, or a free 45 degree step beside it
    for k in range(4):
        assert W.slide(after, W.NEG_Y, W.lateral(W.NEG_Y, k), W.ALL_LOOSE, W.clip(after, None))[1] == 0
    assert W.settle(after, W.NEG_Y)["moved"] == 0


def test_records_and_masks():
    assert W.RESULT_DTYPE.itemsize == 64 and W.APPLIED_DTYPE.itemsize == 64 and W.QUERY_DTYPE.itemsize == 72
    assert W.ALL_LOOSE == (0xFFFFFFFF,) * 7 + (0x7FFFFFFF,) and W.loose_mask([0, 33, (62, 65), 254]) == (1, 2 | (3 << 30), 3, 0, 0, 0, 0, 1 << 30)
    grid = np.zeros((6, 6, 6), np.uint8)
    empty = W.settle(grid, W.POS_X, region=((3, 0, 0), (2, 5, 5)))
    assert empty.tobytes() == W.zero_result().tobytes()
    whole = W.settle(grid, W.POS_X)
    assert int(whole["columns"]) == 36 and whole["lo"].tolist() == [255] * 3 and whole["hi"].tolist() == [0] * 3
    assert W.refused(3, 0, 0, (0,) * 3, (0,) * 3, W.ALL_LOOSE) and W.refused(4, 0, 0, (0,) * 3, (0, 256, 0), W.ALL_LOOSE)
    assert W.refused(4, 0, 0, (0,) * 3, (0,) * 3, (0,) * 7 + (1 << 31,)) and W.refused(4, 0, 0, (0,) * 3, (0,) * 3, W.ALL_LOOSE, 257)
    assert not W.refused(4, 0, 0, (9, 9, 9), (0, 0, 0), W.ALL_LOOSE, 256)
