"""The witness of the model deltas (tests/delta_witness.py) held to a plain per-voxel loop over 12^3 blocks -- three bricks per axis --
written from the header's sentences one voxel at a time, and to hand-counted cases."""
import itertools

import numpy as np
import pytest

import delta_witness as W


def pair(seed, density=0.5, change=0.4):
    rng = np.random.default_rng(seed)
    before = np.where(rng.random((12,) * 3) < density, rng.integers(1, 5, (12,) * 3), 0).astype(np.uint8)
    fresh = np.where(rng.random((12,) * 3) < density, rng.integers(1, 5, (12,) * 3), 0).astype(np.uint8)
    return before, np.where(rng.random((12,) * 3) < change, fresh, before).astype(np.uint8)


def loop(before, after, kinds, palette, region):
    """the same answer, voxel by voxel, in the list's order: cell, brick, voxel bit"""
    lo, hi = ((0, 0, 0), (11, 11, 11)) if region is None else region
    hi = tuple(min(h, 11) for h in hi)
    rows, solid = [], [0, 0]
    order = sorted(itertools.product(range(12), repeat=3),
                   key=lambda p: ([c // 16 for c in p], [c // 4 % 4 for c in p], [c % 4 for c in p]))
    for x, y, z in order:
        if not all(l <= c <= h for l, c, h in zip(lo, (x, y, z), hi)):
            continue
        a, b = int(before[x, y, z]), int(after[x, y, z])
        solid[0] += a != 0
        solid[1] += b != 0
        if a == b:
            continue
        kind = W.ADDED if a == 0 else W.REMOVED if b == 0 else W.REPAINTED
        if not kind & kinds or (palette >= 0 and palette + 1 not in (a, b)):
            continue
        rows.append(((x << 16) | (y << 8) | z, kind, a - 1 if a else 255, b - 1 if b else 255, a, b, (x, y, z)))
    return rows, solid


QUERIES = [(W.ALL, -1, None)] + [(k, -1, None) for k in range(1, 7)] + [(W.ALL, 2, None), (5, 0, None), (W.ALL, -1, ((2, 3, 1), (9, 6, 10))),
                                                                        (6, 3, ((5, 0, 0), (5, 255, 255))), (W.ALL, -1, ((4, 4, 4), (7, 7, 7)))]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_a_per_voxel_loop(seed):
    before, after = pair(seed)
    listed = 0
    for kinds, palette, region in QUERIES:
        result, voxels, counts = W.delta(before, after, kinds, palette, region)
        rows, solid = loop(before, after, kinds, palette, region)
        assert voxels["key"].tolist() == [r[0] for r in rows] and voxels["kind"].tolist() == [r[1] for r in rows]
        assert voxels["before"].tolist() == [r[2] for r in rows] and voxels["after"].tolist() == [r[3] for r in rows] and not voxels["reserved"].any()
        assert int(result["voxels"]) == len(rows)
        assert [int(result[n]) for n in ("added", "removed", "repainted")] == [sum(1 for r in rows if r[1] == bit) for bit in (1, 2, 4)]
        assert [int(result["solid_before"]), int(result["solid_after"])] == solid
        assert result["lo"].tolist() == [min((r[6][k] for r in rows), default=255) for k in range(3)]
        assert result["hi"].tolist() == [max((r[6][k] for r in rows), default=0) for k in range(3)]
        assert not result["reserved"].any() and int(result["pad0"]) == int(result["pad1"]) == 0
        for row, at in ((0, 4), (1, 5)):
            assert counts[row].tolist() == np.bincount([r[at] for r in rows], minlength=256).tolist()
        assert int(counts[0].sum()) == int(counts[1].sum()) == len(rows)
        assert int(counts[0, 0]) == int(result["added"]) and int(counts[1, 0]) == int(result["removed"])
        listed += len(rows)
    assert listed > 1000


def test_hand_counted_cases():
    before, after = np.zeros((12,) * 3, np.uint8), np.zeros((12,) * 3, np.uint8)
    before[3, 3, 3], after[3, 3, 3] = 2, 2                      # the same: not listed
    before[0, 0, 1] = 1                                         # removed
    after[11, 11, 11] = 4                                       # added
    before[4, 0, 0], after[4, 0, 0] = 1, 3                      # repainted
    result, voxels, counts = W.delta(before, after)
    assert voxels.tolist() == [(1, W.REMOVED, 0, 255, 0), (4 << 16, W.REPAINTED, 0, 2, 0), ((11 << 16) | (11 << 8) | 11, W.ADDED, 255, 3, 0)]
    assert [int(result[n]) for n in ("voxels", "added", "removed", "repainted", "solid_before", "solid_after")] == [3, 1, 1, 1, 3, 3]
    assert result["lo"].tolist() == [0, 0, 0] and result["hi"].tolist() == [11, 11, 11]
    assert counts[0].nonzero()[0].tolist() == [0, 1] and counts[0, 1] == 2 and counts[1].nonzero()[0].tolist() == [0, 3, 4]
    # the filter looks at both sides; the region at the voxel
    assert W.delta(before, after, palette=2)[1]["key"].tolist() == [4 << 16]
    assert W.delta(before, after, palette=0)[1]["key"].tolist() == [1, 4 << 16]
    assert W.delta(before, after, region=((4, 0, 0), (255, 255, 255)))[0]["voxels"] == 2
    inverted = W.delta(before, after, region=((5, 0, 0), (4, 255, 255)))
    assert inverted[0].tobytes() == W.zero_result().tobytes() and len(inverted[1]) == 0 and not inverted[2].any()
    same = W.delta(before, before)
    assert int(same[0]["voxels"]) == 0 and same[0]["lo"].tolist() == [255] * 3 and int(same[0]["solid_before"]) == 3


def test_apply_round_trip_conflicts_and_duplicates():
    before, after = pair(7)
    _, voxels, _ = W.delta(before, after)
    n = len(voxels)
    forward, changed, conflicts = W.apply(before, voxels)
    assert np.array_equal(forward, after) and (changed, conflicts) == (n, 0)
    back, changed, conflicts = W.apply(forward, voxels, backward=True)
    assert np.array_equal(back, before) and (changed, conflicts) == (n, 0)
    again, changed, conflicts = W.apply(after, voxels)
    assert np.array_equal(again, after) and (changed, conflicts) == (0, n)
    # a key named twice keeps its last record; the survivor is judged on the grid as it stood
    twice = np.zeros(3, W.VOXEL_DTYPE)
    twice["key"] = [5, 9, 5]
    twice["before"], twice["after"] = [W.NONE, 1, 7], [2, W.NONE, 3]
    grid = np.zeros((12,) * 3, np.uint8)
    grid[0, 0, 9] = 2
    out, changed, conflicts = W.apply(grid, twice)
    assert out[0, 0, 5] == 4 and out[0, 0, 9] == 0 and (changed, conflicts) == (2, 1)          # (0, 0, 5) was None, not index 7
    assert W.survivors(twice)["after"].tolist() == [W.NONE, 3]
    # the plain loop
    want = grid.copy()
    for key, _, b, a, _ in twice.tolist():
        want[key >> 16, (key >> 8) & 255, key & 255] = 0 if a == 255 else a + 1
    assert np.array_equal(out, want)
