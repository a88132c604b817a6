"""tests/neighbour_witness.py against a plain triple loop over voxels and offsets, on grids of at most 12^3 (a grid is a tree of its own
size): the three neighbourhoods, walls on and off, a region, a hand-made tie, the fallback when nobody votes, generations up to a
fixed point, and the dtypes' sizes."""
import numpy as np
import pytest

import neighbour_witness as W


def loop_step(grid, neighbourhood, birth, survive, palette, majority, region, walls):
    """one generation voxel by voxel: (grid after, counts (2, 27), born, died, lo, hi)"""
    shape = grid.shape
    box = W.clip(grid, region)
    after = grid.copy()
    counts = np.zeros((2, W.BINS), np.uint32)
    born = died = 0
    lo, hi = [255] * 3, [0] * 3
    if box is None:
        return after, counts, 0, 0, lo, hi
    reach = {6: 1, 18: 2, 26: 3}[neighbourhood]
    for x in range(box[0][0], box[1][0] + 1):
        for y in range(box[0][1], box[1][1] + 1):
            for z in range(box[0][2], box[1][2] + 1):
                n, held = 0, []
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dz in (-1, 0, 1):
                            if not 1 <= abs(dx) + abs(dy) + abs(dz) <= reach:
                                continue
                            p = (x + dx, y + dy, z + dz)
                            if all(0 <= c < s for c, s in zip(p, shape)):
                                if grid[p]:
                                    n += 1
                                    held.append(int(grid[p]))
                            elif walls:
                                n += 1
                solid = grid[x, y, z] != 0
                counts[int(solid), n] += 1
                change = False
                if not solid and (birth >> n) & 1:
                    byte = palette + 1
                    if majority and held:
                        byte = min(set(held), key=lambda b: (-held.count(b), b))
                    after[x, y, z] = byte
                    born += 1
                    change = True
                if solid and not (survive >> n) & 1:
                    after[x, y, z] = 0
                    died += 1
                    change = True
                if change:
                    lo, hi = [min(a, b) for a, b in zip(lo, (x, y, z))], [max(a, b) for a, b in zip(hi, (x, y, z))]
    return after, counts, born, died, lo, hi


def random_grid(seed, shape, density, materials):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, materials + 1, shape), 0).astype(np.uint8)


RULES = {W.FACES: (W.count_mask(1, (4, 6)), W.count_mask((2, 6))), W.EDGES: (W.count_mask((7, 18)), W.count_mask((5, 18))),
         W.CORNERS: (W.count_mask((14, 26)), W.count_mask((13, 26)))}


@pytest.mark.parametrize("neighbourhood", W.NEIGHBOURHOODS)
@pytest.mark.parametrize("walls", [False, True])
def test_histogram_and_one_generation(neighbourhood, walls):
    birth, survive = RULES[neighbourhood]
    for seed, shape, density, region in ((1, (9, 12, 7), 0.5, None), (2, (12, 12, 12), 0.2, ((2, 0, 5), (9, 11, 6))), (3, (5, 6, 12), 0.9, ((4, 5, 11), (4, 5, 11))),
                                         (4, (8, 8, 8), 0.5, ((3, 3, 3), (2, 7, 7))), (5, (6, 6, 6), 0.0, None)):
        grid = random_grid(seed, shape, density, 4)
        for majority in (False, True):
            want_after, want_counts, born, died, lo, hi = loop_step(grid, neighbourhood, birth, survive, 9, majority, region, walls)
            result, counts = W.neighbours(grid, neighbourhood, birth, survive, region=region, walls=walls)
            assert np.array_equal(counts, want_counts), (seed, majority)
            assert (int(result["born"]), int(result["died"]), result["lo"].tolist(), result["hi"].tolist()) == (born, died, lo, hi)
            box = W.clip(grid, region)
            voxels = 0 if box is None else int(np.prod([h - l + 1 for l, h in zip(*box)]))
            assert int(result["voxels"]) == voxels == int(counts.sum()) and int(result["solid"]) == int(counts[1].sum())
            assert not counts[:, neighbourhood + 1:].any()
            after, applied, table, _ = W.apply(grid, neighbourhood, birth, survive, 1, 9, majority, region, walls)
            assert np.array_equal(after, want_after), (seed, majority)
            assert table.tolist() == [[born, died]] and int(applied["generations"]) == int(born + died > 0)
            assert (applied["lo"].tolist(), applied["hi"].tolist()) == (lo, hi)
        if box is None:
            assert result.tobytes() == W.zero_result().tobytes() and applied.tobytes() == W.zero_applied().tobytes()


def test_a_hand_made_tie_and_the_fallback():
    grid = np.zeros((5, 5, 5), np.uint8)
    grid[1, 2, 2], grid[3, 2, 2], grid[2, 1, 2], grid[2, 3, 2] = 7, 4, 4, 7           # two of byte 4 and two of byte 7 round (2, 2, 2)
    after, applied, _, info = W.apply(grid, W.FACES, W.count_mask(4), W.count_mask((0, 6)), palette=99, majority=True)
    assert after[2, 2, 2] == 4 and int(applied["born"]) == 1 and info == {"ties": 1, "voted_by_two": 1, "fallback": 0}
    grid[2, 2, 1] = 7                                                                # ... a third 7 breaks the tie
    after, _, _, info = W.apply(grid, W.FACES, W.count_mask(5), W.count_mask((0, 6)), palette=99, majority=True)
    assert after[2, 2, 2] == 7 and info["ties"] == 0
    # nobody votes: count 0 gives birth in an empty grid, and a corner voxel born from its three walls alone
    empty = np.zeros((3, 3, 3), np.uint8)
    after, applied, _, info = W.apply(empty, W.CORNERS, 1, 0, palette=5, majority=True)
    assert np.all(after == 6) and int(applied["born"]) == 27 and info["fallback"] == 27
    after, applied, _, info = W.apply(empty, W.FACES, W.count_mask(3), 0, palette=5, majority=True, walls=True)
    assert np.count_nonzero(after) == 8 and after[0, 0, 0] == after[2, 2, 2] == after[0, 2, 0] == 6 and info["fallback"] == 8
    assert np.array_equal(after, loop_step(empty, W.FACES, W.count_mask(3), 0, 5, True, None, True)[0])


def test_generations_up_to_a_fixed_point():
    grid = random_grid(11, (10, 11, 12), 0.5, 3)
    birth, survive = W.count_mask(5, 6), W.count_mask((2, 6))
    after, applied, table, _ = W.apply(grid, W.FACES, birth, survive, 40, palette=1, majority=True, region=((1, 1, 1), (8, 9, 10)))
    now, rows = grid, []
    for g in range(40):
        now, _, born, died, _, _ = loop_step(now, W.FACES, birth, survive, 1, True, ((1, 1, 1), (8, 9, 10)), False)
        rows.append([born, died])
    last = max(g for g, row in enumerate(rows) if sum(row)) + 1
    assert np.array_equal(after, now) and table.tolist() == rows and 1 < last < 40 and int(applied["generations"]) == last
    assert not table[last:].any() and int(applied["born"]) == sum(r[0] for r in rows) and int(applied["died"]) == sum(r[1] for r in rows)
    assert int(applied["solid_before"]) == np.count_nonzero(grid[1:9, 1:10, 1:11]) and int(applied["solid_after"]) == np.count_nonzero(now[1:9, 1:10, 1:11])
    assert np.array_equal(after[0], grid[0]) and np.array_equal(after[:, :, 11], grid[:, :, 11])       # outside the region: untouched
    # the replicator never rests: every generation changes something
    seed = np.zeros((12, 12, 12), np.uint8)
    seed[5, 6, 7] = 3
    _, applied, table, _ = W.apply(seed, W.FACES, W.count_mask(1), 0, 5, palette=2)
    assert int(applied["generations"]) == 5 and (table.sum(axis=1) > 0).all()


def test_masks_offsets_refusals_and_layouts():
    assert W.count_mask((14, 26)) == sum(1 << n for n in range(14, 27)) and W.count_mask(5, 6) == 0x60 and W.count_mask() == 0
    assert [len(W.offsets(n)) for n in W.NEIGHBOURHOODS] == [6, 18, 26]
    assert W.QUERY_DTYPE.itemsize == 48 and W.RESULT_DTYPE.itemsize == 64 and W.APPLIED_DTYPE.itemsize == 64
    assert not W.refused(6, 3, 254, 0x7F, 0x7F, generations=256)
    for bad in (dict(neighbourhood=0), dict(neighbourhood=7), dict(neighbourhood=27), dict(flags=4), dict(palette=-1), dict(palette=255), dict(birth=1 << 7),
                dict(survive=1 << 7), dict(lo=(0, 256, 0)), dict(hi=(255, 255, 256)), dict(generations=0), dict(generations=257)):
        assert W.refused(**{"neighbourhood": 6, **bad}), bad
    assert W.refused(18, birth=1 << 19) and not W.refused(18, birth=1 << 18) and W.refused(26, survive=1 << 27) and not W.refused(26, survive=1 << 26)
