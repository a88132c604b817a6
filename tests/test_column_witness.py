"""The witness of the model columns (tests/column_witness.py) held to a plain per-voxel loop over small regions, written from the
header's sentences one column and one voxel at a time, and to two identities on random grids: the runs seen from a side are the exposed
faces of that side (tests/surface_witness.py, without walls), and layer k from the low side is layer n - 1 - k from the high side."""
import numpy as np
import pytest

import column_witness as W
import surface_witness as SW

SHAPE = (12, 10, 14)


def random_grid(seed, density, shape=SHAPE, materials=4):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, materials + 1, shape), 0).astype(np.uint8)


def loop_column(grid, face, palette, region, u, v):
    """the runs of one column as [(position, length, gap)], near end first, and the coordinates of its positions"""
    axis, from_high = W.side(face)
    lo, hi = region
    hi = tuple(min(h, n - 1) for h, n in zip(hi, grid.shape))
    coords = list(range(lo[axis], hi[axis] + 1))
    if from_high:
        coords.reverse()
    voxels = []
    for c in coords:
        p = [0, 0, 0]
        p[axis], p[W.U_AXIS[axis]], p[W.V_AXIS[axis]] = c, u, v
        voxels.append(tuple(p))
    runs, gap, position = [], 0, 0
    while position < len(voxels):
        byte = int(grid[voxels[position]])
        if byte != 0 if palette < 0 else byte == palette + 1:
            start = position
            while position < len(voxels) and (int(grid[voxels[position]]) != 0 if palette < 0 else int(grid[voxels[position]]) == palette + 1):
                position += 1
            runs.append((start, position - start, gap))
            gap = 0
        else:
            gap += 1
            position += 1
    return runs, voxels


def loop(grid, face, palette, region, layer):
    """(cells as nested lists of tuples, result fields as a dict, counts) column by column"""
    axis, _ = W.side(face)
    lo, hi = region
    hi = tuple(min(h, n - 1) for h, n in zip(hi, grid.shape))
    ua, va = W.U_AXIS[axis], W.V_AXIS[axis]
    cells, counts = [], [0] * 256
    r = dict(columns=0, hit=0, voxels=0, runs=0, depth_sum=0, nearest=None, farthest=None, lo=[255] * 3, hi=[0] * 3)
    for v in range(lo[va], hi[va] + 1):
        row = []
        for u in range(lo[ua], hi[ua] + 1):
            runs, voxels = loop_column(grid, face, palette, (lo, hi), u, v)
            r["columns"] += 1
            r["runs"] += len(runs)
            if layer >= len(runs):
                row.append((0, 255, 0, len(runs)))
                counts[0] += 1
                continue
            start, length, _ = runs[layer]
            x, y, z = voxels[start]
            index = int(grid[x, y, z]) - 1
            row.append((voxels[start][axis], index, length - 1, len(runs)))
            counts[1 + index] += 1
            r["hit"] += 1
            r["voxels"] += length
            r["depth_sum"] += start
            key = (x << 16) | (y << 8) | z
            if r["nearest"] is None or (start, key) < r["nearest"]:
                r["nearest"] = (start, key)
            if r["farthest"] is None or (-start, key) < r["farthest"]:
                r["farthest"] = (-start, key)
            r["lo"] = [min(a, b) for a, b in zip(r["lo"], (x, y, z))]
            r["hi"] = [max(a, b) for a, b in zip(r["hi"], (x, y, z))]
        cells.append(row)
    return cells, r, counts


def loop_apply(grid, value, face, where, depth, palette, region, layer):
    axis, _ = W.side(face)
    lo, hi = region
    hi = tuple(min(h, n - 1) for h, n in zip(hi, grid.shape))
    ua, va = W.U_AXIS[axis], W.V_AXIS[axis]
    out = grid.copy()
    for v in range(lo[va], hi[va] + 1):
        for u in range(lo[ua], hi[ua] + 1):
            runs, voxels = loop_column(grid, face, palette, (lo, hi), u, v)
            if layer >= len(runs):
                continue
            start, length, gap = runs[layer]
            span = range(start, start + min(depth, length)) if where == W.RUN else range(start - min(depth, gap), start)
            for position in span:
                out[voxels[position]] = 0 if value < 0 else value + 1
    return out, int(np.count_nonzero(out != grid))


WHOLE = ((0, 0, 0), (255, 255, 255))
REGIONS = [WHOLE, ((2, 1, 3), (9, 8, 10)), ((5, 0, 0), (5, 255, 255)), ((0, 4, 0), (255, 4, 255)), ((0, 0, 6), (255, 255, 6)), ((3, 3, 3), (3, 3, 3)),
           ((1, 2, 3), (11, 2, 3))]


@pytest.mark.parametrize("density", [0.15, 0.5, 0.9])
def test_against_a_per_voxel_loop(density):
    grid = random_grid(int(density * 100), density)
    hits = 0
    for k, region in enumerate(REGIONS):
        for face in W.FACES:
            for layer, palette in ((0, -1), (1, -1), (2, 1), (0, 3), (6, -1)):
                if (k + layer) % 2 and region is not WHOLE:                     # (half of the combinations on the cut regions)
                    continue
                result, cells, counts = W.columns(grid, face, palette, region, layer)
                want_cells, want, want_counts = loop(grid, face, palette, region, layer)
                assert cells.shape == (len(want_cells), len(want_cells[0])) and cells.tolist() == want_cells, (region, face, layer, palette)
                assert [int(result[n]) for n in ("columns", "hit", "voxels", "runs", "depth_sum")] == [want[n] for n in ("columns", "hit", "voxels", "runs", "depth_sum")]
                assert int(result["nearest_key"]) == (want["nearest"][1] if want["hit"] else W.NO_KEY)
                assert int(result["farthest_key"]) == (want["farthest"][1] if want["hit"] else W.NO_KEY)
                assert result["lo"].tolist() == want["lo"] and result["hi"].tolist() == want["hi"]
                assert not result["reserved"].any() and int(result["pad0"]) == int(result["pad1"]) == 0
                assert counts.tolist() == want_counts and int(counts.sum()) == int(result["columns"]) and int(counts[0]) == want["columns"] - want["hit"]
                hits += want["hit"]
    assert hits > 1000


@pytest.mark.parametrize("density", [0.3, 0.7])
def test_apply_against_a_per_voxel_loop(density):
    grid = random_grid(7 + int(density * 10), density)
    changed_in_all = 0
    cases = [(W.RUN, 1, 5, -1, 0), (W.RUN, 3, -1, -1, 0), (W.RUN, 256, -1, -1, 1), (W.GAP, 1, 6, -1, 0), (W.GAP, 256, 7, -1, 1), (W.GAP, 2, -1, 2, 0),
             (W.RUN, 2, 9, 1, 1), (W.GAP, 256, 0, 3, 0)]
    for k, (where, depth, value, palette, layer) in enumerate(cases):
        for face in W.FACES:
            region = REGIONS[(k + W.FACES.index(face)) % 2]
            got, changed = W.apply(grid, value, face, where, depth, palette, region, layer)
            want, want_changed = loop_apply(grid, value, face, where, depth, palette, region, layer)
            assert np.array_equal(got, want) and changed == want_changed, (where, depth, value, palette, layer, face)
            changed_in_all += changed
    assert changed_in_all > 1000
    same, changed = W.apply(grid, -1, W.POS_Y, W.GAP, 4)                         # clearing a gap of empty voxels changes nothing
    assert changed == 0 and np.array_equal(same, grid)
    assert W.apply(grid, 3, W.POS_Y, region=((4, 0, 0), (3, 9, 9)))[1] == 0      # lo > hi: legal, empty


def test_hand_counted_column():
    grid = np.zeros((1, 1, 16), np.uint8)
    grid[0, 0, [1, 2, 3, 6, 9, 10, 15]] = [1, 1, 2, 3, 2, 2, 4]
    result, cells, counts = W.columns(grid, W.NEG_Z)
    assert cells.tolist() == [[(1, 0, 2, 4)]] and int(result["runs"]) == 4 and int(result["depth_sum"]) == 1 and int(result["nearest_key"]) == 1
    assert W.columns(grid, W.POS_Z)[1].tolist() == [[(15, 3, 0, 4)]]
    assert W.columns(grid, W.POS_Z, layer=1)[1].tolist() == [[(10, 1, 1, 4)]]
    assert W.columns(grid, W.POS_Z, layer=4)[1].tolist() == [[(0, 255, 0, 4)]]
    assert W.columns(grid, W.NEG_Z, palette=1)[1].tolist() == [[(3, 1, 0, 2)]]  # 3, then 9..10: the voxels between are see-through
    assert W.columns(grid, W.NEG_Z, region=((0, 0, 2), (0, 0, 9)), layer=2)[1].tolist() == [[(9, 1, 0, 3)]]   # both ends cut: 2..3, 6, 9
    result, _, counts = W.columns(grid, W.POS_Z, region=((0, 0, 5), (0, 0, 4)))
    assert result.tobytes() == W.zero_result().tobytes() and not counts.any()
    assert W.apply(grid, 8, W.NEG_Z, W.GAP, 256, layer=2)[0][0, 0].tolist() == [0, 1, 1, 2, 0, 0, 3, 9, 9, 2, 2, 0, 0, 0, 0, 4]
    peeled, changed = W.apply(grid, -1, W.POS_Z, W.RUN, 1, layer=1)
    assert changed == 1 and np.array_equal(peeled, W.apply(grid, -1, W.NEG_Z, W.RUN, 256, region=((0, 0, 10), (0, 0, 12)))[0]) and peeled[0, 0, 10] == 0


@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
def test_runs_are_the_exposed_faces_of_the_side(density):
    grid = random_grid(40 + int(density * 100), density, (20, 18, 22))
    exposed = SW.exposure(grid, walls=False)
    for d, face in enumerate(W.FACES):
        result, cells, _ = W.columns(grid, face)
        assert int(result["runs"]) == int(cells["runs"].sum()) == np.count_nonzero(exposed & (1 << d)) > 0


@pytest.mark.parametrize("density", [0.1, 0.5])
def test_a_layer_from_the_low_side_is_one_from_the_high_side(density):
    grid = random_grid(50 + int(density * 100), density, (9, 24, 8))
    checked = 0
    for low, high in ((W.NEG_X, W.POS_X), (W.NEG_Y, W.POS_Y), (W.NEG_Z, W.POS_Z)):
        for region in (None, ((1, 2, 1), (7, 20, 6))):
            ups = [W.columns(grid, low, region=region, layer=k)[1] for k in range(13)]
            downs = [W.columns(grid, high, region=region, layer=k)[1] for k in range(13)]
            runs = ups[0]["runs"].astype(np.int64)
            assert np.array_equal(runs, downs[0]["runs"]) and runs.max() < 13
            for k in range(13):
                for v, u in np.argwhere(runs > k).tolist():
                    up, down = ups[k][v, u], downs[runs[v, u] - 1 - k][v, u]
                    assert int(down["palette"]) != 255 and int(up["length_minus_1"]) == int(down["length_minus_1"])
                    assert int(down["at"]) == int(up["at"]) + int(up["length_minus_1"])          # `at` moved to the run's other end
                    checked += 1
                assert np.all(ups[k]["palette"][runs <= k] == 255)
    assert checked > 500
