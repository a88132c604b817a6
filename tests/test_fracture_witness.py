"""tests/fracture_witness.py held to statements that do not come from it: one seed owns everything; two seeds at an even distance
split at a plane that goes to the lower index, and swapping them swaps everything but that plane; a per-voxel pure-Python loop on a 10^3
world gives the same labels, cells, result, seams, detach and apply; the two sum identities; max_distance2 = 0 labels exactly the solid
voxels that are seeds."""
import itertools

import numpy as np

import fracture_witness as W


def small_world(seed, density=0.6, n=10):
    rng = np.random.default_rng(seed)
    grid = np.where(rng.random((n, n, n)) < density, rng.integers(1, 5, (n, n, n)), 0).astype(np.uint8)
    return rng, grid


def test_one_seed_labels_everything_zero():
    _, grid = small_world(1)
    for seed in ((4, 4, 4), (-1024, 1279, 0), (1279, 1279, 1279)):
        lab, far = W.labels(grid, [seed], scale=(16, 16, 16))
        assert ((lab == 0) == (grid != 0)).all() and (lab[grid == 0] == W.NO_CELL).all()
        r = W.result(grid, lab, far, n_seeds=1)
        assert int(r["solid"]) == int(r["labelled"]) == int(r["largest_voxels"]) == np.count_nonzero(grid) and int(r["cells"]) == 1
        assert int(r["cut_faces"]) == 0 and int(r["largest_cell"]) == 0 and not W.seams(lab).any()
        x, y, z = np.argwhere(grid != 0)[far[grid != 0].argmax()]
        assert int(r["max_d2"]) == 16 * ((x - seed[0]) ** 2 + (y - seed[1]) ** 2 + (z - seed[2]) ** 2) < 1 << 27


def test_two_seeds_at_an_even_distance_the_mid_plane_goes_to_the_lower_index():
    grid = np.ones((12, 9, 9), np.uint8)
    for axis in range(3):
        g = np.moveaxis(grid, 0, axis)
        a, b = [4, 4, 4], [4, 4, 4]
        a[axis], b[axis] = 2, 8                             # mid-plane at 5
        lab, _ = W.labels(g, [a, b])
        swapped, _ = W.labels(g, [b, a])
        along = np.moveaxis(lab, axis, 0)
        assert (along[:6] == 0).all() and (along[6:] == 1).all()
        plane = np.zeros(g.shape, bool)
        np.moveaxis(plane, axis, 0)[5] = True
        assert (swapped[plane] == 0).all() and (lab[plane] == 0).all()          # the plane: the lower index either way
        assert (swapped[~plane] == 1 - lab[~plane].astype(np.int64)).all()      # everything else swaps
        # one voxel thick seams, on the lower cell's side; each cut face once
        s = W.seams(lab)
        assert (np.moveaxis(s, axis, 0)[5]).all() and np.count_nonzero(s) == plane.sum()
        r = W.result(g, lab, W.labels(g, [a, b])[1], n_seeds=2)
        assert int(r["cut_faces"]) == plane.sum()
    # an odd distance has no tie: swapping swaps everything
    lab, _ = W.labels(grid, [(2, 4, 4), (7, 4, 4)])
    swapped, _ = W.labels(grid, [(7, 4, 4), (2, 4, 4)])
    assert (swapped == 1 - lab.astype(np.int64)).all()
    # a duplicate seed gets nothing
    lab, _ = W.labels(grid, [(2, 4, 4), (2, 4, 4), (8, 4, 4)])
    assert not (lab == 1).any() and (lab == 0).any() and (lab == 2).any()


def loop_labels(grid, seeds, region, palette, scale, limit):
    n = grid.shape[0]
    lab = np.full(grid.shape, W.NO_CELL, np.uint16)
    far = {}
    solid = 0
    lo, hi = region
    for x, y, z in itertools.product(range(n), repeat=3):
        if grid[x, y, z] == 0 or not all(l <= c <= min(h, 255) for c, l, h in zip((x, y, z), lo, hi)):
            continue
        if palette is not None and grid[x, y, z] != palette + 1:
            continue
        solid += 1
        best = None
        for i, s in enumerate(seeds):
            d2 = scale[0] * (x - s[0]) ** 2 + scale[1] * (y - s[1]) ** 2 + scale[2] * (z - s[2]) ** 2
            if best is None or (d2, i) < best:
                best = (d2, i)
        if best is not None and (limit is None or best[0] <= limit):
            lab[x, y, z] = best[1]
            far[(x, y, z)] = best[0]
    return lab, far, solid


def test_a_per_voxel_loop_on_a_small_world():
    for trial in range(6):
        rng, grid = small_world(10 + trial)
        n = grid.shape[0]
        seeds = [tuple(int(c) for c in s) for s in rng.integers(-3, n + 3, (7, 3))]
        seeds += [seeds[2], (-1024, 5, 1279)]
        region = ((0, 0, 0), (255, 255, 255)) if trial % 2 == 0 else ((1, 2, 0), (7, 8, 300))
        palette = None if trial < 3 else 2
        scale = [(1, 1, 1), (1, 16, 3), (5, 1, 2)][trial % 3]
        limit = None if trial % 3 == 0 else 9 * (trial + 1)
        lab, far = W.labels(grid, seeds, region, palette, scale, limit)
        want, want_far, solid = loop_labels(grid, seeds, region, palette, scale, limit)
        assert np.array_equal(lab, want) and (lab != W.NO_CELL).any()
        assert W.at(lab, [(1, 2, 3), (9, 9, 9)]).tolist() == [want[1, 2, 3], want[9, 9, 9]]
        # records, by loops over the labelled voxels and their six neighbours
        cells = [dict(voxels=0, cut=0, lo=[255] * 3, hi=[0] * 3, sum=[0] * 3) for _ in seeds]
        cut_once = 0
        seam = np.zeros(grid.shape, bool)
        for (x, y, z), d2 in want_far.items():
            c = cells[want[x, y, z]]
            c["voxels"] += 1
            for r, v in enumerate((x, y, z)):
                c["lo"][r], c["hi"][r], c["sum"][r] = min(c["lo"][r], v), max(c["hi"][r], v), c["sum"][r] + v
            for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                q = (x + dx, y + dy, z + dz)
                if all(0 <= v < n for v in q) and want[q] != W.NO_CELL and want[q] != want[x, y, z]:
                    c["cut"] += 1
                    if want[q] > want[x, y, z]:
                        cut_once += 1
                        seam[x, y, z] = True
        rec = W.cells(lab, len(seeds))
        for i, c in enumerate(cells):
            assert (int(rec["voxels"][i]), int(rec["cut_faces"][i])) == (c["voxels"], c["cut"])
            assert rec["lo"][i].tolist() == c["lo"] and rec["hi"][i].tolist() == c["hi"] and rec["sum"][i].tolist() == c["sum"]
            assert int(rec["reserved0"][i]) == int(rec["reserved1"][i]) == 0
        assert np.array_equal(W.seams(lab), seam)
        r = W.result(grid, lab, far, region, palette, len(seeds))
        sizes = [c["voxels"] for c in cells]
        assert int(r["solid"]) == solid and int(r["labelled"]) == len(want_far) and int(r["cut_faces"]) == cut_once
        assert int(r["cells"]) == sum(1 for v in sizes if v) and int(r["largest_voxels"]) == max(sizes) and int(r["largest_cell"]) == sizes.index(max(sizes))
        assert int(r["max_d2"]) == max(want_far.values())
        assert r["lo"].tolist() == [min(p[k] for p in want_far) for k in range(3)] and r["hi"].tolist() == [max(p[k] for p in want_far) for k in range(3)]
        assert not r["reserved"].any() and int(r["reserved0"]) == int(r["reserved1"]) == 0
        # the two identities
        assert int(rec["voxels"].sum()) == int(r["labelled"]) and int(rec["cut_faces"].sum()) == 2 * int(r["cut_faces"])
        assert int(rec["voxels"][8]) == 0                                     # the duplicate of seed 2
        # detach and apply
        which = [0, 3, 3, 8]
        piece, rest, after = W.detach(grid, lab, which)
        moved = np.isin(want, [0, 3])
        assert np.array_equal(piece != 0, moved) and np.array_equal(piece + rest, grid) and not (piece.astype(bool) & rest.astype(bool)).any()
        assert (after[moved] == W.NO_CELL).all() and np.array_equal(after[~moved], lab[~moved])
        for where, value in ((W.SEAMS, -1), (W.LABELLED, 7), (W.SEAMS, 1)):
            got, changed = W.apply(grid, lab, where, value)
            chosen = seam if where == W.SEAMS else want != W.NO_CELL
            byte = 0 if value < 0 else value + 1
            assert (got[chosen] == byte).all() and np.array_equal(got[~chosen], grid[~chosen]) and changed == np.count_nonzero(grid[chosen] != byte)


def test_empty_results_and_refusals():
    _, grid = small_world(3)
    for seeds, region in (([], None), ([(1, 1, 1)], ((5, 5, 5), (4, 9, 9))), ([(1, 1, 1)], ((0, 300, 0), (9, 400, 9)))):
        lab, far = W.labels(grid, seeds, region)
        r = W.result(grid, lab, far, region, None, len(seeds))
        assert (lab == W.NO_CELL).all() and int(r["labelled"]) == int(r["cells"]) == int(r["largest_voxels"]) == int(r["cut_faces"]) == int(r["max_d2"]) == 0
        assert int(r["largest_cell"]) == 0xFFFFFFFF and r["lo"].tolist() == [255] * 3 and r["hi"].tolist() == [0] * 3
        assert int(r["solid"]) == (np.count_nonzero(grid) if region is None else 0)       # n_seeds == 0: solid is still counted
        rec = W.cells(lab, len(seeds))
        assert not rec["voxels"].any() and (rec["lo"] == 255).all() and not rec["hi"].any() and not rec["sum"].any()
    assert not W.refused() and not W.refused(254, (16, 1, 16), seeds=[(-1024, 1279, 0)])
    for bad in (dict(palette=-2), dict(palette=255), dict(scale=(0, 1, 1)), dict(scale=(1, 17, 1)), dict(flags=1), dict(reserved0=1), dict(reserved=2),
                dict(seeds=[(0, 0, -1025)]), dict(seeds=[(1280, 0, 0)]), dict(seed_reserved=1)):
        assert W.refused(**bad), bad
    assert W.apply_refused(2, 0) and W.apply_refused(W.SEAMS, 255) and W.apply_refused(W.LABELLED, -2) and not W.apply_refused(W.SEAMS, -1)
    assert [W.SEED_DTYPE.itemsize, W.QUERY_DTYPE.itemsize, W.RESULT_DTYPE.itemsize, W.CELL_DTYPE.itemsize] == [16, 48, 64, 40]


def test_max_distance2_zero_labels_exactly_the_solid_voxels_that_are_seeds():
    rng, grid = small_world(5, density=0.5)
    seeds = [tuple(int(c) for c in s) for s in rng.integers(0, 10, (40, 3))] + [(-1, 0, 0), (10, 3, 3)]
    lab, far = W.labels(grid, seeds, max_distance2=0)
    first = {}
    for i, s in enumerate(seeds):
        first.setdefault(s, i)
    want = np.full(grid.shape, W.NO_CELL, np.uint16)
    for s, i in first.items():
        if all(0 <= c < 10 for c in s) and grid[s] != 0:
            want[s] = i
    assert np.array_equal(lab, want) and 0 < np.count_nonzero(lab != W.NO_CELL) < 40 and not far.any()
