"""tests/joints_witness.py held to independent statements: a per-face Python loop written from the header's sentences, the two identities
that tie the records to fracture's cut_faces (tests/fracture_witness.py), the symmetry under swapping two seeds' indices, and two
hand-made cases with closed forms."""
import numpy as np

import fracture_witness as FW
import joints_witness as W


def loop_joints(grid, group, labels=None, region=None):
    """the header, sentence by sentence, one face at a time"""
    box = W.clip(region)
    acc = {}
    if box is None:
        return acc
    lo, hi = box

    def group_of(p):
        if any(not 0 <= p[k] < grid.shape[k] for k in range(3)) or any(not lo[k] <= p[k] <= hi[k] for k in range(3)) or grid[p] == 0:
            return None                                                    # does not exist
        if group == W.MATERIALS:
            return int(grid[p]) - 1
        return W.REST if labels[p] == W.NO_CELL else int(labels[p])

    for p in map(tuple, np.argwhere(grid != 0)):
        g = group_of(p)
        if g is None:
            continue
        for r in range(3):
            q = tuple(p[k] + (k == r) for k in range(3))
            n = group_of(q)
            if n is None or n == g:
                continue
            a, b = min(g, n), max(g, n)
            direction = 2 * r + (1 if g == a else 0)                       # from the a voxel to the b voxel
            centre = [2 * p[k] + 1 + (k == r) for k in range(3)]
            rec = acc.setdefault((a, b), dict(faces=0, by_face=[0] * 6, lo2=[512] * 3, hi2=[0] * 3, sum2=[0] * 3))
            rec["faces"] += 1
            rec["by_face"][direction] += 1
            for k in range(3):
                rec["lo2"][k] = min(rec["lo2"][k], centre[k])
                rec["hi2"][k] = max(rec["hi2"][k], centre[k])
                rec["sum2"][k] += centre[k]
    return acc


def as_dict(records):
    return {(int(r["a"]), int(r["b"])): dict(faces=int(r["faces"]), by_face=r["by_face"].tolist(), lo2=r["lo2"].tolist(), hi2=r["hi2"].tolist(),
                                             sum2=[int(v) for v in r["sum2"]]) for r in records}


def ordered(records):
    keys = [(int(r["a"]), int(r["b"])) for r in records]
    return keys == sorted(keys) and len(set(keys)) == len(keys) and all(a < b for a, b in keys)


def small_block(seed, size=(7, 6, 8), at=(10, 13, 9), materials=5, density=0.8):
    rng = np.random.default_rng(seed)
    grid = np.zeros((32, 32, 32), np.uint8)
    x, y, z = at
    grid[x:x + size[0], y:y + size[1], z:z + size[2]] = np.where(rng.random(size) < density, rng.integers(1, materials + 1, size), 0)
    return rng, grid


def test_witness_against_a_per_face_loop():
    for seed in (1, 2):
        rng, grid = small_block(seed)
        labels = np.where(grid != 0, rng.integers(0, 6, grid.shape), W.NO_CELL).astype(np.uint16)
        labels[(grid != 0) & (rng.random(grid.shape) < 0.2)] = W.NO_CELL          # solid voxels of the rest
        for region in (None, ((11, 13, 10), (15, 17, 14)), ((12, 14, 11), (12, 14, 11)), ((0, 0, 0), (300, 255, 255)), ((13, 0, 0), (12, 255, 255))):
            for group in (W.MATERIALS, W.CELLS):
                got = W.joints(grid, group, labels, region)
                assert ordered(got) and as_dict(got) == loop_joints(grid, group, labels, region), (seed, region, group)
                assert np.all(got["by_face"].sum(axis=1) == got["faces"]) and not got["reserved0"].any() and not got["reserved1"].any()
        assert len(W.joints(grid, W.CELLS, labels)) > 0 and W.REST in W.joints(grid, W.CELLS, labels)["b"]
        assert len(W.joints(grid, W.MATERIALS, region=((12, 14, 11), (12, 14, 11)))) == 0


def test_fracture_identities():
    rng = np.random.default_rng(5)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[4:28, 4:28, 4:28] = 1
    seeds = np.random.default_rng(11).integers(2, 30, (12, 3))
    for limit in (None, 60):
        lab, far = FW.labels(grid, seeds, max_distance2=limit)
        got = W.joints(grid, W.CELLS, lab)
        cells, result = FW.cells(lab, len(seeds)), FW.result(grid, lab, far, n_seeds=len(seeds))
        inner = got[got["b"] != W.REST]
        assert int(inner["faces"].sum()) == int(result["cut_faces"]) > 0
        for c in range(len(seeds)):
            assert int(inner["faces"][(inner["a"] == c) | (inner["b"] == c)].sum()) == int(cells["cut_faces"][c]), c
        assert (W.REST in got["b"]) == (limit is not None)
    # a random block, a region that cuts it: only what exists inside the region shares faces
    _, block = small_block(3, size=(12, 11, 13), density=0.6)
    seeds = rng.integers(8, 24, (9, 3))
    lab, far = FW.labels(block, seeds)
    got = W.joints(block, W.CELLS, lab)
    assert int(got["faces"].sum()) == int(FW.face_counts(lab)[1].sum())


def test_swapping_two_seeds_swaps_a_and_b_and_mirrors_by_face():
    _, grid = small_block(4, size=(12, 11, 13), density=0.9)
    seeds = np.random.default_rng(6).integers(8, 24, (7, 3))
    lab, _ = FW.labels(grid, seeds, max_distance2=40)
    i, j = 1, 5
    swapped = lab.copy()
    swapped[lab == i], swapped[lab == j] = j, i
    before, after = as_dict(W.joints(grid, W.CELLS, lab)), as_dict(W.joints(grid, W.CELLS, swapped))
    turn = {i: j, j: i}
    want = {}
    for (a, b), rec in before.items():
        a2, b2 = turn.get(a, a), turn.get(b, b)
        rec = dict(rec)
        if a2 > b2:
            a2, b2 = b2, a2
            f = rec["by_face"]
            rec["by_face"] = [f[1], f[0], f[3], f[2], f[5], f[4]]
        want[(a2, b2)] = rec
    assert after == want and any(a == i or b == i for a, b in before) and (i, j) in before


def test_two_voxels_side_by_side_along_each_axis():
    for r in range(3):
        for low_first in (True, False):
            grid = np.zeros((256,) * 3, np.uint8)
            p = [200, 17, 254]
            p[r] = 254
            q = list(p)
            q[r] = 255
            grid[tuple(p)], grid[tuple(q)] = (4, 10) if low_first else (10, 4)       # palette indices 3 and 9
            got = W.joints(grid, W.MATERIALS)
            assert len(got) == 1
            rec = got[0]
            centre = [2 * p[k] + 1 + (k == r) for k in range(3)]
            by_face = [0] * 6
            by_face[2 * r + (1 if low_first else 0)] = 1
            assert (int(rec["a"]), int(rec["b"]), int(rec["faces"])) == (3, 9, 1) and rec["by_face"].tolist() == by_face
            assert rec["lo2"].tolist() == rec["hi2"].tolist() == [int(v) for v in rec["sum2"]] == centre


def test_two_layer_slab_in_closed_form():
    for axis in range(3):
        grid, rec = W.slab_case(axis)
        got = W.joints(grid, W.MATERIALS)
        assert len(got) == 1 and got[0].tobytes() == rec.tobytes() and int(got[0]["faces"]) == 1600
