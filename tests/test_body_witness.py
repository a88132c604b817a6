"""The witness of the model bodies (tests/body_witness.py) held to a per-voxel loop in Python integers on a 12^3 crop and to identities:
unit weights give the island witness's sums, a translated piece moves its moments by the parallel-axis formulas, a solid box has the
textbook tensor through api.body_properties (compared as Fractions), and a record of mass 0 gives zeros. No device."""
from fractions import Fraction

import numpy as np

import body_witness as W
import island_witness as IW
from dust_amd import api


def _crop(seed=5, n=12, density=0.6):
    rng = np.random.default_rng(seed)
    grid = np.where(rng.random((n, n, n)) < density, rng.integers(1, 6, (n, n, n)), 0).astype(np.uint8)
    weights = rng.integers(0, 65536, W.WEIGHTS)
    weights[0], weights[1] = 0, 65535
    return grid, weights


def _loop(grid, group, weights, palette, region, labels, names):
    """the header text, one voxel at a time, Python ints only"""
    out = {k: dict(voxels=0, lo=[255] * 3, hi=[0] * 3, mass=0, m1=[0] * 3, m2=[0] * 6) for k in names}
    lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
    for x in range(grid.shape[0]):
        for y in range(grid.shape[1]):
            for z in range(grid.shape[2]):
                g = int(grid[x, y, z])
                p = (x, y, z)
                if g == 0 or any(p[r] < lo[r] or p[r] > hi[r] for r in range(3)) or (palette >= 0 and g != palette + 1):
                    continue
                key = 0 if group == W.ALL else g - 1 if group == W.MATERIALS else int(labels[x, y, z])
                if group == W.ISLANDS and key == W.NO_ISLAND or group == W.CELLS and key == W.NO_CELL:
                    continue
                w = 1 if weights is None else int(weights[g - 1])
                r = out[key]
                r["voxels"] += 1
                r["lo"] = [min(a, b) for a, b in zip(r["lo"], p)]
                r["hi"] = [max(a, b) for a, b in zip(r["hi"], p)]
                r["mass"] += w
                for a in range(3):
                    r["m1"][a] += w * p[a]
                for k, (a, b) in enumerate(W.PAIRS):
                    r["m2"][k] += w * p[a] * p[b]
    return out


def _same(records, loop):
    assert len(records) == len(loop)
    for r, (key, want) in zip(records, loop.items()):
        got = dict(voxels=int(r["voxels"]), lo=r["lo"].tolist(), hi=r["hi"].tolist(), mass=int(r["mass"]), m1=[int(v) for v in r["m1"]],
                   m2=[int(v) for v in r["m2"]])
        assert int(r["key"]) == key and got == want, (key, got, want)
        assert r["reserved0"] == 0 and r["reserved1"] == 0


def test_witness_equals_the_per_voxel_loop():
    grid, weights = _crop()
    labels = IW.label(grid)
    keys = sorted(int(k) for k in np.unique(labels[labels != W.NO_ISLAND]))
    rng = np.random.default_rng(6)
    cells = np.where(grid != 0, rng.integers(0, 5, grid.shape), W.NO_CELL).astype(np.uint16)
    cells[grid == 3] = W.NO_CELL                                           # counted voxels that belong to no group
    for w in (None, weights):
        for palette in (-1, 1):
            for region in (None, ((2, 3, 1), (9, 7, 11)), ((5, 5, 5), (5, 5, 5)), ((4, 0, 0), (3, 11, 11))):
                _same(W.bodies(grid, W.ALL, w, palette, region), _loop(grid, W.ALL, w, palette, region, None, [0]))
                _same(W.bodies(grid, W.MATERIALS, w, palette, region), _loop(grid, W.MATERIALS, w, palette, region, None, range(W.WEIGHTS)))
                _same(W.bodies(grid, W.ISLANDS, w, palette, region, labels), _loop(grid, W.ISLANDS, w, palette, region, labels, keys))
                _same(W.bodies(grid, W.CELLS, w, palette, region, cells, 7), _loop(grid, W.CELLS, w, palette, region, cells, range(7)))
    empty = W.bodies(grid, W.ISLANDS, weights, -1, ((4, 0, 0), (3, 11, 11)), labels)
    assert empty["key"].tolist() == keys and not empty["voxels"].any() and np.all(empty["lo"] == 255) and not empty["hi"].any()
    assert empty.tobytes() == b"".join(W.zero_record(k).tobytes() for k in keys)


def test_unit_weights_give_the_island_witness_sums():
    grid, _ = _crop(seed=8, density=0.3)
    labels = IW.label(grid, IW.CORNERS)
    islands = IW.records(labels)
    got = W.bodies(grid, W.ISLANDS, None, labels=labels)
    assert len(islands) > 3
    for field, theirs in (("key", "key"), ("voxels", "voxels"), ("lo", "lo"), ("hi", "hi"), ("m1", "sum")):
        assert np.array_equal(got[field], islands[theirs]), field
    assert np.array_equal(got["mass"], islands["voxels"])
    whole = W.bodies(grid, W.ALL)[0]
    assert int(whole["voxels"]) == int(islands["voxels"].sum()) and np.array_equal(whole["m2"], got["m2"].sum(axis=0))


def test_translation_moves_the_moments_by_the_parallel_axis_formulas():
    grid, weights = _crop(seed=9)
    t = (100, 7, 200)
    moved = np.zeros((256, 256, 256), np.uint8)
    moved[tuple(slice(o, o + 12) for o in t)] = grid
    for group in (W.ALL, W.MATERIALS):
        here, there = W.bodies(grid, group, weights), W.bodies(moved, group, weights)
        assert W.translate(here, t).tobytes() == there.tobytes()
    # and through the helper: the same tensor, the centre moved
    m0, c0, i0 = api.body_properties(W.bodies(grid, W.ALL, weights))
    m1, c1, i1 = api.body_properties(W.bodies(moved, W.ALL, weights))
    assert np.array_equal(m0, m1) and np.array_equal(i0, i1) and np.allclose(c1 - c0, t, rtol=0, atol=1e-9)


def test_solid_box_has_the_textbook_tensor():
    for (a, b, c), at, w, size in (((5, 3, 2), (0, 0, 0), 1, 1.0), ((7, 1, 4), (249, 3, 99), 65535, 0.25), ((1, 1, 1), (255, 255, 255), 3, 2.0)):
        grid = np.zeros((256, 256, 256), np.uint8)
        grid[at[0]:at[0] + a, at[1]:at[1] + b, at[2]:at[2] + c] = 9
        weights = np.zeros(W.WEIGHTS, np.int64)
        weights[8] = w
        mass, com, inertia = api.body_properties(W.bodies(grid, W.ALL, weights), voxel_size=size)
        M, s2 = Fraction(w * a * b * c), Fraction(size) ** 2
        assert Fraction(mass[0]) == M
        assert [Fraction(v) for v in com[0]] == [(Fraction(2 * o + n, 2)) * Fraction(size) for o, n in zip(at, (a, b, c))]
        want = [M * (b * b + c * c) / 12 * s2, M * (a * a + c * c) / 12 * s2, M * (a * a + b * b) / 12 * s2]
        assert [Fraction(inertia[0, k, k]) for k in range(3)] == [Fraction(float(v)) for v in want]
        assert not inertia[0][~np.eye(3, dtype=bool)].any()


def test_zero_mass_gives_zeros_and_products_have_their_sign():
    grid = np.zeros((8, 8, 8), np.uint8)
    grid[1, 2, 3] = grid[4, 4, 4] = 2
    records = W.bodies(grid, W.MATERIALS, np.zeros(W.WEIGHTS, np.int64))
    assert records[1]["voxels"] == 2 and records[1]["mass"] == 0 and records[1]["lo"].tolist() == [1, 2, 3]
    mass, com, inertia = api.body_properties(records)
    assert mass.shape == (255,) and com.shape == (255, 3) and inertia.shape == (255, 3, 3)
    assert not mass.any() and not com.any() and not inertia.any()
    # two unit voxels along the diagonal (0,0,0)-(1,1,1): C_ab = 1/2 for every pair, I_xy = -1/2, I_xx = 1/2 + 1/2 + 2/6
    pair = np.zeros((4, 4, 4), np.uint8)
    pair[0, 0, 0] = pair[1, 1, 1] = 1
    mass, com, inertia = api.body_properties(W.bodies(pair, W.ALL))
    assert mass[0] == 2 and com[0].tolist() == [1.0, 1.0, 1.0]
    assert inertia[0, 0, 1] == inertia[0, 1, 0] == inertia[0, 1, 2] == inertia[0, 0, 2] == -0.5
    assert [Fraction(inertia[0, k, k]) for k in range(3)] == [Fraction(float(Fraction(4, 3)))] * 3
    assert len(api.body_properties(records[:0])[0]) == 0


def test_refusals_of_the_witness():
    assert not W.refused()
    assert W.refused(group=4) and W.refused(flags=1) and W.refused(reserved=(0, 1)) and W.refused(palette=-2) and W.refused(palette=255)
    assert W.refused(region=((0, 0, 256), (255, 255, 255))) and W.refused(region=((0, 0, 0), (255, 256, 255)))
    assert not W.refused(region=((9, 0, 0), (3, 255, 255)))
