"""The instance listing of the scene box kernels (box_query.hpp, list_instances), path by path, for overlap_boxes and sweep_boxes alike.
The other GPU tests never say which path a query took -- the grid cells, the group boxes of a LARGE scene, or the scan of every
instance box in id order -- so each case here is the smallest scene that reaches one, and it asserts its own premises: how many
instances meet the query (from the witness's boxes) and how many grid cells the query covers (from api.top_level_build on the same
boxes), each on the intended side of the kernel's thresholds (256 candidates, 512 cells) by a factor of two where the scene allows it
(a scene of 300 instances can put no more than 300 beyond the 256). Instances are axis-aligned (90-degree turns), so the exact
witnesses apply: Witness.exact of test_gpu_overlap.py and tests/sweep_witness.py."""
import numpy as np
import pytest

from dust_amd import api, scenes, synth
from sweep_witness import SweepWitness
from test_gpu_overlap import Witness, as_rows

pytestmark = pytest.mark.gpu

F = np.float32
NO_HIT = 0xFFFFFFFF
CAND, CELLS = 256, 512   # kBoxCand, kBoxGridCells

TURNS = [np.eye(3), np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]]), np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]]),
         np.array([[-1, 0, 0], [0, -1, 0], [0, 0, 1]]), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])]


def scene_of(centres, seed):
    """instances of ONE 8^3 model (its eight corners solid: the voxels' bounds are the model's), turned by 90 degrees, centred at `centres`"""
    rng = np.random.default_rng(seed)
    solid = rng.random((8, 8, 8)) < 0.3
    solid[::7, ::7, ::7] = True
    x, y, z = np.nonzero(solid)
    pal = synth.make_palette(seed)
    model = api.flatten_model(np.stack([x, y, z, rng.integers(0, 255, x.size)], axis=1).astype(np.uint8), (8, 8, 8), pal)
    instances = []
    for i, c in enumerate(np.asarray(centres, np.float64)):
        m = np.zeros((3, 4), F)
        m[:, :3] = TURNS[i % len(TURNS)]
        m[:, 3] = c - m[:, :3].astype(np.float64) @ np.full(3, 4.0)
        instances.append((0, m.reshape(12)))
    return scenes.SceneDesc([model], pal, instances)


def lattice(nx, ny, step, rng):
    """nx x ny centres on a plane, `step` apart, heights in quarter voxels (so that a plate coming down meets them at different times)"""
    gx, gy = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), rng.integers(-4, 5, nx * ny) * 0.25], axis=1)


def _line():
    return scene_of([(10.0 * i, 0.0, 0.0) for i in range(40)], 1)


def _cluster():   # every instance's box holds [0, 2]^3: centres within [-1, 3]^3
    return scene_of(np.random.default_rng(2).integers(-4, 13, (300, 3)) * 0.25, 2)


def _plane40():
    return scene_of(lattice(8, 5, 400.0, np.random.default_rng(3)), 3)


def _plane300():
    return scene_of(lattice(20, 15, 150.0, np.random.default_rng(4)), 4)


def _small_boxes():
    rng = np.random.default_rng(5)
    n = 24
    lo = np.stack([np.round(rng.uniform(-10.0, 395.0, n) * 2.0) / 2.0, np.round(rng.uniform(-8.0, 4.0, n) * 2.0) / 2.0,
                   np.round(rng.uniform(-8.0, 4.0, n) * 2.0) / 2.0], axis=1)
    size = rng.integers(1, 13, (n, 3)).astype(np.float64)
    d = rng.uniform(-15.0, 15.0, (n, 3))
    d[rng.random((n, 3)) < 0.25] = 0.0
    return lo, lo + size, d


# name -> (scene, the path's premises {"cells": "few" | "many", "meet": "few" | "over", "large": bool}, queries)
#   queries(wlo, whi) -> (overlap lo, hi), (sweep lo, hi, delta): the sweep's SWEPT box takes the same path as the overlap boxes
CASES = {
    "grid_listed": (_line, dict(cells="few", meet="few", large=False),
                    lambda wlo, whi: (_small_boxes()[:2], _small_boxes())),
    "grid_overflow_scan": (_cluster, dict(cells="few", meet="over", large=True),
                           lambda wlo, whi: ((np.zeros((1, 3)), np.full((1, 3), 2.0)),
                                             (np.zeros((2, 3)), np.full((2, 3), 2.0), np.array([[0.5, 0.25, 0.0], [-0.25, 0.5, 0.5]])))),
    "many_cells_scan": (_plane40, dict(cells="many", meet="all", large=False),
                        lambda wlo, whi: (((wlo - 5.0)[None], (whi + 5.0)[None]), plate(wlo, whi, wlo[1], whi[1]))),
    "groups_listed": (_plane300, dict(cells="many", meet="few", large=True),
                      lambda wlo, whi: ((np.array([[wlo[0] - 5.0, 100.0, -10.0]]), np.array([[whi[0] + 5.0, 350.0, 10.0]])),
                                        plate(wlo, whi, 100.0, 350.0))),
    "groups_overflow_scan": (_plane300, dict(cells="many", meet="over", large=True),
                             lambda wlo, whi: (((wlo - 5.0)[None], (whi + 5.0)[None]), plate(wlo, whi, wlo[1], whi[1]))),
}


def plate(wlo, whi, y0, y1):
    """a plate one voxel thick over x, [y0, y1] of the scene, above it, coming down through it (and the same going up from below)"""
    lo = np.array([[wlo[0] - 5.0, y0, whi[2] + 3.0], [wlo[0] - 5.0, y0, wlo[2] - 4.0]])
    hi = np.array([[whi[0] + 5.0, y1, whi[2] + 4.0], [whi[0] + 5.0, y1, wlo[2] - 3.0]])
    return lo, hi, np.array([[0.0, 0.0, -30.0], [0.0, 0.5, 30.0]])


def cells_covered(grid, lo, hi):
    dim = np.asarray(grid["dim"], np.int64)
    cl = np.clip(np.floor((np.asarray(lo, np.float64) - grid["lo"]) / grid["cell"]), 0, dim - 1)
    ch = np.clip(np.floor((np.asarray(hi, np.float64) - grid["lo"]) / grid["cell"]), 0, dim - 1)
    return int(np.prod(ch - cl + 1))


def check_premises(name, wit, lo, hi):
    """the path the listing takes for box [lo, hi], from the witness's boxes alone (no device)"""
    want = CASES[name][1]
    grid = api.top_level_build(wit.boxes)
    n = len(wit.boxes)
    assert (grid["n_groups"] > 0) == want["large"] and (n > 256) == want["large"], (name, n, grid["n_groups"])
    cells = cells_covered(grid, lo, hi)
    meet = int((np.all(wit.boxes[:, 3:] >= np.asarray(lo, F), axis=1) & np.all(wit.boxes[:, :3] <= np.asarray(hi, F), axis=1)).sum())
    if want["cells"] == "few":
        assert 2 * cells <= CELLS, (name, cells)
    else:
        assert cells >= 2 * CELLS and int(np.prod(grid["dim"])) > 2 * CELLS, (name, cells, grid["dim"])
    if want["meet"] == "few":
        assert 2 * meet <= CAND, (name, meet)
    elif want["meet"] == "over":
        assert meet > CAND, (name, meet)
    else:
        assert meet == n, (name, meet)
    return cells, meet


_built = {}


def built(name):
    make = CASES[name][0]
    if make not in _built:
        desc = make()
        _built[make] = (desc, Witness(desc), SweepWitness(desc))
    return _built[make]


def queries(name):
    desc, wit, swit = built(name)
    wlo, whi = wit.boxes[:, :3].min(0), wit.boxes[:, 3:].max(0)
    (olo, ohi), (slo, shi, d) = CASES[name][2](wlo, whi)
    return (np.asarray(olo, F), np.asarray(ohi, F)), (np.asarray(slo, F), np.asarray(shi, F), np.asarray(d, F))


def all_premises(name):
    desc, wit, swit = built(name)
    (olo, ohi), (slo, shi, d) = queries(name)
    out = [check_premises(name, wit, olo[i], ohi[i]) for i in range(len(olo))]
    for i in range(len(slo)):   # the swept box: the union of the box at t = 0 and t = 1 (float32, as the kernel forms it)
        out.append(check_premises(name, wit, np.minimum(slo[i], slo[i] + d[i]), np.maximum(shi[i], shi[i] + d[i])))
    return out


_scenes = {}


def device_scene(name):
    make = CASES[name][0]
    if make not in _scenes:
        ctx = api.Context(device=0)
        _scenes[make] = (ctx, scenes.hip_scene(ctx, built(name)[0]))
    return _scenes[make][1]


@pytest.mark.parametrize("name", list(CASES))
def test_listing_path(name):
    desc, wit, swit = built(name)
    all_premises(name)
    scene = device_scene(name)
    (olo, ohi), (slo, shi, d) = queries(name)
    # 1. overlap: counts and records are the witness's, in (instance, block, voxel) order
    want = [wit.exact(olo[i], ohi[i]) for i in range(len(olo))]
    counts, per = scene.overlap_boxes(olo, ohi, capacity=np.array([len(w) for w in want]))
    for i in range(len(olo)):
        assert counts[i] == len(want[i]), (i, counts[i], len(want[i]))
        assert np.array_equal(as_rows(per[i]), want[i]), i
    assert sum(len(w) for w in want) > 0
    # 2. a sweep that does not move agrees with the overlap result
    rest = scene.sweep_boxes(olo, ohi, np.zeros((len(olo), 3), F))
    assert np.array_equal(rest["instance"] != NO_HIT, counts > 0)
    assert np.all(rest["t"][counts > 0] == 0) and np.all(rest["t"][counts == 0] == 1)
    # 3. moving sweeps: whole records, byte for byte
    for ignore_start in (False, True):
        got = scene.sweep_boxes(slo, shi, d, ignore_start=ignore_start)
        for i in range(len(slo)):
            w = swit.exact(slo[i], shi[i], d[i], ignore_start=ignore_start)
            assert got[i].tobytes() == w.tobytes(), (i, ignore_start, got[i], w)
        if not ignore_start:
            assert (got["instance"] != NO_HIT).any()
