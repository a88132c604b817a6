"""The path the flood field and the distance field share on the device (dust_amd/csrc/grid.hpp, field.hpp): voxel addressing, the lookup
kernel and the apply kernel with its root-cell box. One 256^3 model whose solid voxels and flood seeds stand at coordinates drawn from
{0, 3, 4, 15, 16, 63, 64, 255} on each axis -- either side of a brick seam, of a root-cell seam and of the tree's edge -- with some off
the diagonal, so that an index formula with two axes swapped reads another voxel. Every expected value comes from
tests/flood_witness.py and tests/distance_witness.py; the counts written out as literals are the witnesses' own, computed when the test
was written, so a scene that degenerates (nothing changes, or everything does) cannot pass."""
import numpy as np
import pytest

import distance_witness as DW
import flood_witness as FW
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

BYTE = 6                                                             # the solid voxels' grid byte: palette index 5
DIAGONAL = (0, 3, 4, 15, 16, 63, 64)                                 # solid at (a, a, a)
OFF_DIAGONAL = ((3, 16, 255), (255, 3, 16), (16, 255, 3), (64, 0, 15), (4, 63, 0))
SEEDS = ((0, 0, 3), (3, 4, 15), (16, 15, 63), (64, 63, 255), (255, 255, 4), (15, 64, 16), (255, 16, 3))      # all empty
FACES = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)])


def scene():
    grid = np.zeros((256,) * 3, np.uint8)
    for a in DIAGONAL:
        grid[a, a, a] = BYTE
    for p in OFF_DIAGONAL:
        grid[p] = BYTE
    return grid


def coordinates():
    """the solid voxels, the seeds and their face neighbours inside the tree"""
    base = np.array([(a, a, a) for a in DIAGONAL] + list(OFF_DIAGONAL) + list(SEEDS))
    xyz = np.concatenate([base] + [base + f for f in FACES])
    return np.unique(xyz[np.all((xyz >= 0) & (xyz < 256), axis=1)], axis=0)


def host_model(grid, pal):
    return api.flatten_model(FW.to_xyzi(grid), (256, 256, 256), pal)


def same_bytes(model, grid, pal):
    return all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


@pytest.fixture(scope="module")
def made():
    grid, pal = scene(), synth.make_palette(61)
    ctx = api.Context(device=0)
    return ctx, api.Model(ctx, *host_model(grid, pal), pal), grid, pal


def test_both_fields_are_read_where_they_were_written(made):
    _, model, grid, _ = made
    xyz = coordinates()
    steps = FW.steps(grid, SEEDS, FW.EMPTY, max_steps=4)
    values = DW.field(grid, DW.TO_SOLID, DW.EUCLIDEAN, max_radius=3)
    want_steps, want_values = FW.at(steps, xyz), DW.at(values, xyz)
    assert len(xyz) == 119 and np.count_nonzero(want_steps == FW.UNREACHED) == 73 and np.count_nonzero(want_values == 0) == 12
    assert np.count_nonzero(want_steps != want_values) == 119       # a lookup that reads the other field cannot pass
    r = model.flood(SEEDS, max_steps=4)
    d = model.distance(max_radius=3)
    assert r.tobytes() == FW.result(steps).tobytes() and d.tobytes() == DW.result(values).tobytes()
    assert (int(r["reached"]), int(d["targets"]), int(d["near"])) == (663, 12, 925)
    got_steps, got_values = model.flood_at(xyz), model.distance_at(xyz)
    assert np.array_equal(got_steps, want_steps) and np.array_equal(got_values, want_values)
    assert not np.array_equal(got_steps, got_values)


# (name, seed, max_steps of the flood, region, max_steps of the apply, root cells the reached voxels span, voxels changed)
FLOOD_APPLIES = (
    ("inside one root cell", (4, 3, 4), 2, None, 2, ((0, 0, 0), (0, 0, 0)), 22),
    ("two cells along x", (15, 4, 4), 2, None, 2, ((0, 0, 0), (1, 0, 0)), 25),
    ("two cells along y", (4, 16, 3), 2, None, 2, ((0, 0, 0), (0, 1, 0)), 25),
    ("two cells along z", (3, 4, 63), 2, None, 2, ((0, 0, 3), (0, 0, 4)), 25),
    ("the corner cell, to voxel 255", (255, 255, 255), 3, None, 3, ((15, 15, 15), (15, 15, 15)), 20),
    ("unreached voxels inside the region", (64, 63, 64), 1, ((60, 60, 60), (68, 68, 68)), None, ((3, 3, 3), (4, 3, 4)), 6),
)


def test_flood_apply_visits_the_cells_of_the_reached_voxels(made):
    _, model, grid, pal = made
    grid = grid.copy()
    for i, (name, seed, max_steps, region, within, cells, count) in enumerate(FLOOD_APPLIES):
        steps = FW.steps(grid, [seed], FW.EMPTY, max_steps=max_steps, region=region)
        reached = np.argwhere(steps != FW.UNREACHED)
        assert [(reached.min(axis=0) >> 4).tolist(), (reached.max(axis=0) >> 4).tolist()] == [list(c) for c in cells], name
        if name.startswith("inside"):
            assert np.all((reached & 15) > 0) and np.all((reached & 15) < 15)      # strictly inside: no voxel on the cell's faces
        if region is not None:      # the sentinel stands inside the region, in cells the apply visits
            inside = steps[tuple(slice(a, b + 1) for a, b in zip(*region))]
            assert np.count_nonzero(inside == FW.UNREACHED) == 723
        after, want = FW.apply(grid, steps, 10 + i, within)
        assert want == count and np.count_nonzero(after != grid) == count, name      # some voxel changes, and only reached ones
        r = model.flood([seed], max_steps=max_steps, region=region)
        assert r.tobytes() == FW.result(steps, region).tobytes(), name
        assert model.flood_apply(10 + i, max_steps=within) == count, name
        assert same_bytes(model, after, pal), name
        grid = after
    made[2][...] = grid      # (the next test goes on from here)


def test_distance_apply_ranges(made):
    _, model, grid, pal = made
    grid = grid.copy()
    values = DW.field(grid, DW.TO_MATERIAL, DW.EUCLIDEAN, max_radius=3, palette=BYTE - 1)
    query = dict(target=L.DISTANCE_TO_MATERIAL, palette=BYTE - 1, max_radius=3)
    assert model.distance(**query).tobytes() == DW.result(values).tobytes()
    assert DW.apply(grid, values, 40, 5, 4)[1] == 0
    assert model.distance_apply(40, 5, 4) == 0 and same_bytes(model, grid, pal)            # lo > hi: nothing
    model.distance(**query)
    after, want = DW.apply(grid, values, 41, 0, 1)                                         # lo = 0: the targets too
    assert want == 76 and np.all(after[values == 0] == 42) and np.count_nonzero(values == 0) == 12
    assert model.distance_apply(41, 0, 1) == want and same_bytes(model, after, pal)
    grid = after
    values = DW.field(grid, DW.TO_MATERIAL, DW.EUCLIDEAN, max_radius=3, palette=41)
    assert model.distance(target=L.DISTANCE_TO_MATERIAL, palette=41, max_radius=3).tobytes() == DW.result(values).tobytes()
    after, want = DW.apply(grid, values, 43, 5, 0xFFFFFFFF)                                # hi = 0xFFFFFFFF: FAR stays out
    far = values == DW.FAR
    assert want == 1126 and np.count_nonzero(far) > 16_000_000 and np.array_equal(after[far], grid[far])
    assert model.distance_apply(43, 5, 0xFFFFFFFF) == want and same_bytes(model, after, pal)
