"""Model joints on the device (dust_hip_model_joints; the contract is in include/dust_hip.h). Every comparison is exact: the records must
be the witness's (tests/joints_witness.py), byte for byte, and under CELLS their faces must sum to the cut_faces of the device's own
Model.fracture records -- k_fracture_records, a kernel tested on its own. The inputs are the smallest at which k_joints can go wrong:
content across the brick edge 11 | 12 and the root-cell edge 15 | 16 on every axis, the tree's two corners, bricks that hold many pairs,
one pair spread over many workgroups, every one of the 32 385 material pairs (which a small region's first table cannot hold: the
table grows), and the one case a 32-bit sum fails."""
import ctypes as C

import numpy as np
import pytest

import fracture_witness as FW
import island_witness as IW
import joints_witness as W
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
FILL = 0x5A
ORIGIN = (9, 118, 201)


def host_model(grid, pal):
    return api.flatten_model(IW.to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def raw(model, group=L.JOINTS_MATERIALS, region=None, capacity=0, query=None, null_records=False, null_query=False, null_count=False):
    """the C call itself on records filled with 0x5A -> (status, n_joints, records): what the call leaves untouched shows"""
    q = L.JointQuery(struct_size=C.sizeof(L.JointQuery), group=group, palette=-1)
    lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
    q.lo[:], q.hi[:] = [int(v) for v in lo], [int(v) for v in hi]
    for name, value in (query or {}).items():
        if name == "reserved":
            q.reserved[:] = value
        else:
            setattr(q, name, value)
    records = np.full(max(capacity, 1) * 80, FILL, np.uint8).view(api.JOINT_DTYPE)
    n = C.c_uint32(0x5A5A5A5A)
    status = model._lib.dust_hip_model_joints(model._h, None if null_query else C.byref(q), None if null_count else C.byref(n),
                                              None if null_records else records.ctypes.data_as(C.c_void_p), capacity)
    return status, n.value, records


def ray_grid(n=8):
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def same(got, want):
    return len(got) == len(want) and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------- materials
def material_grids():
    """(block, every): a 10 x 9 x 11 block of all 255 palette indices at density 0.85 across 11 | 12 and 15 | 16 on every axis with
    voxel pairs of different materials at the tree's two corners along x, y and z; and a 64^3 block at 9..72 of uniformly random
    indices, which holds every one of the 32 385 pairs"""
    rng = np.random.default_rng(201)
    grid = np.zeros((256,) * 3, np.uint8)
    block = np.where(rng.random((10, 9, 11)) < 0.85, rng.integers(1, 256, (10, 9, 11)), 0)
    block.reshape(-1)[:255] = rng.permutation(255) + 1                           # every index at least once
    block[3, 3, 3] = 7                                                            # (12, 12, 12): the one-voxel region's voxel
    grid[9:19, 9:18, 9:20] = block
    grid[0, 0, 0], grid[1, 0, 0], grid[0, 1, 0], grid[0, 0, 1] = 2, 3, 4, 5
    grid[255, 255, 255], grid[254, 255, 255], grid[255, 254, 255], grid[255, 255, 254] = 255, 9, 10, 11
    every = np.zeros((256,) * 3, np.uint8)
    every[9:73, 9:73, 9:73] = rng.integers(1, 256, (64,) * 3)
    grid.setflags(write=False)
    every.setflags(write=False)
    return grid, every


GRIDS = {}


def shared(name):
    """the two material grids and the witness's records of the second, made once"""
    if not GRIDS:
        GRIDS["block"], GRIDS["every"] = material_grids()
        GRIDS["every_records"] = W.joints(GRIDS["every"], W.MATERIALS)
    return GRIDS[name]


REGIONS = (None, ((10, 13, 9), (17, 16, 18)), ((12, 12, 12), (12, 12, 12)), ((0, 0, 0), (255, 255, 255)), ((0, 0, 0), (255, 300, 1000)), ((13, 0, 0), (12, 255, 255)),
           ((256, 0, 0), (300, 255, 255)))


def check_materials(model, grid):
    for region in REGIONS:
        got, want = model.joints(L.JOINTS_MATERIALS, region), W.joints(grid, W.MATERIALS, region=region)
        assert same(got, want), region
        assert raw(model, region=region)[:2] == (L.OK, len(want))
    assert len(model.joints(L.JOINTS_MATERIALS, REGIONS[2])) == 0 == len(model.joints(L.JOINTS_MATERIALS, REGIONS[5]))


def test_materials_on_a_model_that_is_not_editable_and_on_one_that_is():
    grid = shared("block")
    pal = synth.make_palette(101)
    ctx = api.Context(device=0)
    origins, directions = ray_grid()
    fixed = make(ctx, grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(fixed, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    assert np.count_nonzero(hits["instance"] != L.NO_HIT) > 0
    source_bytes = [a.tobytes() for a in fixed.read()]
    check_materials(fixed, grid)
    whole = fixed.joints(L.JOINTS_MATERIALS)
    assert whole["lo2"].min(axis=0).tolist() == [1, 1, 1] and whole["hi2"].max(axis=0).tolist() == [511, 511, 511]       # the tree's two corners
    # CELLS needs what only an editable model holds
    assert raw(fixed, L.JOINTS_CELLS, capacity=4)[0] == L.ERR_NOT_READY
    # the model stays as it was created: not editable, the generation where it was -- the committed scene keeps answering
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()

    # the same model, now editable and read in place, an edit included
    fixed.set_voxels([(12, 12, 12), (11, 12, 12), (200, 3, 77), (200, 3, 78)], [9, -1, 254, 0])
    edited = grid.copy()
    edited[12, 12, 12], edited[11, 12, 12], edited[200, 3, 77], edited[200, 3, 78] = 10, 0, 255, 1
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    check_materials(fixed, edited)
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit was needed: the generation has not moved
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fixed.read(), host_model(edited, pal)))


# ---------------------------------------------------------------- cells
def check_cells(model, grid, lab, result, cells, region=None, identities=True):
    want = W.joints(grid, W.CELLS, lab, region)
    got = model.joints(L.JOINTS_CELLS, region)
    assert same(got, want), region
    if identities:                                                                # against the device's own fracture records
        inner = got[got["b"] != L.JOINT_REST]
        assert int(inner["faces"].sum()) == int(result["cut_faces"])
        for c in range(len(cells)):
            assert int(inner["faces"][(inner["a"] == c) | (inner["b"] == c)].sum()) == int(cells["cut_faces"][c]), c
    return got


def test_cells_on_a_solid_cube_with_and_without_a_limit():
    grid = np.zeros((256,) * 3, np.uint8)
    grid[4:28, 4:28, 4:28] = 1
    seeds = np.random.default_rng(11).integers(2, 30, (12, 3))
    pal = synth.make_palette(102)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for limit in (None, 60):
        result, cells = model.fracture(seeds, max_distance2=limit)
        lab, _ = FW.labels(grid, seeds, max_distance2=limit)
        assert cells.tobytes() == FW.cells(lab, 12).tobytes()
        got = check_cells(model, grid, lab, result, cells)
        rest = got[got["b"] == L.JOINT_REST]
        assert (len(rest) > 0) == (limit is not None) and len(got) > 12


def random_block(seed, size):
    """tests/test_gpu_fracture.py's block"""
    rng = np.random.default_rng(seed)
    grid = np.zeros((256,) * 3, np.uint8)
    x, y, z = ORIGIN
    grid[x:x + size[0], y:y + size[1], z:z + size[2]] = np.where(rng.random(size) < 0.5, rng.integers(1, 5, size), 0)
    return rng, grid


def test_cells_on_a_random_block_regions_a_filtered_fracture_and_two_runs():
    rng, grid = random_block(9, (33, 29, 35))
    seeds = np.concatenate([rng.integers(0, 30, (40, 3)) + np.array(ORIGIN), rng.integers(-200, 400, (20, 3))])
    pal = synth.make_palette(103)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    result, cells = model.fracture(seeds)
    lab, _ = FW.labels(grid, seeds)
    got = check_cells(model, grid, lab, result, cells)
    assert len(got) > 60 and L.JOINT_REST not in got["b"]
    cut = ((15, 120, 210), (30, 140, 228))
    check_cells(model, grid, lab, result, cells, region=cut, identities=False)
    check_cells(model, grid, lab, result, cells, region=((0, 0, 0), (255, 255, 255)))
    assert model.joints(L.JOINTS_CELLS).tobytes() == got.tobytes()                 # two runs give the same bytes
    assert model.joints(L.JOINTS_CELLS, capacity=7).tobytes() == got[:7].tobytes()
    # a fracture that used a palette filter: the other materials are the rest
    result, cells = model.fracture(seeds, palette=1)
    lab, _ = FW.labels(grid, seeds, palette=1)
    got = check_cells(model, grid, lab, result, cells)
    assert np.count_nonzero(got["b"] == L.JOINT_REST) > 0
    check_cells(model, grid, lab, result, cells, region=cut, identities=False)
    # ... and one that used a region: what lies outside it is the rest too
    result, cells = model.fracture(seeds, region=cut)
    lab, _ = FW.labels(grid, seeds, region=cut)
    got = check_cells(model, grid, lab, result, cells)
    assert np.count_nonzero(got["b"] == L.JOINT_REST) > 0


# ---------------------------------------------------------------- every pair, the capacity convention, the table's growth
def test_every_material_pair_capacities_growth_and_two_runs():
    grid, want = shared("every"), shared("every_records")
    assert len(want) == 255 * 254 // 2 == 32385                                   # the witness confirms: every pair is there
    pal = synth.make_palette(104)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    got = model.joints(L.JOINTS_MATERIALS)
    assert len(got) == 32385 and got.tobytes() == want.tobytes()
    assert model.joints(L.JOINTS_MATERIALS).tobytes() == got.tobytes()             # two runs give the same bytes
    # the block's own bounds: 125 root cells, a first table of 2048 slots, which 32 385 pairs overflow -- it is doubled five times
    tight = ((9, 9, 9), (72, 72, 72))
    assert model.joints(L.JOINTS_MATERIALS, tight).tobytes() == want.tobytes()
    part = ((9, 9, 9), (40, 72, 72))
    assert same(model.joints(L.JOINTS_MATERIALS, part), W.joints(grid, W.MATERIALS, region=part))
    # capacity 100: the first 100 records and not a byte more; capacity 0 counts, with or without an array
    status, n, records = raw(model, capacity=100)
    assert (status, n) == (L.OK, 32385) and records.tobytes() == want[:100].tobytes()
    padded = np.full(140 * 80, FILL, np.uint8)
    q = L.JointQuery(struct_size=C.sizeof(L.JointQuery), group=L.JOINTS_MATERIALS, palette=-1)
    q.hi[:] = [255, 255, 255]
    count = C.c_uint32()
    assert model._lib.dust_hip_model_joints(model._h, C.byref(q), C.byref(count), padded.ctypes.data_as(C.c_void_p), 100) == L.OK
    assert count.value == 32385 and padded[:8000].tobytes() == want[:100].tobytes() and np.all(padded[8000:] == FILL)
    status, n, records = raw(model, capacity=0)
    assert (status, n) == (L.OK, 32385) and np.all(records.view(np.uint8) == FILL)
    assert raw(model, capacity=0, null_records=True)[:2] == (L.OK, 32385)
    status, n, records = raw(model, capacity=32385 + 3)
    assert (status, n) == (L.OK, 32385) and records[:32385].tobytes() == want.tobytes() and np.all(records[32385:].view(np.uint8) == FILL)


# ---------------------------------------------------------------- one pair across workgroups
def test_one_pair_across_nine_root_cells_on_every_axis():
    pal = synth.make_palette(105)
    ctx = api.Context(device=0)
    for axis in range(3):
        grid, rec = W.slab_case(axis)
        got = make(ctx, grid, pal).joints(L.JOINTS_MATERIALS)
        assert len(got) == 1 and got[0].tobytes() == rec.tobytes()
        assert int(got[0]["faces"]) == 1600 == int(got[0]["by_face"][2 * axis])


# ---------------------------------------------------------------- the 64-bit sums
def test_sums_past_two_to_the_thirty_two_in_closed_form():
    """The whole tree in slabs one voxel thick along x, index 0 where x is even and index 1 where it is odd, the other way round in the
    layers y = 253 and y = 255. One family of parallel interfaces over the whole tree sums to 255 / 256 of 2^32; the three interfaces
    along y take sum2[z] past it. The pattern does not depend on z, so the record follows from the witness on one z layer."""
    pal = synth.make_palette(106)
    ctx = api.Context(device=0)
    model = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    odd, even = np.arange(1, 256, 2), np.arange(0, 256, 2)
    lo = [(0, 0, 0)] + [(x, 0, 0) for x in odd]
    hi = [(256, 256, 256)] + [(x + 1, 256, 256) for x in odd]
    index = [0] + [1] * 128
    for y in (253, 255):
        lo += [(x, y, 0) for x in even] + [(x, y, 0) for x in odd]
        hi += [(x + 1, y + 1, 256) for x in even] + [(x + 1, y + 1, 256) for x in odd]
        index += [1] * 128 + [0] * 128
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, lo, hi, op=L.EDIT_FILL, palette=index))
    layer = np.zeros((256, 256, 1), np.uint8)
    layer[:, :, 0] = 1 + (np.arange(256)[:, None] & 1)
    layer[:, 253, 0] = layer[:, 255, 0] = 2 - (np.arange(256) & 1)
    one = W.joints(layer, W.MATERIALS)
    assert len(one) == 1 and int(one[0]["faces"]) == 255 * 256 + 3 * 256
    want = one[0].copy()
    want["faces"] *= 256
    want["by_face"] *= 256
    want["sum2"][:2] *= 256
    want["sum2"][2] = int(one[0]["faces"]) * 65536                                # the sum of 2 z + 1 over 0..255
    want["lo2"][2], want["hi2"][2] = 1, 511
    assert int(want["sum2"][2]) == 4278190080 + 3 * 16777216 > 1 << 32
    xyz = [(0, 0, 0), (1, 0, 0), (0, 253, 9), (1, 255, 200), (255, 254, 255)]
    assert model.get_voxels(xyz).tolist() == [0, 1, 1, 0, 1]
    got = model.joints(L.JOINTS_MATERIALS)
    assert len(got) == 1 and got[0].tobytes() == want.tobytes()


# ---------------------------------------------------------------- state and refusals
def test_validity_refusals_and_the_model_is_only_read():
    rng, grid = random_block(12, (20, 18, 21))
    seeds = rng.integers(0, 20, (9, 3)) + np.array(ORIGIN)
    pal = synth.make_palette(107)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    points = [tuple(int(v) for v in p) for p in np.argwhere(grid != 0)[::97]]
    status, n, records = raw(model, L.JOINTS_CELLS, capacity=4)                   # before any fracture
    assert status == L.ERR_NOT_READY and n == 0x5A5A5A5A and np.all(records.view(np.uint8) == FILL) and b"fracture" in model._lib.dust_hip_last_error()
    islands = model.find_islands(L.ISLANDS_FACES)[1]
    model.distance(max_radius=3)
    model.flood([points[0]], medium=L.FLOOD_SOLID)
    result, cells = model.fracture(seeds, max_distance2=90)
    lab, _ = FW.labels(grid, seeds, max_distance2=90)
    keys, values, steps, labels = model.island_of(points), model.distance_at(points), model.flood_at(points), model.fracture_at(points)
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    origins, directions = ray_grid()
    hits = scene.trace_rays(origins, directions)
    check_cells(model, grid, lab, result, cells)
    assert same(model.joints(L.JOINTS_MATERIALS), W.joints(grid, W.MATERIALS))
    # the model was only read: labelling, fields and generation stand
    assert model.island_of(points).tolist() == keys.tolist() and model.distance_at(points).tolist() == values.tolist()
    assert model.flood_at(points).tolist() == steps.tolist() and model.fracture_at(points).tolist() == labels.tolist()
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()
    assert model.find_islands(L.ISLANDS_FACES)[1].tobytes() == islands.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))
    # every refusal leaves n_joints and the records as they were
    size = C.sizeof(L.JointQuery)
    refusals = [dict(query=dict(struct_size=size - 1)), dict(query=dict(struct_size=0)), dict(group=2), dict(group=0xFFFFFFFF), dict(query=dict(flags=1)),
                dict(query=dict(palette=0)), dict(query=dict(palette=254)), dict(query=dict(reserved=[1, 0])), dict(query=dict(reserved=[0, 7])),
                dict(null_query=True), dict(null_records=True)]
    for case in refusals:
        status, n, records = raw(model, capacity=4, **case)
        assert status == L.ERR_INVALID_ARGUMENT and n == 0x5A5A5A5A and np.all(records.view(np.uint8) == FILL), case
    status, _, records = raw(model, capacity=4, null_count=True)
    assert status == L.ERR_INVALID_ARGUMENT and np.all(records.view(np.uint8) == FILL)
    assert raw(model, query=dict(struct_size=size + 8), capacity=1)[0] == L.OK     # a larger struct of a later version is taken
    # a carving detach: the labelling stands, the records are the witness's on the carved grid
    model.fracture_detach([1, 4], receive=False)
    _, rest, lab_after = FW.detach(grid, lab, [1, 4])
    after = model.joints(L.JOINTS_CELLS)
    assert same(after, W.joints(rest, W.CELLS, lab_after)) and not np.any(np.isin(after["a"], [1, 4]) | np.isin(after["b"], [1, 4]))
    # an edit ends the cell field; MATERIALS goes on
    model.set_voxels([(1, 1, 1), (2, 1, 1)], [3, 4])
    status, n, records = raw(model, L.JOINTS_CELLS, capacity=4)
    assert status == L.ERR_NOT_READY and n == 0x5A5A5A5A and np.all(records.view(np.uint8) == FILL)
    edited = rest.copy()
    edited[1, 1, 1], edited[2, 1, 1] = 4, 5
    assert same(model.joints(L.JOINTS_MATERIALS), W.joints(edited, W.MATERIALS))
