"""Model bodies on the device (dust_hip_model_bodies; the contract is in include/dust_hip.h). Every comparison is exact: the records
must be the witness's (tests/body_witness.py), byte for byte, and under unit weights their voxels, bounds and first moments must be
those of find_islands, of fracture and of a whole-tree census -- three kernels tested on their own. The inputs are the smallest at
which k_bodies can go wrong: content across the brick edge 11 | 12 and the root-cell edge 15 | 16 on every axis, the tree's two
corners, bricks that hold several groups, groups that span root cells, weights 0 and 65535, and the one case a 32-bit sum fails."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import body_witness as W
import fracture_witness as FW
import island_witness as IW
import shape_edit_witness as SW
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
FILL = 0x5A


def host_model(grid, pal):
    return api.flatten_model(IW.to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


def raw(model, group=L.BODIES_ALL, weights=None, palette=-1, region=None, capacity=0, query=None, null_records=False):
    """the C call itself on records filled with 0x5A -> (status, n_bodies, records): what the call leaves untouched shows"""
    q = L.BodyQuery(struct_size=C.sizeof(L.BodyQuery), group=group, palette=palette)
    lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
    q.lo[:], q.hi[:] = [int(v) for v in lo], [int(v) for v in hi]
    for name, value in (query or {}).items():
        if name == "reserved":
            q.reserved[:] = value
        else:
            setattr(q, name, value)
    records = np.full(max(capacity, 1) * 96, FILL, np.uint8).view(api.BODY_DTYPE)
    n = C.c_uint32(0x5A5A5A5A)
    w = None if weights is None else np.ascontiguousarray(weights, np.uint16)
    status = model._lib.dust_hip_model_bodies(model._h, C.byref(q), None if w is None else w.ctypes.data_as(C.c_void_p), C.byref(n),
                                              None if null_records else records.ctypes.data_as(C.c_void_p), capacity)
    return status, n.value, records


def ray_grid(n=8):
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def random_weights(rng):
    weights = rng.integers(0, 65536, W.WEIGHTS)
    weights[rng.integers(0, 255, 6)] = 0
    weights[rng.integers(0, 255, 6)] = 65535
    weights[:4] = 0, 65535, 1, 40000
    return weights


# ---------------------------------------------------------------- all and materials
def materials_grid():
    """all 255 palette indices: a 10 x 9 x 11 block across 11 | 12 and 15 | 16 on every axis, a second block far away in another
    root cell row, and the tree's two corner voxels"""
    rng = np.random.default_rng(201)
    grid = np.zeros((256,) * 3, np.uint8)
    block = np.where(rng.random((10, 9, 11)) < 0.85, rng.integers(1, 256, (10, 9, 11)), 0)
    block.reshape(-1)[:255] = rng.permutation(255) + 1                           # every index at least once
    block[3, 3, 3] = 7                                                            # (12, 12, 12): the one-voxel region's voxel
    grid[9:19, 9:18, 9:20] = block
    grid[140:150, 77:83, 250:256] = np.where(rng.random((10, 6, 6)) < 0.5, rng.integers(1, 4, (10, 6, 6)), 0)
    grid[0, 0, 0], grid[255, 255, 255] = 2, 255
    grid.setflags(write=False)
    return grid


REGIONS = (None, ((10, 13, 9), (17, 16, 18)), ((12, 12, 12), (12, 12, 12)), ((0, 0, 0), (255, 255, 255)), ((13, 0, 0), (12, 255, 255)))


def check_all_and_materials(model, grid, weights):
    grid = W.voxel_list(grid)
    for w in (None, weights):
        for palette in (-1, 6):
            for region in REGIONS:
                for group, n in ((L.BODIES_ALL, 1), (L.BODIES_MATERIALS, 255)):
                    got = model.bodies(group, w, palette, region)
                    assert len(got) == n and got.tobytes() == W.bodies(grid, group, w, palette, region).tobytes(), (group, palette, region)


def test_all_and_materials_on_a_model_that_is_not_editable_and_on_one_that_is():
    grid = materials_grid()
    rng = np.random.default_rng(202)
    weights = random_weights(rng)
    pal = synth.make_palette(91)
    ctx = api.Context(device=0)
    origins, directions = ray_grid()

    fixed = make(ctx, grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(fixed, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    assert np.count_nonzero(hits["instance"] != L.NO_HIT) > 0
    source_bytes = [a.tobytes() for a in fixed.read()]
    check_all_and_materials(fixed, grid, weights)
    whole = fixed.bodies()[0]
    assert int(whole["voxels"]) == np.count_nonzero(grid) == int(whole["mass"]) and whole["lo"].tolist() == [0] * 3 and whole["hi"].tolist() == [255] * 3
    # a whole-tree census counts the same voxels: voxels, bounds and first moments byte for byte
    census = fixed.census(api.edit_shapes(L.SHAPE_BOX, (0, 0, 0), (256, 256, 256)), tables=False)[0][0]
    assert (int(census["solid"]), census["lo"].tobytes(), census["hi"].tobytes(), census["sum"].tobytes()) == \
        (int(whole["voxels"]), whole["lo"].tobytes(), whole["hi"].tobytes(), whole["m1"].tobytes())
    by_material = fixed.bodies(L.BODIES_MATERIALS, weights)
    assert by_material["key"].tolist() == list(range(255)) and np.all(by_material["voxels"] > 0)
    assert int(by_material["mass"].sum()) == int(fixed.bodies(L.BODIES_ALL, weights)[0]["mass"])
    # ISLANDS and CELLS need what only an editable model holds
    assert raw(fixed, L.BODIES_ISLANDS, capacity=4)[0] == L.ERR_NOT_READY and raw(fixed, L.BODIES_CELLS, capacity=4)[0] == L.ERR_NOT_READY
    # the model stays as it was created: not editable, the generation where it was -- the committed scene keeps answering
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()
    fixed.find_islands(L.ISLANDS_FACES, capacity=0)                               # the first-edit transition happens HERE, not in bodies
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY

    # the same model, now editable and read in place, an edit included
    fixed.set_voxels([(12, 12, 12), (11, 12, 12), (200, 3, 77)], [9, -1, 254])
    edited = grid.copy()
    edited[12, 12, 12], edited[11, 12, 12], edited[200, 3, 77] = 10, 0, 255
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    check_all_and_materials(fixed, edited, weights)
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit was needed: the generation has not moved
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fixed.read(), host_model(edited, pal)))


# ---------------------------------------------------------------- islands
def islands_grid():
    """thirteen islands under FACES: two interleaved inside one brick (planes x = 20 and x = 22 of brick 5, 5, 5) and a third between
    them in the brick next to it, an 8 x 8 plate over four root cells, a single voxel, a solid block of mixed materials across
    15 | 16, six small cubes of one material each, and the tree's far corner"""
    rng = np.random.default_rng(203)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[20, 20:24, 20:24], grid[22, 20:24, 20:24] = 1, 2
    grid[21, 20:23, 25], grid[23, 20, 20] = 3, 2                                  # (23, 20, 20) joins the x = 22 plane
    grid[12:20, 12:20, 40] = rng.integers(1, 5, (8, 8))
    grid[100, 100, 100] = 200
    grid[10:21, 60:66, 13:19] = rng.integers(1, 256, (11, 6, 6))
    for i in range(6):
        grid[60 + 10 * i:63 + 10 * i, 70:73, 80:83] = 10 + i
    grid[255, 255, 255] = 255
    grid.setflags(write=False)
    return grid


def test_islands_against_find_islands_capacities_detach_and_empty_islands():
    grid = islands_grid()
    rng = np.random.default_rng(204)
    weights = random_weights(rng)
    pal = synth.make_palette(92)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    labels = IW.label(grid)
    n, islands = model.find_islands(L.ISLANDS_FACES)
    assert n == 13 and islands.tobytes() == IW.records(labels).tobytes()
    keys = islands["key"].tolist()
    # unit weights: field for field find_islands' records
    plain = model.bodies(L.BODIES_ISLANDS)
    assert len(plain) == n
    for field, theirs in (("key", "key"), ("voxels", "voxels"), ("lo", "lo"), ("hi", "hi"), ("m1", "sum")):
        assert plain[field].tobytes() == islands[theirs].tobytes(), field
    assert plain.tobytes() == W.bodies(grid, W.ISLANDS, None, labels=labels).tobytes()
    weighted = model.bodies(L.BODIES_ISLANDS, weights)
    assert weighted.tobytes() == W.bodies(grid, W.ISLANDS, weights, labels=labels).tobytes()
    # capacity 0, 3 and all: the total whatever the capacity, the slots past it untouched
    status, total, records = raw(model, L.BODIES_ISLANDS, weights, capacity=0)
    assert (status, total) == (L.OK, n) and np.all(records.view(np.uint8) == FILL)
    status, total, records = raw(model, L.BODIES_ISLANDS, weights, capacity=0, null_records=True)
    assert (status, total) == (L.OK, n)
    status, total, records = raw(model, L.BODIES_ISLANDS, weights, capacity=3)
    assert (status, total) == (L.OK, n) and records.tobytes() == weighted[:3].tobytes()
    status, total, records = raw(model, L.BODIES_ISLANDS, weights, capacity=n + 4)
    assert (status, total) == (L.OK, n) and records[:n].tobytes() == weighted.tobytes() and np.all(records[n:].view(np.uint8) == FILL)
    # a region or a palette filter that empties an island leaves its zero record with its key
    for palette, region in ((-1, ((0, 0, 0), (21, 255, 255))), (1, None), (-1, ((16, 16, 30), (255, 255, 255))), (-1, ((9, 0, 0), (8, 255, 255)))):
        got = model.bodies(L.BODIES_ISLANDS, weights, palette, region)
        want = W.bodies(grid, W.ISLANDS, weights, palette, region, labels, keys)
        assert got.tobytes() == want.tobytes() and got["key"].tolist() == keys and np.count_nonzero(got["voxels"] == 0) > 0
    assert model.island_of([(22, 21, 21), (100, 100, 100)]).tolist() == [int(labels[22, 21, 21]), int(labels[100, 100, 100])]
    # after a detach of two islands the bodies are those of the remaining ones
    gone = [keys[2], keys[7]]
    model.detach_islands(gone, want_model=False)
    _, rest = IW.detach(grid, labels, gone)
    left = np.where(np.isin(labels, gone), W.NO_ISLAND, labels).astype(np.uint32)
    after = model.bodies(L.BODIES_ISLANDS, weights)
    assert len(after) == n - 2 and after["key"].tolist() == [k for k in keys if k not in gone]
    assert after.tobytes() == W.bodies(rest, W.ISLANDS, weights, labels=left).tobytes()
    again_n, again = model.find_islands(L.ISLANDS_FACES)
    assert again_n == n - 2 and again["key"].tobytes() == after["key"].tobytes()
    # an edit ends the labelling
    model.set_voxels([(1, 1, 1)], [3])
    assert raw(model, L.BODIES_ISLANDS, capacity=4)[0] == L.ERR_NOT_READY


# ---------------------------------------------------------------- cells
def test_cells_against_fracture_with_and_without_a_limit_and_after_a_detach():
    rng = np.random.default_rng(205)
    origin = np.array((9, 118, 201))
    grid = np.zeros((256,) * 3, np.uint8)
    grid[9:49, 118:158, 201:241] = np.where(rng.random((40,) * 3) < 0.5, rng.integers(1, 5, (40,) * 3), 0)
    weights = random_weights(rng)
    pal = synth.make_palette(93)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    assert raw(model, L.BODIES_CELLS, capacity=4)[0] == L.ERR_NOT_READY           # no fracture yet
    inside = rng.integers(0, 40, (14, 3)) + origin
    seeds = np.concatenate([inside[:9], inside[3:4], inside[9:], [(1200, -900, 700)]])      # seed 9 repeats seed 3, seed 15 is far away
    assert len(seeds) == 16
    for limit in (None, 150):
        _, cells = model.fracture(seeds, max_distance2=limit)
        lab, _ = FW.labels(grid, seeds, max_distance2=limit)
        assert cells.tobytes() == FW.cells(lab, 16).tobytes() and cells["voxels"][9] == 0 and cells["voxels"][15] == 0
        plain = model.bodies(L.BODIES_CELLS)
        assert len(plain) == 16 and plain["key"].tolist() == list(range(16))
        for field, theirs in (("voxels", "voxels"), ("lo", "lo"), ("hi", "hi"), ("m1", "sum")):
            assert plain[field].tobytes() == cells[theirs].tobytes(), field
        assert plain.tobytes() == W.bodies(grid, W.CELLS, None, labels=lab, keys=16).tobytes()
        assert (int(plain["voxels"].sum()) < np.count_nonzero(grid)) == (limit is not None)          # voxels that answer NO_CELL belong to no group
        for palette, region in ((-1, None), (2, ((20, 118, 201), (37, 140, 255)))):
            got = model.bodies(L.BODIES_CELLS, weights, palette, region)
            assert got.tobytes() == W.bodies(grid, W.CELLS, weights, palette, region, lab, 16).tobytes()
        status, total, records = raw(model, L.BODIES_CELLS, weights, capacity=5)
        assert (status, total) == (L.OK, 16) and records.tobytes() == W.bodies(grid, W.CELLS, weights, labels=lab, keys=16)[:5].tobytes()
    # a carving detach: the removed cells are zero records, the rest stand
    model.fracture_detach([1, 4], receive=False)
    _, rest, lab_after = FW.detach(grid, lab, [1, 4])
    after = model.bodies(L.BODIES_CELLS, weights)
    assert after.tobytes() == W.bodies(rest, W.CELLS, weights, labels=lab_after, keys=16).tobytes()
    assert after[1].tobytes() == W.zero_record(1).tobytes() and after[4].tobytes() == W.zero_record(4).tobytes()
    assert raw(model, L.BODIES_ISLANDS, capacity=4)[0] == L.ERR_NOT_READY


# ---------------------------------------------------------------- the 64-bit sums
def test_full_tree_of_the_heaviest_material_in_closed_form():
    """an empty model filled whole, every weight 65535: the sums a 32-bit accumulator fails, against closed forms"""
    pal = synth.make_palette(94)
    ctx = api.Context(device=0)
    model = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    assert model.edit_shapes(SW.shapes(SW.shape(SW.BOX, (-1e30,) * 3, (1e30,) * 3, op=SW.FILL, palette=254))).tolist() == [1 << 24]
    s1, s2 = sum(range(256)), sum(x * x for x in range(256))
    assert (s1, s2) == (32640, 5559680)
    for weights, w in ((np.full(255, 65535), 65535), (None, 1)):
        body = model.bodies(L.BODIES_ALL, weights)[0]
        assert int(body["key"]) == 0 and int(body["voxels"]) == 1 << 24 and body["lo"].tolist() == [0] * 3 and body["hi"].tolist() == [255] * 3
        assert int(body["mass"]) == w << 24
        assert [int(v) for v in body["m1"]] == [w * 65536 * s1] * 3
        assert [int(v) for v in body["m2"]] == [w * 65536 * s2] * 3 + [w * 256 * s1 * s1] * 3
    by_material = model.bodies(L.BODIES_MATERIALS, np.full(255, 65535))
    assert by_material[254].tobytes()[4:] == model.bodies(L.BODIES_ALL, np.full(255, 65535))[0].tobytes()[4:]
    assert by_material[:254].tobytes() == b"".join(W.zero_record(k).tobytes() for k in range(254))
    inner = model.bodies(L.BODIES_ALL, np.full(255, 65535), 254, ((3, 250, 17), (200, 255, 17)))[0]
    assert int(inner["voxels"]) == 198 * 6 and int(inner["m2"][2]) == 65535 * 198 * 6 * 17 * 17


# ---------------------------------------------------------------- state, refusals, determinism
def test_state_refusals_and_determinism():
    grid = islands_grid()
    rng = np.random.default_rng(206)
    weights = random_weights(rng)
    pal = synth.make_palette(95)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    points = [(22, 21, 21), (12, 12, 40), (100, 100, 100), (30, 30, 30), (255, 255, 255)]
    # before anything is labelled
    assert raw(model, L.BODIES_ISLANDS, capacity=4)[0] == L.ERR_NOT_READY and b"find_islands" in model._lib.dust_hip_last_error()
    assert raw(model, L.BODIES_CELLS, capacity=4)[0] == L.ERR_NOT_READY
    n, islands = model.find_islands(L.ISLANDS_FACES)
    model.distance(max_radius=3)
    model.flood([(30, 30, 30)], max_steps=60)
    seeds = [(15, 15, 40), (20, 62, 15), (70, 71, 81)]
    model.fracture(seeds)
    keys, values, steps, cells = model.island_of(points), model.distance_at(points), model.flood_at(points), model.fracture_at(points)
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    origins, directions = ray_grid()
    hits = scene.trace_rays(origins, directions)
    first = [model.bodies(group, w).tobytes() for group in (L.BODIES_ALL, L.BODIES_MATERIALS, L.BODIES_ISLANDS, L.BODIES_CELLS) for w in (None, weights)]
    second = [model.bodies(group, w).tobytes() for group in (L.BODIES_ALL, L.BODIES_MATERIALS, L.BODIES_ISLANDS, L.BODIES_CELLS) for w in (None, weights)]
    assert first == second                                                        # two runs give identical bytes
    # the model was only read: labelling, fields and generation stand
    assert model.island_of(points).tolist() == keys.tolist() and model.distance_at(points).tolist() == values.tolist()
    assert model.flood_at(points).tolist() == steps.tolist() and model.fracture_at(points).tolist() == cells.tolist()
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()
    assert model.find_islands(L.ISLANDS_FACES)[1].tobytes() == islands.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))
    # every refusal leaves n_bodies and the records as they were
    size = C.sizeof(L.BodyQuery)
    refusals = [dict(query=dict(struct_size=size - 1)), dict(query=dict(struct_size=0)), dict(group=4), dict(group=0xFFFFFFFF), dict(query=dict(flags=1)),
                dict(query=dict(reserved=[1, 0])), dict(query=dict(reserved=[0, 7])), dict(palette=-2), dict(palette=255),
                dict(region=((256, 0, 0), (255, 255, 255))), dict(region=((0, 0, 0), (255, 1000, 255))), dict(capacity=4, null_records=True)]
    for case in refusals:
        case.setdefault("capacity", 4)
        status, total, records = raw(model, weights=weights, **case)
        assert status == L.ERR_INVALID_ARGUMENT and total == 0x5A5A5A5A and np.all(records.view(np.uint8) == FILL), case
    assert raw(model, query=dict(struct_size=size + 8), capacity=1)[0] == L.OK     # a larger struct of a later version is taken
    # an edit ends the labelling and the cell field; ALL and MATERIALS go on
    model.set_voxels([(1, 1, 1)], [3])
    for group in (L.BODIES_ISLANDS, L.BODIES_CELLS):
        status, total, records = raw(model, group, capacity=4)
        assert status == L.ERR_NOT_READY and total == 0x5A5A5A5A and np.all(records.view(np.uint8) == FILL)
    edited = grid.copy()
    edited[1, 1, 1] = 4
    assert model.bodies(L.BODIES_ALL, weights).tobytes() == W.bodies(edited, W.ALL, weights).tobytes()


# ---------------------------------------------------------------- the helper on device records
def exact_properties(grid, weights, size):
    """mass, centre and tensor of a grid's voxels as solid cubes of side `size`, from the voxels themselves, in Fractions"""
    xyz = np.argwhere(grid != 0)
    w = [int(weights[int(g) - 1]) for g in grid[grid != 0]]
    s = Fraction(size)
    mass = sum(w)
    com = [sum(Fraction(2 * int(p[a]) + 1, 2) * m for p, m in zip(xyz, w)) / mass for a in range(3)]
    tensor = [[Fraction(0)] * 3 for _ in range(3)]
    for p, m in zip(xyz, w):
        r = [Fraction(2 * int(p[a]) + 1, 2) - com[a] for a in range(3)]
        for a in range(3):
            for b in range(3):
                tensor[a][b] += m * ((sum(v * v for v in r) + Fraction(1, 6) if a == b else 0) - r[a] * r[b])
    return mass, [c * s for c in com], [[v * s * s for v in row] for row in tensor]


def test_body_properties_of_device_records():
    pal = synth.make_palette(96)
    ctx = api.Context(device=0)
    weights = np.zeros(255, np.int64)
    weights[4], weights[9] = 2700, 700
    box = np.zeros((256,) * 3, np.uint8)
    box[14:19, 30:33, 15:17] = 5                                                  # 5 x 3 x 2 across 15 | 16
    ell = np.zeros((256,) * 3, np.uint8)
    ell[100:108, 50:52, 60:62], ell[100:102, 52:57, 60:62] = 5, 10                # an L of two materials
    for grid, size in ((box, 1.0), (ell, 0.125), (ell, 0.1)):
        records = make(ctx, grid, pal).bodies(L.BODIES_ALL, weights)
        assert records.tobytes() == W.bodies(grid, W.ALL, weights).tobytes()
        mass, com, inertia = api.body_properties(records, voxel_size=size)
        want_mass, want_com, want_tensor = exact_properties(grid, weights, size)
        assert mass[0] == want_mass and com[0].tolist() == [float(c) for c in want_com]
        assert inertia[0].tolist() == [[float(v) for v in row] for row in want_tensor]
    mass, com, inertia = api.body_properties(make(ctx, box, pal).bodies(L.BODIES_ALL, weights))
    M = Fraction(2700 * 30)
    assert [Fraction(inertia[0, k, k]) for k in range(3)] == [Fraction(float(M * v / 12)) for v in (3 * 3 + 2 * 2, 5 * 5 + 2 * 2, 5 * 5 + 3 * 3)]
