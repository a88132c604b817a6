"""Model neighbourhoods on the device (dust_hip_model_neighbours, dust_hip_model_neighbours_apply; the contract is in
include/dust_hip.h). Every comparison is exact: the result, the table, the applied record and its per-generation rows must be what the
witness says (tests/neighbour_witness.py), an apply must leave the model a host build of the witness's grid, and a read-only call must
leave the model as it found it."""
import ctypes as C
import functools

import numpy as np
import pytest

import neighbour_witness as W
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
HIERARCHY = ("root", "host_root", "mid", "dense_mask", "bmin", "bmax")
CAVE = (W.count_mask((14, 26)), W.count_mask((13, 26)))                              # the 4-5 rule of the 26 neighbourhood
RULES = {W.FACES: (W.count_mask(1, (4, 6)), W.count_mask((2, 6))), W.EDGES: (W.count_mask((7, 18)), W.count_mask((5, 18))), W.CORNERS: CAVE}


def host_model(grid, pal):
    return api.flatten_model(to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


def check(model, grid, neighbourhood, **query):
    """one read-only query on the device and in the witness: result and table agree; returns them"""
    result, counts = model.neighbours(neighbourhood, **query)
    want_result, want_counts = W.neighbours(grid, neighbourhood, **query)
    assert result.dtype == api.NEIGHBOURS_RESULT_DTYPE and counts.shape == (2, 27) and counts.dtype == np.uint32
    assert np.array_equal(counts, want_counts), (neighbourhood, query, counts, want_counts)
    assert result.tobytes() == want_result.tobytes(), (neighbourhood, query, result, want_result)
    assert int(counts[1].sum()) == int(result["solid"]) and int(counts[0].sum()) == int(result["voxels"]) - int(result["solid"])
    assert not counts[:, neighbourhood + 1:].any()
    alone, none = model.neighbours(neighbourhood, tables=False, **query)              # without the table: the same result
    assert alone.tobytes() == result.tobytes() and none is None
    return result, counts


def same_model(model, ctx, grid, pal):
    """the model is, byte for byte, a host build of `grid`"""
    fresh = make(ctx, grid, pal)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), fresh.read()))
    got, want = model.read_hierarchy(), fresh.read_hierarchy()
    assert got["n_mid"] == want["n_mid"] and got["extent_log2"] == want["extent_log2"]
    for name in HIERARCHY:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name


def check_apply(ctx, model, grid, pal, neighbourhood, birth, survive, generations=1, **rule):
    """one apply on the device and in the witness: the record, the rows and the model agree; returns the witness's answer"""
    applied, table = model.neighbours_apply(neighbourhood, birth, survive, generations, per_generation=True, **rule)
    after, want, want_table, info = W.apply(grid, neighbourhood, birth, survive, generations, **rule)
    assert applied.dtype == api.NEIGHBOURS_APPLIED_DTYPE and table.shape == (generations, 2) and table.dtype == np.uint32
    assert np.array_equal(table, want_table), (table[:12], want_table[:12])
    assert applied.tobytes() == want.tobytes(), (applied, want)
    same_model(model, ctx, after, pal)
    return after, want, want_table, info


def test_single_voxels():
    """(3, 15, 127) and (4, 16, 128) touch corner to corner, so the second has a model of its own; the 26 neighbours of each cross a
    brick edge, a root-cell edge and the 127 | 128 plane in every diagonal combination, or leave the tree"""
    pal = synth.make_palette(71)
    ctx = api.Context(device=0)
    first, second = np.zeros((256,) * 3, np.uint8), np.zeros((256,) * 3, np.uint8)
    for k, voxel in enumerate(((3, 15, 127), (0, 0, 0), (255, 255, 255), (0, 255, 128))):
        first[voxel] = 1 + k
    second[4, 16, 128] = 9
    for grid, inside, corners in ((first, 1, 3), (second, 1, 0)):
        model = make(ctx, grid, pal)
        for nb in W.NEIGHBOURHOODS:
            in_tree = {W.FACES: (3, 4), W.EDGES: (6, 9), W.CORNERS: (7, 11)}[nb]      # of a voxel in a corner of the tree, on an edge of it
            for walls in (False, True):
                result, counts = check(model, grid, nb, birth=W.count_mask(1), survive=0, walls=walls)
                assert int(result["solid"]) == inside + corners == int(result["died"])
                if not walls:                                                         # every voxel alone: count 0, and each neighbour sees exactly it
                    seen = inside * nb + (2 * in_tree[0] + in_tree[1] if corners else 0)
                    assert int(counts[1, 0]) == inside + corners and int(counts[0, 1]) == seen == int(result["born"]) and not counts[:, 2:].any()
            check(model, grid, nb, birth=W.count_mask(1), region=((2, 14, 126), (5, 17, 129)))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def test_solid_blocks():
    pal = synth.make_palette(72)
    ctx = api.Context(device=0)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[112:144, 112:144, 112:144], grid[0:20, 0:20, 0:20], grid[236:256, 236:256, 236:256] = 1, 2, 3
    model = make(ctx, grid, pal)
    sides = (32, 20, 20)
    for nb in W.NEIGHBOURHOODS:
        for walls in (False, True):
            _, counts = check(model, grid, nb, birth=RULES[nb][0], survive=RULES[nb][1], walls=walls)
            if walls:
                continue
            corner, edge, face, inner = {W.FACES: (3, 4, 5, 6), W.EDGES: (6, 9, 13, 18), W.CORNERS: (7, 11, 17, 26)}[nb]
            want = np.zeros(27, np.int64)
            for n in sides:
                want[corner] += 8
                want[edge] += 12 * (n - 2)
                want[face] += 6 * (n - 2) ** 2
                want[inner] += (n - 2) ** 3
            assert counts[1].tolist() == want.tolist()
    # under walls the two blocks in the tree's corners keep one free corner each, and have one with every neighbour solid
    _, counts = model.neighbours(W.CORNERS, walls=True)
    assert int(counts[1, 7]) == 8 + 2 and int(counts[1, 26]) == 30 ** 3 + 2 * 18 ** 3 + 2 * (1 + 3 * 18 + 3 * 18 ** 2)


@functools.lru_cache(maxsize=None)
def random_fill(density, materials):
    """a fill of [0, 64)^3 and one of [112, 144)^3, across 127 | 128"""
    rng = np.random.default_rng(int(density * 1000) + materials)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[:64, :64, :64] = np.where(rng.random((64,) * 3) < density, rng.integers(1, materials + 1, (64,) * 3), 0)
    grid[112:144, 112:144, 112:144] = np.where(rng.random((32,) * 3) < density, rng.integers(1, materials + 1, (32,) * 3), 0)
    grid.setflags(write=False)
    return grid


def ray_grid(n=8):
    """n * n rays along -x over the image of [0, 64)^3 under ROTATED"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


@pytest.mark.parametrize("density,materials", [(0.1, 3), (0.5, 6), (0.9, 4)])
def test_random_fills(density, materials):
    grid = random_fill(density, materials)
    pal = synth.make_palette(73)
    ctx = api.Context(device=0)
    lib = L.load()
    origins, directions = ray_grid()
    # a model that was never edited: read through the scratch masks, left as it was found, a scene committed on it keeps answering
    model = make(ctx, grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    source_bytes = [a.tobytes() for a in model.read()]
    changes = 0
    for nb in W.NEIGHBOURHOODS:
        result, _ = check(model, grid, nb, birth=RULES[nb][0], survive=RULES[nb][1])
        changes += int(result["born"]) + int(result["died"])
    assert changes > 1000
    check(model, grid, W.CORNERS, birth=CAVE[0], survive=CAVE[1], region=((5, 17, 30), (58, 40, 131)))          # cuts bricks on every axis
    check(model, grid, W.EDGES, birth=RULES[W.EDGES][0], survive=RULES[W.EDGES][1], region=((5, 17, 30), (58, 40, 131)), walls=True)
    result, counts = check(model, grid, W.CORNERS, birth=CAVE[0], survive=CAVE[1], region=((21, 22, 23), (21, 22, 23)))
    assert int(result["voxels"]) == 1 == int(counts.sum())
    # lo > hi: the zero result, bounds 255 / 0, the table's words as the call would leave an empty region
    q = model._neighbours_query(W.CORNERS, CAVE[0], CAVE[1], 0, 0, ((9, 9, 9), (8, 200, 200)))
    result = np.full(64, 0x5A, np.uint8).view(api.NEIGHBOURS_RESULT_DTYPE)
    counts = np.full(54, 0x5A5A5A5A, np.uint32)
    assert lib.dust_hip_model_neighbours(model._h, C.byref(q), result.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)) == L.OK
    assert result[0].tobytes() == W.zero_result().tobytes() and not counts.any()
    assert lib.dust_hip_model_neighbours(model._h, C.byref(q), None, None) == L.OK                               # every output may be null
    assert [a.tobytes() for a in model.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()          # no commit: the generation has not moved
    model.find_islands(L.ISLANDS_FACES, capacity=0)                                   # the first-edit transition happens HERE, not in neighbours
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY
    check(model, grid, W.CORNERS, birth=CAVE[0], survive=CAVE[1])                     # ... and the editable model answers the same


@functools.lru_cache(maxsize=None)
def half_fill():
    """a half-density six-material fill of [104, 152)^3, across 127 | 128"""
    rng = np.random.default_rng(74)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[104:152, 104:152, 104:152] = np.where(rng.random((48,) * 3) < 0.5, rng.integers(1, 7, (48,) * 3), 0)
    grid.setflags(write=False)
    return grid


@pytest.mark.parametrize("neighbourhood", W.NEIGHBOURHOODS)
@pytest.mark.parametrize("majority", [False, True])
def test_one_generation(neighbourhood, majority):
    grid = half_fill()
    pal = synth.make_palette(75)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    birth, survive = RULES[neighbourhood]
    asked, _ = model.neighbours(neighbourhood, birth=birth, survive=survive, tables=False)       # ask first ...
    after, want, _, info = check_apply(ctx, model, grid, pal, neighbourhood, birth, survive, 1, palette=200, majority=majority)
    assert int(asked["born"]) == int(want["born"]) > 1000 and int(asked["died"]) == int(want["died"]) > 1000       # ... apply after
    assert asked["lo"].tolist() == want["lo"].tolist() and asked["hi"].tolist() == want["hi"].tolist()
    if majority:                                                                                 # the vote was put to the test: ties, and more than one voter
        assert info["ties"] >= 1 and info["voted_by_two"] >= 1 and not np.any(after == 201)
    else:
        assert np.count_nonzero(after == 201) == int(want["born"])
    check(model, after, neighbourhood, birth=birth, survive=survive)


def test_both_buffers():
    """the replicator from a single voxel changes something in every generation: an odd and an even number of generations both leave
    the result in the model's own grid"""
    grid = np.zeros((256,) * 3, np.uint8)
    grid[3, 15, 127] = 4
    pal = synth.make_palette(76)
    ctx = api.Context(device=0)
    for generations in (2, 3, 5):
        model = make(ctx, grid, pal)
        _, want, table, _ = check_apply(ctx, model, grid, pal, W.FACES, W.count_mask(1), 0, generations, palette=7)
        assert int(want["generations"]) == generations and (table.sum(axis=1) > 0).all()
    model = make(ctx, grid, pal)                                                      # without the rows: the same record
    assert model.neighbours_apply(W.FACES, W.count_mask(1), 0, 5, palette=7).tobytes() == want.tobytes()


def test_fixed_point():
    rng = np.random.default_rng(77)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[8:56, 8:56, 8:56] = np.where(rng.random((48,) * 3) < 0.5, rng.integers(1, 4, (48,) * 3), 0)
    pal = synth.make_palette(77)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    birth, survive = W.count_mask(5, 6), W.count_mask((2, 6))
    after, want, table, _ = check_apply(ctx, model, grid, pal, W.FACES, birth, survive, 64, palette=3)
    assert 2 < int(want["generations"]) < 63 and not table[int(want["generations"]):].any()      # however seldom the library looks, it does not show
    # the same model again: nothing changes, and the generation is bumped all the same
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    origins, directions = ray_grid()
    scene.trace_rays(origins, directions)
    again, rows = model.neighbours_apply(W.FACES, birth, survive, 64, palette=3, per_generation=True)
    assert int(again["generations"]) == 0 and int(again["born"]) == int(again["died"]) == 0 and not rows.any()
    assert int(again["solid_before"]) == int(again["solid_after"]) == np.count_nonzero(after)
    assert again["lo"].tolist() == [255] * 3 and again["hi"].tolist() == [0] * 3
    same_model(model, ctx, after, pal)
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY


def test_region_and_walls_in_an_apply():
    pal = synth.make_palette(78)
    ctx = api.Context(device=0)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[10:21, 30, 30] = 5                                                           # a bar across the region's face x = 15 | 16
    grid[2, 2, 2], grid[250, 3, 250] = 8, 9
    region = ((0, 0, 0), (15, 255, 255))
    model = make(ctx, grid, pal)
    after, want, _, _ = check_apply(ctx, model, grid, pal, W.FACES, W.count_mask(1), W.count_mask((2, 6)), 1, palette=11, region=region)
    # inside: the bar's end at x = 10 dies (one neighbour), the one at x = 15 lives on its outside neighbour; outside nothing moves
    assert after[10, 30, 30] == 0 and after[15, 30, 30] == 5 and after[15, 31, 30] == 12 and after[16, 31, 30] == 0 and after[20, 30, 30] == 5
    assert after[250, 3, 250] == 9 and after[250, 4, 250] == 0 and int(want["hi"][0]) == 15
    # the tree's corner: three walls give birth under WALLS, and nobody votes -- the fallback; without WALLS nothing is born there
    corner = ((0, 0, 0), (7, 7, 7))
    for walls in (False, True):
        model = make(ctx, grid, pal)
        after, want, _, info = check_apply(ctx, model, grid, pal, W.FACES, W.count_mask(3), W.count_mask((0, 6)), 2, palette=20, majority=True, region=corner,
                                           walls=walls)
        assert (after[0, 0, 0] == 21) == walls and (int(want["born"]) > 0) == walls and after[2, 2, 2] == 8
        assert (info["fallback"] >= 1) == walls
    model = make(ctx, grid, pal)                                                      # the whole tree inside walls: every corner of it
    after, want, _, info = check_apply(ctx, model, grid, pal, W.FACES, W.count_mask(3), W.count_mask((0, 6)), 1, palette=20, majority=True, walls=True)
    assert int(want["born"]) == 8 == info["fallback"] and after[255, 255, 255] == after[0, 255, 0] == 21


def test_state():
    grid = random_fill(0.1, 3)
    pal = synth.make_palette(79)
    ctx = api.Context(device=0)
    origins, directions = ray_grid()
    points = [(13, 26, 14), (20, 30, 16), (200, 200, 200)]
    model = make(ctx, grid, pal)
    model.find_islands(L.ISLANDS_FACES, capacity=0)
    model.distance(max_radius=3)
    model.flood([(100, 100, 100)], max_steps=90)
    keys, values, steps = model.island_of(points), model.distance_at(points), model.flood_at(points)
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    # a read-only call moves no generation and leaves the labelling and both fields valid
    first = check(model, grid, W.CORNERS, birth=CAVE[0], survive=CAVE[1])
    second = check(model, grid, W.CORNERS, birth=CAVE[0], survive=CAVE[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))             # two calls, the same bytes
    assert model.island_of(points).tolist() == keys.tolist() and model.distance_at(points).tolist() == values.tolist()
    assert model.flood_at(points).tolist() == steps.tolist()
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()
    # an apply is an edit: the labelling and both fields are gone, and the scene needs a commit
    applied = model.neighbours_apply(W.CORNERS, CAVE[0], CAVE[1], 3, majority=True)
    assert int(applied["generations"]) >= 1
    assert status_of(lambda: model.island_of(points)) == L.ERR_NOT_READY and status_of(lambda: model.distance_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: model.flood_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY
    scene.commit()
    assert len(scene.trace_rays(origins, directions)) == len(hits)
    # two runs of the same apply on equal models give equal bytes
    twin = make(ctx, grid, pal)
    assert twin.neighbours_apply(W.CORNERS, CAVE[0], CAVE[1], 3, majority=True).tobytes() == applied.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), twin.read()))
    same_model(model, ctx, W.apply(grid, W.CORNERS, CAVE[0], CAVE[1], 3, majority=True)[0], pal)


def test_refusals_on_the_device_path():
    grid = random_fill(0.1, 3)
    pal = synth.make_palette(80)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    result = np.full(64, 0x5A, np.uint8).view(api.NEIGHBOURS_RESULT_DTYPE)
    applied = np.full(64, 0x5A, np.uint8).view(api.NEIGHBOURS_APPLIED_DTYPE)
    counts = np.full(54, 0x5A5A5A5A, np.uint32)
    rows = np.full(512, 0x5A5A5A5A, np.uint32)
    rp, ap, cp, gp = (a.ctypes.data_as(C.c_void_p) for a in (result, applied, counts, rows))

    def query(neighbourhood=26, flags=0, palette=0, birth=0, survive=0, lo=(0, 0, 0), hi=(255, 255, 255), size=C.sizeof(L.NeighboursQuery)):
        q = L.NeighboursQuery(struct_size=size, neighbourhood=neighbourhood, flags=flags, palette=palette, birth=birth, survive=survive)
        q.lo[:], q.hi[:] = lo, hi
        return q
    bad = [query(neighbourhood=0), query(neighbourhood=7), query(neighbourhood=27), query(flags=4), query(flags=1 << 31), query(palette=-1), query(palette=255),
           query(birth=1 << 27), query(survive=1 << 27), query(neighbourhood=6, birth=1 << 7), query(neighbourhood=18, survive=1 << 19), query(lo=(0, 256, 0)),
           query(hi=(255, 255, 256)), query(size=47), query(size=0)]
    for q in bad:
        assert lib.dust_hip_model_neighbours(model._h, C.byref(q), rp, cp) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_neighbours_apply(model._h, C.byref(q), 1, ap, gp) == L.ERR_INVALID_ARGUMENT
    for q in bad[:-2]:                                                                # ... and each of those is one the witness refuses too
        assert W.refused(q.neighbourhood, q.flags, q.palette, q.birth, q.survive, tuple(q.lo), tuple(q.hi))
    good = query(birth=CAVE[0], survive=CAVE[1])
    assert lib.dust_hip_model_neighbours(model._h, None, rp, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_neighbours(None, C.byref(good), rp, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_neighbours_apply(model._h, None, 1, ap, gp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_neighbours_apply(None, C.byref(good), 1, ap, gp) == L.ERR_INVALID_ARGUMENT
    for generations in (0, 257, 0xFFFFFFFF):
        assert lib.dust_hip_model_neighbours_apply(model._h, C.byref(good), generations, ap, gp) == L.ERR_INVALID_ARGUMENT
    assert result.tobytes() == b"\x5a" * 64 and applied.tobytes() == b"\x5a" * 64 and np.all(counts == 0x5A5A5A5A) and np.all(rows == 0x5A5A5A5A)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))      # no refused apply touched the model
    # a larger struct_size is a newer caller's; null outputs are fine; an apply on an empty region is legal and changes nothing
    assert lib.dust_hip_model_neighbours(model._h, C.byref(query(size=64)), None, None) == L.OK
    empty = query(birth=CAVE[0], survive=CAVE[1], lo=(3, 0, 0), hi=(2, 255, 255))
    assert lib.dust_hip_model_neighbours_apply(model._h, C.byref(empty), 256, ap, gp) == L.OK
    assert applied[0].tobytes() == W.zero_applied().tobytes() and not rows.any()
    assert lib.dust_hip_model_neighbours_apply(model._h, C.byref(good), 1, None, None) == L.OK
    same_model(model, ctx, W.apply(grid, W.CORNERS, CAVE[0], CAVE[1], 1)[0], pal)
    # unsupported exactly where set_voxels is, before the query is looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    assert status_of(lambda: deep.neighbours(W.FACES)) == L.ERR_UNSUPPORTED and status_of(lambda: deep.neighbours_apply(W.FACES, 0, 0)) == L.ERR_UNSUPPORTED
    assert lib.dust_hip_model_neighbours(deep._h, C.byref(bad[0]), rp, cp) == L.ERR_UNSUPPORTED
