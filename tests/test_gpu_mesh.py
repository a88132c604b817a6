"""Model meshes on the device (dust_hip_model_mesh; the contract is in include/dust_hip.h). Every comparison is exact: the result and
the full list must be, byte for byte, what the witness says (tests/mesh_witness.py), and a mesh call must leave the model as it
found it."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_witness as W
import shape_edit_witness as SW
import surface_witness as S
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
PLATE = ((120, 30, 120), (149, 32, 149))


def host_model(grid, pal):
    return api.flatten_model(to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


@functools.lru_cache(maxsize=None)
def hand_built_grid():
    """the smallest shapes at which the merge can go wrong, each away from the others"""
    grid = np.zeros((256,) * 3, np.uint8)
    grid[0, 0, 0], grid[255, 255, 255] = 1, 2                   # the two corners of the tree
    grid[10:80, 200, 200], grid[204, 10:80, 204], grid[208, 208, 10:80] = 3, 4, 5      # bars across 15 | 16, 31 | 32 and 63 | 64
    grid[:, 220, 100], grid[224, :, 104], grid[228, 108, :] = 6, 6, 6                  # full-height columns: the extent 256
    grid[120:150, 30:33, 120:150] = 8                           # the plate: 3 thick along y
    grid[123, 31, 124] = 0                                      # ... with a cavity in its middle layer
    grid[120:150, 30:33, 134:136] = 9                           # ... and a stripe of a second material, two voxels wide along z
    for k in range(4):
        grid[60 + k, 150, 20:25 + k] = 1                        # a staircase whose rows share u0 but not u1 (+-y: u = z, v = x)
        grid[60 + k, 160, 20 + k:30] = 1                        # ... and one sharing u1 but not u0
    grid[70, 150, 20:25], grid[71, 150, 20:25] = 1, 2           # two stacked identical runs of different materials
    grid[80, 150, 20:40], grid[81, 150, 20:30] = 1, 1           # a run under a longer run
    grid[100:104, 104:108, 108:112] = 7                         # one brick exactly
    grid[160:176, 60:76, 160:176] = (np.indices((16,) * 3).sum(axis=0) & 1).astype(np.uint8) * 4      # a 3-D checkerboard
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def random_block_grid(which):
    """a 40^3 block across 15 | 16 and 31 | 32 on every axis: density 0.5 with one material, 0.9 with two, 0.97 with three"""
    density, materials = ((0.5, 1), (0.9, 2), (0.97, 3))[which]
    rng = np.random.default_rng(110 + which)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[10:50, 10:50, 10:50] = np.where(rng.random((40,) * 3) < density, rng.integers(1, materials + 1, (40,) * 3), 0)
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def exposed_of(which, walls):
    return S.exposure(hand_built_grid() if which == "hand" else random_block_grid(which), walls)


def check(model, grid, exposed=None, **query):
    """one query on the device and in the witness: result and full list agree; returns them"""
    result, quads = model.mesh(**query)
    want_result, want_quads = W.mesh(grid, exposed=exposed, **query)
    assert result.dtype == api.MESH_RESULT_DTYPE and quads.dtype == api.MESH_QUAD_DTYPE
    assert result.tobytes() == want_result.tobytes(), (query, result, want_result)
    assert len(quads) == len(want_quads), (query, len(quads), len(want_quads))
    bad = np.flatnonzero(quads != want_quads)
    assert len(bad) == 0, (query, bad[:5], quads[bad[:5]], want_quads[bad[:5]])
    assert quads.tobytes() == want_quads.tobytes()
    alone, none = model.mesh(capacity=0, **query)                                 # counts only: the same result
    assert alone.tobytes() == result.tobytes() and len(none) == 0
    surface_query = {k: v for k, v in query.items() if k != "any_palette"}
    assert result["faces_by_face"].tolist() == model.surface(capacity=0, **surface_query)[0]["by_face"].tolist()
    return result, quads


@pytest.mark.parametrize("walls", [False, True])
def test_hand_built_grid(walls):
    grid = hand_built_grid()
    pal = synth.make_palette(61)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    exposed = exposed_of("hand", walls)
    for any_palette in (False, True):
        result, quads = check(model, grid, exposed, walls=walls, any_palette=any_palette)
        assert int(result["largest"]) == (900 if any_palette else 420)
        for d in range(6):
            one, one_quads = check(model, grid, exposed, faces=1 << d, walls=walls, any_palette=any_palette)
            assert one_quads.tobytes() == quads[quads["face"] == d].tobytes() and int(one["quads"]) == int(result["quads_by_face"][d])
        by_key = {}
        for q in quads:
            by_key.setdefault(int(q["key"]), []).append((int(q["face"]), int(q["du"]), int(q["dv"])))
        # the corners of the tree: three faces each under walls, six without
        assert [f for f, _, _ in by_key[0]] == ([1, 3, 5] if walls else [0, 1, 2, 3, 4, 5])
        assert [f for f, _, _ in by_key[(255 << 16) | (255 << 8) | 255]] == ([0, 2, 4] if walls else [0, 1, 2, 3, 4, 5])
        # the bars, 70 long: along x a column of one-voxel rows for the +-y faces (u = z, v = x), one run for the +-z faces (u = y, v = x)
        assert by_key[(10 << 16) | (200 << 8) | 200] == [(0, 0, 0), (2, 0, 69), (3, 0, 69), (4, 0, 69), (5, 0, 69)]
        assert by_key[(204 << 16) | (10 << 8) | 204] == [(0, 0, 69), (1, 0, 69), (2, 0, 0), (4, 69, 0), (5, 69, 0)]
        assert by_key[(208 << 16) | (208 << 8) | 10] == [(0, 69, 0), (1, 69, 0), (2, 69, 0), (3, 69, 0), (4, 0, 0)]
        # the full-height columns: the extent 256 is stored as 255
        assert (2, 0, 255) in by_key[(0 << 16) | (220 << 8) | 100] and (0, 0, 255) in by_key[(224 << 16) | (0 << 8) | 104]
        assert (0, 255, 0) in by_key[(228 << 16) | (108 << 8) | 0] and (2, 255, 0) in by_key[(228 << 16) | (108 << 8) | 0]
        # the full brick: one 4 x 4 quad per direction
        brick, brick_quads = check(model, grid, exposed, region=((100, 104, 108), (103, 107, 111)), walls=walls, any_palette=any_palette)
        assert brick["quads_by_face"].tolist() == [1] * 6 and np.all(brick_quads["du"] == 3) and np.all(brick_quads["dv"] == 3)
        # the checkerboard: every quad is one face
        board, _ = check(model, grid, exposed, region=((160, 60, 160), (175, 75, 175)), walls=walls, any_palette=any_palette)
        assert int(board["quads"]) == int(board["faces"]) == 6 * 16 ** 3 // 2 and int(board["largest"]) == 1
        # the plate: the stripe cuts every run along z in three, so +-x and +-y have three quads where +-z (u = y) has one; the
        # cavity adds one face per direction; any_palette merges it back
        plate, _ = check(model, grid, exposed, region=PLATE, walls=walls, any_palette=any_palette)
        assert plate["quads_by_face"].tolist() == ([2] * 6 if any_palette else [4, 4, 4, 4, 2, 2])
        assert int(plate["faces"]) == 2 * 900 + 4 * 90 + 6 and int(plate["largest"]) == (900 if any_palette else 14 * 30)
        # +y over the staircases and the stacked runs (slice y = 150: rows x, runs along z)
        stairs, stair_quads = check(model, grid, exposed, faces=L.FACE_POS_Y, region=((60, 150, 0), (63, 160, 255)), walls=walls, any_palette=any_palette)
        assert int(stairs["quads"]) == 8 and np.all(stair_quads["dv"] == 0) and int(stairs["faces"]) == 26 + 34      # neither staircase merges
        stacked, _ = check(model, grid, exposed, faces=L.FACE_POS_Y, region=((70, 150, 0), (71, 150, 255)), walls=walls, any_palette=any_palette)
        assert (int(stacked["quads"]), int(stacked["faces"])) == (1 if any_palette else 2, 10)
        under, _ = check(model, grid, exposed, faces=L.FACE_POS_Y, region=((80, 150, 0), (81, 150, 255)), walls=walls, any_palette=any_palette)
        assert (int(under["quads"]), int(under["faces"]), int(under["largest"])) == (2, 30, 20)
    check(model, grid, exposed, palette=8, walls=walls)                           # the stripe's material alone: the plate's other two thirds do not show
    check(model, grid, exposed, palette=7, faces=L.FACE_POS_Y | L.FACE_NEG_X, walls=walls, any_palette=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def test_full_tree_and_empty_model():
    pal = synth.make_palette(62)
    ctx = api.Context(device=0)
    model = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    zero = W.zero_result()
    for any_palette in (False, True):
        result, quads = model.mesh(any_palette=any_palette)
        assert result.tobytes() == zero.tobytes() == bytes(64) and len(quads) == 0
    assert model.mesh(region=((9, 9, 9), (8, 200, 200)))[0].tobytes() == zero.tobytes()      # lo > hi: legal and empty
    assert model.edit_shapes(SW.shapes(SW.shape(SW.BOX, (-1e30,) * 3, (1e30,) * 3, op=SW.FILL, palette=254))).tolist() == [1 << 24]
    for any_palette in (False, True):
        result, quads = model.mesh(any_palette=any_palette)
        assert (int(result["quads"]), int(result["faces"]), int(result["largest"])) == (6, 393216, 65536)
        assert result["quads_by_face"].tolist() == [1] * 6 and result["faces_by_face"].tolist() == [65536] * 6
        assert quads["face"].tolist() == list(range(6)) and np.all(quads["du"] == 255) and np.all(quads["dv"] == 255) and np.all(quads["palette"] == 254)
        assert quads["key"].tolist() == [0, 255 << 16, 0, 255 << 8, 0, 255]
        walled, none = model.mesh(walls=True, any_palette=any_palette)
        assert walled.tobytes() == zero.tobytes() and len(none) == 0
    assert model.mesh(region=((9, 9, 9), (8, 200, 200)))[0].tobytes() == zero.tobytes()
    inner, inner_quads = model.mesh(region=((5, 0, 7), (5, 255, 7)))              # a column of the full tree: its two ends show
    assert inner["quads_by_face"].tolist() == [0, 0, 1, 1, 0, 0] and inner_quads["key"].tolist() == [(5 << 16) | 7, (5 << 16) | (255 << 8) | 7]


def test_random_blocks_and_regions():
    pal = synth.make_palette(63)
    ctx = api.Context(device=0)
    grids = [random_block_grid(k) for k in range(3)]
    models = [make(ctx, g, pal) for g in grids]
    rng = np.random.default_rng(111)
    # slabs through the whole block, cuts through bricks, whole slices of each axis, one-voxel regions, the tree's near and far parts
    regions = [((10, 10, 10), (49, 49, 20)), ((10, 10, 10), (17, 49, 49)), ((8, 8, 8), (51, 20, 51)), ((12, 13, 14), (30, 33, 47)), ((15, 0, 0), (16, 255, 255)),
               ((0, 31, 0), (255, 32, 255)), ((0, 0, 20), (255, 255, 20)), ((30, 0, 0), (30, 255, 255)), ((20, 20, 20), (20, 20, 20)), ((11, 12, 13), (11, 12, 13)),
               ((0, 0, 0), (63, 63, 17)), ((32, 32, 32), (255, 255, 255))]
    for _ in range(8):
        lo = rng.integers(5, 40, 3)
        regions.append((tuple(int(v) for v in lo), tuple(int(v) for v in lo + rng.integers(3, 30, 3))))
    listed = larger = 0
    for k, region in enumerate(regions):
        which = k % 3
        grid = grids[which]
        walls, any_palette = bool(k & 1), bool((k >> 1) & 1)
        faces, palette = (63, 63, 63, 8, 21, 42, 36)[k % 7], (-1, -1, -1, 0, 1)[k % 5]
        query = dict(region=region, faces=faces, palette=palette, walls=walls, any_palette=any_palette)
        result, quads = check(models[which], grid, exposed_of(which, walls), **query)
        # the quads, drawn back, are the faces the surface call counts: each one once
        covered, twice = W.rasterise(quads, (64,) * 3)
        box = S.clip(grid, region)
        want = np.zeros(grid.shape, np.uint8)
        looked_at = grid[box] != 0 if palette < 0 else grid[box] == palette + 1
        want[box] = np.where(looked_at, exposed_of(which, walls)[box] & np.uint8(faces), 0)
        assert not twice and np.array_equal(covered, want[:64, :64, :64]) and not want[64:].any(), query
        listed += len(quads)
        larger += int(np.count_nonzero((quads["du"].astype(np.int64) + 1) * (quads["dv"].astype(np.int64) + 1) > 1))
    # rows really merged (the witness alone: 41 885 quads, 11 749 of them larger than one face)
    assert listed > 3000 and 4 * larger >= listed, (listed, larger)


def test_capacity():
    grid = random_block_grid(1)
    pal = synth.make_palette(64)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    region = ((12, 10, 14), (40, 35, 30))
    want_result, want = W.mesh(grid, region=region, exposed=exposed_of(1, False))
    total = len(want)
    assert total > 500
    q = L.MeshQuery(struct_size=C.sizeof(L.MeshQuery), faces=L.FACES_ALL, palette=-1)
    q.lo[:], q.hi[:] = region
    for capacity in (0, 1, total - 1, total, total + 5):
        out = np.full((total + 8) * 8, 0x5A, np.uint8).view(api.MESH_QUAD_DTYPE)
        result = np.zeros(1, api.MESH_RESULT_DTYPE)
        assert lib.dust_hip_model_mesh(model._h, C.byref(q), result.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), capacity) == L.OK
        written = min(capacity, total)
        assert out[:written].tobytes() == want[:written].tobytes(), capacity
        assert out[written:].tobytes() == b"\x5a" * (8 * (total + 8 - written)), capacity
        assert result[0].tobytes() == want_result.tobytes(), capacity
    # through the Python call: a given capacity truncates, None lists everything
    assert model.mesh(region=region, capacity=7)[1].tobytes() == want[:7].tobytes()
    assert model.mesh(region=region)[1].tobytes() == want.tobytes()


def ray_grid(n=8):
    """n * n rays along -x over the image of [0, 64)^3 under ROTATED"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def test_the_model_is_only_read():
    grid = random_block_grid(0)
    pal = synth.make_palette(65)
    ctx = api.Context(device=0)
    origins, directions = ray_grid()
    points = [(13, 26, 14), (20, 30, 16), (200, 200, 200)]
    region = ((0, 0, 0), (40, 40, 40))

    # a model that was never edited stays as it was created, and a scene committed on it keeps answering
    fixed = make(ctx, grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(fixed, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    assert np.count_nonzero(hits["instance"] != L.NO_HIT) > 5
    source_bytes = [a.tobytes() for a in fixed.read()]
    check(fixed, grid, exposed_of(0, False), region=region)
    fixed.mesh(capacity=0, any_palette=True)                                      # (masks only: no grid is made)
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fixed.read(), host_model(grid, pal)))
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit: the generation has not moved
    fixed.find_islands(L.ISLANDS_FACES, capacity=0)                               # the first-edit transition happens HERE, not in mesh
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY

    # an editable model is read in place, edits included; its labelling and both fields stand
    loose = make(ctx, grid, pal)
    loose.set_voxels([(20, 30, 16), (21, 30, 16), (60, 60, 60)], [2, -1, 0])
    edited = grid.copy()
    edited[20, 30, 16], edited[21, 30, 16], edited[60, 60, 60] = 3, 0, 1
    assert all(x.tobytes() == y.tobytes() for x, y in zip(loose.read(), host_model(edited, pal)))
    loose.find_islands(L.ISLANDS_FACES, capacity=0)
    loose.distance(max_radius=3)
    loose.flood([(100, 100, 100)], max_steps=90)
    keys, values, steps = loose.island_of(points), loose.distance_at(points), loose.flood_at(points)
    scene2 = api.Scene(ctx)
    scene2.add_instance(loose, ROTATED.reshape(12))
    scene2.commit()
    hits2 = scene2.trace_rays(origins, directions)
    check(loose, edited)
    check(loose, edited, palette=2, faces=L.FACE_POS_Y, walls=True, any_palette=True)
    assert loose.island_of(points).tolist() == keys.tolist() and loose.distance_at(points).tolist() == values.tolist()
    assert loose.flood_at(points).tolist() == steps.tolist()
    assert scene2.trace_rays(origins, directions).tobytes() == hits2.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(loose.read(), host_model(edited, pal)))


def test_determinism_and_refusals():
    grid = random_block_grid(1)
    pal = synth.make_palette(66)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    first, second = model.mesh(), model.mesh()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)) and int(first[0]["quads"]) > 1000

    result = np.full(64, 0x5A, np.uint8).view(api.MESH_RESULT_DTYPE)
    quads = np.full(16 * 8, 0x5A, np.uint8).view(api.MESH_QUAD_DTYPE)
    before = result.tobytes(), quads.tobytes()
    rp, qp = (a.ctypes.data_as(C.c_void_p) for a in (result, quads))

    def query(faces=63, flags=0, palette=-1, lo=(0, 0, 0), hi=(255, 255, 255), size=C.sizeof(L.MeshQuery)):
        q = L.MeshQuery(struct_size=size, faces=faces, flags=flags, palette=palette)
        q.lo[:], q.hi[:] = lo, hi
        return q
    bad = [query(faces=0), query(faces=64), query(flags=4), query(flags=1 << 31), query(palette=-2), query(palette=255), query(lo=(0, 256, 0)),
           query(hi=(255, 255, 256)), query(lo=(1 << 31, 0, 0)), query(size=47), query(size=0)]
    for q in bad:
        assert lib.dust_hip_model_mesh(model._h, C.byref(q), rp, qp, 16) == L.ERR_INVALID_ARGUMENT
    good = query()
    assert lib.dust_hip_model_mesh(model._h, None, rp, qp, 16) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_mesh(model._h, C.byref(good), rp, None, 16) == L.ERR_INVALID_ARGUMENT      # null quads with capacity > 0
    assert (result.tobytes(), quads.tobytes()) == before
    # every output may be null; a larger struct_size is a newer caller's; both flags together are fine
    assert lib.dust_hip_model_mesh(model._h, C.byref(query(size=64)), None, None, 0) == L.OK
    assert lib.dust_hip_model_mesh(model._h, C.byref(query(flags=3)), None, None, 0) == L.OK
    assert lib.dust_hip_model_mesh(model._h, C.byref(query(lo=(3, 0, 0), hi=(2, 255, 255))), rp, qp, 16) == L.OK
    assert result.tobytes() == bytes(64) and quads.tobytes() == before[1]          # lo > hi: the zero result, nothing listed
    result[:] = np.frombuffer(before[0], api.MESH_RESULT_DTYPE)
    # unsupported exactly where set_voxels is, before the query is looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(grid, pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        assert status_of(lambda: unsupported.mesh()) == L.ERR_UNSUPPORTED
        for q in (bad[0], bad[2], bad[4], bad[6]):
            assert lib.dust_hip_model_mesh(unsupported._h, C.byref(q), rp, qp, 16) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_mesh(unsupported._h, None, rp, qp, 16) == L.ERR_UNSUPPORTED
    assert (result.tobytes(), quads.tobytes()) == before
