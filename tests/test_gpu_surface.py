"""Model surfaces on the device (dust_hip_model_surface, dust_hip_model_surface_apply; the contract is in include/dust_hip.h). Every
comparison is exact: the result, the list and the tables must be, byte for byte, what the witness says (tests/surface_witness.py), an
apply must leave the model a host build of the witness's grid, and a surface call must leave the model as it found it."""
import ctypes as C
import functools

import numpy as np
import pytest

import shape_edit_witness as SW
import surface_witness as W
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)


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
    """single voxels at the two corners of the tree; pairs across the brick edge 3 | 4 and the root-cell edge 15 | 16 on each axis; a full
    brick; a 3-thick plate; a block of mixed materials across 15 | 16"""
    rng = np.random.default_rng(93)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[0, 0, 0], grid[255, 255, 255] = 1, 2
    for axis in range(3):
        for edge, at in ((3, 40), (15, 48)):
            a, b = [at + 8 * axis] * 3, [at + 8 * axis] * 3
            a[axis], b[axis] = edge + 64, edge + 65          # 67 | 68 and 79 | 80: the same edges, away from the other pieces
            grid[tuple(a)], grid[tuple(b)] = 3 + axis, 4 + axis
    grid[100:104, 104:108, 108:112] = 7                      # one brick exactly
    grid[120:150, 30:33, 120:150] = 8                        # the plate: 3 thick along y
    grid[123, 31, 124] = 0                                   # ... with a cavity in its middle layer
    grid[10:22, 10:22, 10:22] = np.where(rng.random((12,) * 3) < 0.8, rng.integers(1, 7, (12,) * 3), 0)
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def six_material_grid():
    """about 5 000 voxels of six materials in [0, 64)^3: a sparse scatter and a dense block across 15 | 16 and 31 | 32 (the recipe of the
    census tests)"""
    rng = np.random.default_rng(82)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[:64, :64, :64] = np.where(rng.random((64,) * 3) < 0.01, rng.integers(1, 7, (64,) * 3), 0)
    grid[13:27, 26:38, 14:20] = np.where(rng.random((14, 12, 6)) < 0.85, rng.integers(1, 7, (14, 12, 6)), 0)
    assert 3000 < np.count_nonzero(grid) < 6000
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def exposed_of(which, walls):
    return W.exposure({"hand": hand_built_grid, "six": six_material_grid}[which](), walls)


def check(model, grid, exposed=None, **query):
    """one query on the device and in the witness: result, full list and tables agree; returns them"""
    result, voxels, counts = model.surface(tables=True, **query)
    want_result, want_voxels, want_counts = W.surface(grid, exposed=exposed, **query)
    assert result.dtype == api.SURFACE_RESULT_DTYPE and voxels.dtype == api.SURFACE_VOXEL_DTYPE and counts.shape == (6, 256) and counts.dtype == np.uint32
    assert result.tobytes() == want_result.tobytes(), (query, result, want_result)
    assert len(voxels) == len(want_voxels), (query, len(voxels), len(want_voxels))
    bad = np.flatnonzero(voxels != want_voxels)
    assert len(bad) == 0, (query, bad[:5], voxels[bad[:5]], want_voxels[bad[:5]])
    assert voxels.tobytes() == want_voxels.tobytes()
    assert np.array_equal(counts, want_counts), (query, np.argwhere(counts != want_counts)[:5])
    assert int(counts.sum()) == int(result["faces"]) == int(result["by_face"].sum()) and not counts[:, 0].any()
    # counts only, and without tables: the same result
    alone, none, no_counts = model.surface(capacity=0, **query)
    assert alone.tobytes() == result.tobytes() and len(none) == 0 and no_counts is None
    return result, voxels, counts


@pytest.mark.parametrize("walls", [False, True])
def test_hand_built_grid(walls):
    grid = hand_built_grid()
    pal = synth.make_palette(51)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    exposed = exposed_of("hand", walls)
    result, voxels, counts = check(model, grid, exposed, walls=walls)
    assert int(result["solid"]) == np.count_nonzero(grid) and result["lo"].tolist() == [0] * 3 and result["hi"].tolist() == [255] * 3
    by_key = {int(v["key"]): int(v["faces"]) for v in voxels}
    assert by_key[0] == (0 if walls else 21) | 42 and by_key[(255 << 16) | (255 << 8) | 255] == 21 | (0 if walls else 42)
    assert by_key[(67 << 16) | (40 << 8) | 40] == 63 & ~L.FACE_POS_X and by_key[(68 << 16) | (40 << 8) | 40] == 63 & ~L.FACE_NEG_X
    assert by_key[(56 << 16) | (79 << 8) | 56] == 63 & ~L.FACE_POS_Y and by_key[(64 << 16) | (64 << 8) | 80] == 63 & ~L.FACE_NEG_Z
    assert sum(1 for k in by_key if 100 <= k >> 16 < 104 and 104 <= (k >> 8) & 255 < 108) == 56 and int(counts[:, 7].sum()) == 96
    assert (123 << 16 | 30 << 8 | 124) in by_key and (130 << 16 | 31 << 8 | 130) not in by_key      # the cavity's floor; the plate's buried middle
    for d in range(6):
        one, _, one_counts = check(model, grid, exposed, faces=1 << d, walls=walls)
        assert int(one["faces"]) == int(one["voxels"]) == int(result["by_face"][d]) and np.array_equal(one_counts[d], counts[d])
        assert not np.delete(one_counts, d, axis=0).any()
    for palette in (6, 0, 3, 200):                                                 # the brick's material, a corner's, a pair's, one nobody has
        part, part_voxels, _ = check(model, grid, exposed, palette=palette, walls=walls)
        assert int(part["solid"]) == np.count_nonzero(grid == palette + 1) and np.all(part_voxels["palette"] == palette)
    check(model, grid, exposed, faces=L.FACE_POS_Y | L.FACE_NEG_X, palette=7, walls=walls)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def test_random_blocks_and_regions_that_cut_through_bricks():
    grid = six_material_grid()
    pal = synth.make_palette(52)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    rng = np.random.default_rng(94)
    total, _, _ = check(model, grid, exposed_of("six", False))
    assert int(total["voxels"]) > 3000
    check(model, grid, exposed_of("six", True), walls=True)
    regions = [((13, 26, 14), (26, 37, 19)), ((14, 27, 15), (25, 36, 18)), ((15, 0, 0), (16, 255, 255)), ((0, 31, 17), (63, 32, 17)), ((5, 5, 5), (5, 5, 5)),
               ((0, 0, 0), (63, 63, 63)), ((32, 32, 32), (255, 255, 255))]
    for _ in range(12):
        lo = rng.integers(0, 40, 3)
        regions.append((tuple(int(v) for v in lo), tuple(int(v) for v in lo + rng.integers(0, 30, 3))))
    listed = 0
    for k, region in enumerate(regions):
        walls, faces, palette = bool(k & 1), (63, 8, 21, 42, 36)[k % 5], (-1, -1, 2, 5)[k % 4]
        result, _, _ = check(model, grid, exposed_of("six", walls), region=region, faces=faces, palette=palette, walls=walls)
        listed += int(result["voxels"])
    assert listed > 3000
    # a voxel on the region's edge keeps its face hidden by a solid neighbour just outside the region
    inner = ((14, 27, 15), (25, 36, 18))
    dense = grid[13:27, 26:38, 14:20] != 0
    x, y, z = [(14, 26 + j, 14 + k) for j, k in np.argwhere(dense[0] & dense[1]).tolist() if 27 <= 26 + j <= 36 and 15 <= 14 + k <= 18][0]
    assert grid[x, y, z] != 0 and grid[x - 1, y, z] != 0 and x == inner[0][0]
    _, voxels, _ = model.surface(region=inner)
    faces = {int(v["key"]): int(v["faces"]) for v in voxels}
    assert not faces.get((x << 16) | (y << 8) | z, 0) & L.FACE_NEG_X
    assert any(f & L.FACE_NEG_X for f in faces.values())


def test_capacity():
    grid = six_material_grid()
    pal = synth.make_palette(53)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    region = ((10, 20, 10), (30, 40, 25))
    want_result, want, _ = W.surface(grid, region=region, exposed=exposed_of("six", False))
    total = len(want)
    assert total > 500
    q = model._surface_query(L.FACES_ALL, -1, region, False)
    for capacity in (0, 1, total - 1, total, total + 5):
        out = np.full((total + 8) * 8, 0x5A, np.uint8).view(api.SURFACE_VOXEL_DTYPE)
        result = np.zeros(1, api.SURFACE_RESULT_DTYPE)
        assert lib.dust_hip_model_surface(model._h, C.byref(q), result.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), capacity, None) == L.OK
        written = min(capacity, total)
        assert out[:written].tobytes() == want[:written].tobytes(), capacity
        assert out[written:].tobytes() == b"\x5a" * (8 * (total + 8 - written)), capacity
        assert result[0].tobytes() == want_result.tobytes(), capacity
    # through the Python call: a given capacity truncates, None lists everything
    assert model.surface(region=region, capacity=7)[1].tobytes() == want[:7].tobytes()
    assert model.surface(region=region)[1].tobytes() == want.tobytes()


def test_full_tree_and_empty_model():
    pal = synth.make_palette(54)
    ctx = api.Context(device=0)
    model = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    zero = W.zero_result()
    result, voxels, counts = model.surface(tables=True)
    assert result.tobytes() == zero.tobytes() and len(voxels) == 0 and not counts.any()
    assert model.surface(region=((9, 9, 9), (8, 200, 200)))[0].tobytes() == zero.tobytes()      # lo > hi: legal and empty
    assert model.edit_shapes(SW.shapes(SW.shape(SW.BOX, (-1e30,) * 3, (1e30,) * 3, op=SW.FILL, palette=254))).tolist() == [1 << 24]
    result, voxels, counts = model.surface(tables=True)
    assert (int(result["voxels"]), int(result["faces"]), int(result["solid"])) == (390152, 393216, 1 << 24) and result["by_face"].tolist() == [65536] * 6
    assert result["lo"].tolist() == [0] * 3 and result["hi"].tolist() == [255] * 3
    assert counts[:, 255].tolist() == [65536] * 6 and int(counts.sum()) == 393216
    key = voxels["key"].astype(np.int64)
    x, y, z = key >> 16, (key >> 8) & 255, key & 255
    assert len(voxels) == 390152 and np.all(np.diff(W.block_order(x, y, z)) > 0) and np.all(voxels["palette"] == 254) and not voxels["reserved"].any()
    want_faces = ((x == 0) * 1 + (x == 255) * 2 + (y == 0) * 4 + (y == 255) * 8 + (z == 0) * 16 + (z == 255) * 32)
    assert np.array_equal(voxels["faces"], want_faces) and want_faces.min() > 0
    walled, none, _ = model.surface(walls=True)
    assert (int(walled["voxels"]), int(walled["faces"]), int(walled["solid"])) == (0, 0, 1 << 24) and len(none) == 0
    assert walled["lo"].tolist() == [255] * 3 and walled["hi"].tolist() == [0] * 3
    assert model.surface(region=((9, 9, 9), (8, 200, 200)), tables=True)[0].tobytes() == zero.tobytes()


def test_surface_apply():
    grid = hand_built_grid()
    pal = synth.make_palette(55)
    ctx = api.Context(device=0)

    def applied(grid, value, **query):
        """one apply on a fresh model: `changed` and the model are the witness's, and a surface call agrees on the edited grid"""
        model = make(ctx, grid, pal)
        first = model.surface(capacity=0, **query)[0]
        changed = model.surface_apply(value, **query)
        after, want_changed = W.apply(grid, value, **query)
        assert changed == want_changed
        assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(after, pal)))
        check(model, after)
        return model, after, changed, first

    # None on the plate peels exactly its outer layer: the middle layer's rim and the voxels round the cavity go, the rest of it stays
    plate = ((120, 30, 120), (149, 32, 149))
    model, after, changed, first = applied(grid, -1, region=plate)
    assert changed == int(first["voxels"]) == 2 * 900 + 4 * 29 + 4
    assert np.count_nonzero(after[120:150, 30:33, 120:150]) == 28 * 28 - 1 - 4 and after[130, 31, 130] == 8 and after[121, 31, 121] == 8
    assert np.array_equal(after[:100], grid[:100])                                # nothing outside the region moved
    # a second peel takes what the first one opened, and only that
    assert model.surface_apply(-1, region=plate) == 28 * 28 - 5 and model.surface(capacity=0)[0]["solid"] == np.count_nonzero(grid) - 30 * 30 * 3 + 1
    # +y only with a palette index paints the tops
    model, after, changed, first = applied(grid, 9, faces=L.FACE_POS_Y)
    assert changed == int(first["voxels"]) and np.count_nonzero(after == 10) == changed and np.all(after[120:150, 32, 120:150] == 10)
    assert after[123, 30, 124] == 10 and after[125, 30, 125] == 8 and after[100, 107, 110] == 10 and after[100, 106, 110] == 7
    # a value equal to the current material changes nothing; under a filter only that material is repainted
    _, _, changed, first = applied(grid, 6, region=((100, 104, 108), (103, 107, 111)))
    assert changed == 0 and int(first["voxels"]) == 56
    _, after, changed, _ = applied(grid, 0, palette=6, walls=True, faces=L.FACE_NEG_Z | L.FACE_POS_X)
    assert changed == 16 + 16 - 4 and np.count_nonzero(after[100:104, 104:108, 108:112] == 1) == 28
    _, _, changed, _ = applied(grid, -1, region=((5, 5, 5), (4, 9, 9)))           # lo > hi: legal, empty
    assert changed == 0


def ray_grid(n=8):
    """n * n rays along -x over the image of [0, 64)^3 under ROTATED"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def test_the_model_is_only_read():
    grid = six_material_grid()
    pal = synth.make_palette(56)
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
    check(fixed, grid, exposed_of("six", False), region=region)
    fixed.surface(capacity=0)                                                     # (masks only: no grid is made)
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit: the generation has not moved
    fixed.find_islands(L.ISLANDS_FACES, capacity=0)                               # the first-edit transition happens HERE, not in surface
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY

    # an editable model is read in place, edits included; its labelling and both fields stand
    loose = make(ctx, grid, pal)
    loose.set_voxels([(20, 30, 16), (21, 30, 16), (60, 60, 60)], [5, -1, 0])
    edited = grid.copy()
    edited[20, 30, 16], edited[21, 30, 16], edited[60, 60, 60] = 6, 0, 1
    loose.find_islands(L.ISLANDS_FACES, capacity=0)
    loose.distance(max_radius=3)
    loose.flood([(100, 100, 100)], max_steps=90)
    keys, values, steps = loose.island_of(points), loose.distance_at(points), loose.flood_at(points)
    scene2 = api.Scene(ctx)
    scene2.add_instance(loose, ROTATED.reshape(12))
    scene2.commit()
    hits2 = scene2.trace_rays(origins, directions)
    check(loose, edited)
    check(loose, edited, palette=5, faces=L.FACE_POS_Y, walls=True)
    assert loose.island_of(points).tolist() == keys.tolist() and loose.distance_at(points).tolist() == values.tolist()
    assert loose.flood_at(points).tolist() == steps.tolist()
    assert scene2.trace_rays(origins, directions).tobytes() == hits2.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(loose.read(), host_model(edited, pal)))

    # surface_apply is an edit: the labelling and both fields are gone, and the scene needs a commit
    assert loose.surface_apply(3, faces=L.FACE_POS_Z, region=region) > 0
    assert status_of(lambda: loose.island_of(points)) == L.ERR_NOT_READY and status_of(lambda: loose.distance_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: loose.flood_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: scene2.trace_rays(origins, directions)) == L.ERR_NOT_READY
    scene2.commit()
    assert len(scene2.trace_rays(origins, directions)) == len(hits2)


def test_determinism_and_refusals():
    grid = six_material_grid()
    pal = synth.make_palette(57)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    first = model.surface(tables=True)
    second = model.surface(tables=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)) and int(first[0]["voxels"]) > 3000
    one, two = make(ctx, grid, pal), make(ctx, grid, pal)
    assert one.surface_apply(-1) == two.surface_apply(-1) and all(x.tobytes() == y.tobytes() for x, y in zip(one.read(), two.read()))

    result = np.full(64, 0x5A, np.uint8).view(api.SURFACE_RESULT_DTYPE)
    voxels = np.full(16 * 8, 0x5A, np.uint8).view(api.SURFACE_VOXEL_DTYPE)
    counts = np.full((6, 256), 0x5A5A5A5A, np.uint32)
    changed = C.c_uint32(0x5A5A5A5A)
    before = result.tobytes(), voxels.tobytes(), counts.tobytes()
    rp, vp, cp = (a.ctypes.data_as(C.c_void_p) for a in (result, voxels, counts))

    def query(faces=63, flags=0, palette=-1, lo=(0, 0, 0), hi=(255, 255, 255), size=C.sizeof(L.SurfaceQuery)):
        q = L.SurfaceQuery(struct_size=size, faces=faces, flags=flags, palette=palette)
        q.lo[:], q.hi[:] = lo, hi
        return q
    bad = [query(faces=0), query(faces=64), query(flags=2), query(flags=1 << 31), query(palette=-2), query(palette=255), query(lo=(0, 256, 0)),
           query(hi=(255, 255, 256)), query(lo=(1 << 31, 0, 0)), query(size=47), query(size=0)]
    for q in bad:
        assert lib.dust_hip_model_surface(model._h, C.byref(q), rp, vp, 16, cp) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_surface_apply(model._h, C.byref(q), 3, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    good = query()
    assert lib.dust_hip_model_surface(model._h, None, rp, vp, 16, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_surface(model._h, C.byref(good), rp, None, 16, cp) == L.ERR_INVALID_ARGUMENT      # null voxels with capacity > 0
    assert lib.dust_hip_model_surface_apply(model._h, None, 3, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_surface_apply(model._h, C.byref(good), 255, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), voxels.tobytes(), counts.tobytes()) == before and changed.value == 0x5A5A5A5A
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))      # no refused apply touched the model
    # every output may be null; a larger struct_size is a newer caller's
    assert lib.dust_hip_model_surface(model._h, C.byref(query(size=64)), None, None, 0, None) == L.OK
    assert lib.dust_hip_model_surface_apply(model._h, C.byref(query(lo=(3, 0, 0), hi=(2, 255, 255))), -1, None) == L.OK
    # unsupported exactly where set_voxels is, before the query is looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(grid, pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        assert status_of(lambda: unsupported.surface()) == L.ERR_UNSUPPORTED and status_of(lambda: unsupported.surface_apply(-1)) == L.ERR_UNSUPPORTED
        for q in (bad[0], bad[4], bad[6]):
            assert lib.dust_hip_model_surface(unsupported._h, C.byref(q), rp, vp, 16, cp) == L.ERR_UNSUPPORTED
            assert lib.dust_hip_model_surface_apply(unsupported._h, C.byref(q), 300, C.byref(changed)) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_surface(unsupported._h, None, rp, vp, 16, cp) == L.ERR_UNSUPPORTED
    assert (result.tobytes(), voxels.tobytes(), counts.tobytes()) == before and changed.value == 0x5A5A5A5A
