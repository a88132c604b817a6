"""Model islands on the device (dust_hip_model_find_islands / island_of / detach_islands; the contract is in include/dust_hip.h). Every
comparison is exact: the records must be the witness's bytes (tests/island_witness.py: the header's definitions in numpy), a detached
piece and the remaining source must read back byte for byte what a host build of the witness's voxels uploads, and a scene showing the
source and the piece at one transform must answer every ray as the scene did before the detach."""
import ctypes as C

import numpy as np
import pytest

import island_witness as W
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

BOTH = (L.ISLANDS_FACES, L.ISLANDS_CORNERS)
BOTTOM = ((0, 0, 0), (255, 0, 255))    # the y = 0 layer
ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)


def key(x, y, z):
    return int(x) << 16 | int(y) << 8 | int(z)


def host_model(grid, pal):
    """(blocks, materials) of a grid through the product's host flatten: what dust_hip_model_create is given for those voxels"""
    return api.flatten_model(W.to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def same_bytes(model, grid, pal):
    return all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


def test_cube_pairs_across_brick_and_root_cell_boundaries():
    """two cubes sharing a face, only an edge, only a corner, or one voxel apart, across a brick's and a root cell's boundary on each
    axis -- on a model fresh from dust_hip_model_create, never edited"""
    pairs, grid = W.cube_pairs()
    pal = synth.make_palette(11)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for connectivity, column in ((L.ISLANDS_FACES, 3), (L.ISLANDS_CORNERS, 4)):
        n, rec = model.find_islands(connectivity)
        assert n == len(rec) == sum(p[column] for p in pairs)
        assert rec.tobytes() == W.records(W.label(grid, connectivity)).tobytes()
        a = model.island_of([p[1] for p in pairs])
        b = model.island_of([p[2] for p in pairs])
        for p, ka, kb in zip(pairs, a, b):
            assert ka == key(*p[1]) and (ka == kb) == (p[column] == 1), (p[0], connectivity)
    assert same_bytes(model, grid, pal)     # labelling moved the model into its editable form and changed no voxel


def test_snake_is_one_island():
    grid, path = W.snake()
    pal = synth.make_palette(12)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for connectivity in BOTH:
        n, rec = model.find_islands(connectivity, anchor=((0, 0, 0), (3, 5, 2)))
        assert n == 1 and len(rec) == 1
        r = rec[0]
        assert r["key"] == min(key(*p) for p in path) and r["voxels"] == len(path)
        assert r["lo"].tolist() == path.min(axis=0).tolist() and r["hi"].tolist() == path.max(axis=0).tolist()
        assert r["sum"].tolist() == path.sum(axis=0).tolist()
        assert r["flags"] == L.ISLAND_ANCHORED and r["reserved"] == 0       # (3, 5, 2) is the snake's first voxel
        assert rec.tobytes() == W.records(W.label(grid, connectivity), anchor=((0, 0, 0), (3, 5, 2))).tobytes()
        assert set(model.island_of(path).tolist()) == {int(r["key"])}


@pytest.mark.parametrize("density", [0.05, 0.30])
def test_random_fill_matches_the_witness(density):
    """sparse, and just under the face-connectivity percolation threshold (0.3116): over ten thousand islands of mixed size"""
    grid = W.random_fill(51, density)
    pal = synth.make_palette(13)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    rng = np.random.default_rng(52)
    anchor = ((30, 0, 0), (50, 255, 100))
    first = {}
    for connectivity in BOTH:
        labels = W.label(grid, connectivity)
        want = W.records(labels, anchor=anchor)
        n, rec = model.find_islands(connectivity, anchor=anchor)
        print(f"density {density} connectivity {connectivity}: {n} islands, largest {int(want['voxels'].max())} voxels")
        assert n == len(want) and (connectivity == L.ISLANDS_CORNERS or n > 10000)
        assert rec.tobytes() == want.tobytes()
        assert 0 < np.count_nonzero(rec["flags"]) < n
        # 10 000 coordinates: 5 000 drawn from the solid voxels, 4 000 anywhere in the filled region (at these densities most of
        # them are empty: 4 000 * 0.70 = 2 800 expected at the denser fill), 1 000 anywhere in the tree
        solid = np.argwhere(grid != 0)
        xyz = np.concatenate([solid[rng.integers(0, len(solid), 5000)], rng.integers(0, 64, (4000, 3)) + (24, 40, 56), rng.integers(0, 256, (1000, 3))])
        got = model.island_of(xyz)
        assert np.array_equal(got, W.island_of(labels, xyz))
        assert np.count_nonzero(got != L.NO_ISLAND) >= 5000 and np.count_nonzero(got == L.NO_ISLAND) >= 2000
        again_n, again = model.find_islands(connectivity, anchor=anchor)       # the labelling stands: described again, the same bytes
        assert again_n == n and again.tobytes() == rec.tobytes()
        first[connectivity] = rec
    for connectivity in BOTH:       # determinism: the other connectivity replaced the labelling, so this labels from scratch again
        n, rec = model.find_islands(connectivity, anchor=anchor)
        assert n == len(first[connectivity]) and rec.tobytes() == first[connectivity].tobytes()


def test_checkerboard_capacity_and_sentinels():
    grid = W.checkerboard(64)
    pal = synth.make_palette(14)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    n, none = model.find_islands(L.ISLANDS_FACES, capacity=0)
    assert n == 131072 and len(none) == 0
    records = np.frombuffer(bytes([0xA5]) * (1500 * 40), api.ISLAND_DTYPE).copy()
    sentinel = records[1000:].tobytes()
    q = L.IslandQuery(struct_size=C.sizeof(L.IslandQuery), connectivity=L.ISLANDS_FACES)
    q.anchor_lo[:] = [1, 1, 1]
    total = C.c_uint32()
    L.check(L.load().dust_hip_model_find_islands(model._h, C.byref(q), C.byref(total), records.ctypes.data_as(C.c_void_p), 1000))
    want = W.records(W.label(grid, W.FACES))
    assert total.value == 131072 == len(want)
    assert records[:1000].tobytes() == want[:1000].tobytes() and records[1000:].tobytes() == sentinel
    assert (want["voxels"] == 1).all()
    n, rec = model.find_islands(L.ISLANDS_CORNERS)
    assert n == 1 and rec.tobytes() == W.records(W.label(grid, W.CORNERS)).tobytes() and rec["voxels"][0] == 131072


def terrain_model(ctx, pal):
    """the terrain block as tools/shape_edit_timing.py builds it, a pillar on it, and the slab carved out of the pillar"""
    model = api.Model(ctx, *api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal), pal)
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 96, 0], [0, 120, 0], [100, 128, 90]],
                                      [[256, 96, 256], [256, 120, 256], [256, 128, 256], [120, 200, 110]], op=L.EDIT_FILL, palette=[1, 2, 3, 4]))
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [100, 150, 90], [120, 154, 110]))
    return model


def test_terrain_workflow_detaches_the_floating_top():
    grid, top = W.terrain()
    pal = synth.make_palette(3)
    ctx = api.Context(device=0)
    model = terrain_model(ctx, pal)
    assert same_bytes(model, grid, pal)
    labels = W.label(grid, W.FACES)
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    assert n == 2 and rec.tobytes() == W.records(labels, anchor=BOTTOM).tobytes()
    floating = rec[(rec["flags"] & L.ISLAND_ANCHORED) == 0]
    assert floating["key"].tolist() == [key(*top)] and model.island_of([top, (100, 149, 90), (100, 151, 90)]).tolist() == [key(*top), 0, L.NO_ISLAND]
    piece = model.detach_islands(floating["key"])
    want_piece, want_rest = W.detach(grid, labels, floating["key"])
    assert same_bytes(piece, want_piece, pal)
    assert same_bytes(model, want_rest, pal)
    assert model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)[1].tobytes() == W.records(labels, anchor=BOTTOM)[:1].tobytes()
    n, rec = piece.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)              # the new model is a model like any other
    assert n == 1 and rec["key"].tolist() == [key(*top)] and rec["flags"].tolist() == [0] and rec["voxels"].tolist() == [20 * 46 * 20]


def ruin():
    """a floor with three pillars: one whole, one cut through (its top floats), one cut twice; and some loose crumbs"""
    grid = np.zeros((256,) * 3, np.uint8)
    grid[20:100, 0:6, 20:100] = 2
    for i, x in enumerate((30, 55, 80)):
        grid[x:x + 7, 6:70, 40:47] = 10 + i
    grid[55:62, 30:33, 40:47] = 0
    grid[80:87, 20:22, 40:47] = 0
    grid[80:87, 47:52, 40:47] = 0
    rng = np.random.default_rng(53)
    for i, c in enumerate(rng.integers(25, 95, (40, 3))):
        if not grid[c[0] - 1:c[0] + 2, c[1] + 80 - 1:c[1] + 80 + 2, c[2] - 1:c[2] + 2].any():
            grid[c[0], c[1] + 80, c[2]] = 30 + i
    return grid


def ray_grid(n=64):
    """n * n rays through the ROTATED instance from two sides"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    u, v = u.reshape(-1), v.reshape(-1)
    half = len(u) // 2
    # world x = tree z + 40, y = tree y - 60, z = 90 - tree x: from above onto the floor, then from the side onto the pillars
    origins = np.stack([55.0 + 90.0 * u, np.full_like(u, 200.0), -15.0 + 180.0 * v], axis=1)
    directions = np.tile(np.float32([0.03, -1.0, 0.02]), (len(u), 1))
    origins[half:] = np.stack([np.full(len(u) - half, 300.0, np.float32), -65.0 + 190.0 * u[half:], -15.0 + 180.0 * (v[half:] - 0.5)], axis=1)
    directions[half:] = np.float32([-1.0, -0.05, 0.02])
    return origins.astype(np.float32), directions


def test_pieces_render_in_place():
    grid = ruin()
    pal = synth.make_palette(15)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    before = api.Scene(ctx)
    before.add_instance(model, ROTATED.reshape(12))
    before.commit()
    origins, directions = ray_grid()
    want = before.trace_rays(origins, directions)
    assert len(want) >= 4000 and 500 < np.count_nonzero(want["instance"] != L.NO_HIT) < len(want)
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    loose = rec["key"][rec["flags"] == 0]
    assert n == len(W.records(W.label(grid, W.FACES))) and len(loose) == n - 1 >= 10
    assert status_of(lambda: before.trace_rays(origins, directions)) == L.ERR_NOT_READY      # the labelling moved the model into its editable form
    piece = model.detach_islands(loose)
    hit_xyz = want["xyz"][want["instance"] != L.NO_HIT]
    assert 0 < np.count_nonzero(piece.get_voxels(hit_xyz) >= 0) < len(hit_xyz)     # the rays see both the pieces and what stayed
    after = api.Scene(ctx)
    after.add_instance(model, ROTATED.reshape(12))
    after.add_instance(piece, ROTATED.reshape(12))
    after.commit()
    got = after.trace_rays(origins, directions)
    assert np.array_equal(got["instance"] == L.NO_HIT, want["instance"] == L.NO_HIT)
    hit = want["instance"] != L.NO_HIT
    for field in ("t", "xyz", "face", "palette"):
        assert got[field][hit].tobytes() == want[field][hit].tobytes(), field
    assert set(got["instance"][hit].tolist()) == {0, 1}


def test_detach_arguments_and_states():
    grid = ruin()
    pal = synth.make_palette(16)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    labels = W.label(grid, W.FACES)
    want = W.records(labels, anchor=BOTTOM)
    assert status_of(lambda: model.island_of([(30, 10, 40)])) == L.ERR_NOT_READY        # never labelled
    assert status_of(lambda: model.detach_islands([0])) == L.ERR_NOT_READY
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    assert rec.tobytes() == want.tobytes()
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    origins, directions = ray_grid(32)
    hits = scene.trace_rays(origins, directions)
    loose = rec["key"][rec["flags"] == 0]
    top1, middle, top2 = key(55, 33, 40), key(80, 22, 40), key(80, 52, 40)
    assert top1 in loose and middle in loose and top2 in loose

    # a second labelling of an editable model leaves committed scenes valid
    assert model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)[1].tobytes() == want.tobytes()
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()

    # KEEP_SOURCE: a copy; the source's bytes and generation stay, the committed scene still renders
    copy = model.detach_islands([top1, top1, top2], keep_source=True)
    assert same_bytes(copy, W.detach(grid, labels, [top1, top2])[0], pal) and same_bytes(model, grid, pal)
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()
    assert status_of(lambda: copy.island_of([(55, 33, 40)])) == L.ERR_NOT_READY              # the new model starts unlabelled

    # refusals: nothing changes
    out = C.c_void_p(0x1234)
    keys = np.array([top1], np.uint32)
    kp = keys.ctypes.data_as(C.c_void_p)
    assert lib.dust_hip_model_detach_islands(model._h, kp, 1, L.DETACH_KEEP_SOURCE, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_detach_islands(model._h, kp, 1, 2, C.byref(out)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_detach_islands(model._h, None, 1, 0, C.byref(out)) == L.ERR_INVALID_ARGUMENT
    for bad in ([top1, key(55, 34, 40)], [key(200, 200, 200)], [top1, 1 << 24], [L.NO_ISLAND]):    # not the smallest voxel; empty; no voxel
        bad = np.array(bad, np.uint32)
        assert lib.dust_hip_model_detach_islands(model._h, bad.ctypes.data_as(C.c_void_p), len(bad), 0, C.byref(out)) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_detach_islands(model._h, bad.ctypes.data_as(C.c_void_p), len(bad), 0, None) == L.ERR_INVALID_ARGUMENT
    assert out.value == 0x1234 and same_bytes(model, grid, pal)
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()
    assert lib.dust_hip_model_detach_islands(model._h, None, 0, 0, C.byref(out)) == L.OK and out.value is None    # n == 0: a no-op
    assert model.detach_islands([]) is None and same_bytes(model, grid, pal)
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()

    # out == NULL deletes; the scene must be committed again; the labelling of the rest stands
    assert model.detach_islands([top1], want_model=False) is None
    piece1, rest1 = W.detach(grid, labels, [top1])
    assert same_bytes(model, rest1, pal)
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY
    scene.commit()
    assert model.island_of([(55, 33, 40), (58, 60, 43), (55, 29, 40), (80, 52, 40)]).tolist() == [L.NO_ISLAND, L.NO_ISLAND, key(20, 0, 20), top2]
    assert status_of(lambda: model.detach_islands([top1])) == L.ERR_INVALID_ARGUMENT          # the removed key is refused from now on
    assert same_bytes(model, rest1, pal)
    piece = model.detach_islands([top2])                                                       # ... another one goes without labelling again
    piece2, rest2 = W.detach(rest1, labels, [top2])
    assert same_bytes(piece, piece2, pal) and same_bytes(model, rest2, pal)
    crumbs = [k for k in loose.tolist() if k not in (top1, middle, top2)]
    assert model.detach_islands(crumbs, want_model=False) is None
    rest3 = W.detach(rest2, labels, crumbs)[1]
    assert same_bytes(model, rest3, pal)
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    assert n == 2 and rec.tobytes() == W.records(W.label(rest3, W.FACES), anchor=BOTTOM).tobytes()    # the floor, and the twice-cut pillar's middle

    # an edit invalidates the labelling, whatever it changes
    model.set_voxels([(200, 200, 200)], [-1])
    assert status_of(lambda: model.island_of([(30, 10, 40)])) == L.ERR_NOT_READY
    assert status_of(lambda: model.detach_islands([0])) == L.ERR_NOT_READY
    model.find_islands(L.ISLANDS_FACES)
    assert model.island_of([(30, 10, 40)]).tolist() == [key(20, 0, 20)]
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]))        # a shape that covers nothing
    assert status_of(lambda: model.island_of([(30, 10, 40)])) == L.ERR_NOT_READY


def test_find_islands_refusals():
    pal = synth.make_palette(17)
    ctx = api.Context(device=0)
    lib = L.load()
    grid = W.full(np.ones((3, 3, 3), np.uint8))
    model = make(ctx, grid, pal)
    q = L.IslandQuery(struct_size=C.sizeof(L.IslandQuery), connectivity=L.ISLANDS_FACES)
    n = C.c_uint32(77)
    rec = np.zeros(2, api.ISLAND_DTYPE)
    rp = rec.ctypes.data_as(C.c_void_p)
    fn = lib.dust_hip_model_find_islands
    assert fn(model._h, None, C.byref(n), rp, 2) == L.ERR_INVALID_ARGUMENT
    assert fn(model._h, C.byref(q), None, rp, 2) == L.ERR_INVALID_ARGUMENT
    assert fn(model._h, C.byref(q), C.byref(n), None, 2) == L.ERR_INVALID_ARGUMENT
    for size, connectivity in ((0, 0), (31, 0), (32, 2), (32, 0xFFFFFFFF)):
        bad = L.IslandQuery(struct_size=size, connectivity=connectivity)
        assert fn(model._h, C.byref(bad), C.byref(n), rp, 2) == L.ERR_INVALID_ARGUMENT
    assert n.value == 77 and not rec.view(np.uint8).any()
    assert status_of(lambda: model.island_of([(0, 0, 0)])) == L.ERR_NOT_READY      # none of these labelled the model
    assert fn(model._h, C.byref(q), C.byref(n), rp, 2) == L.OK and n.value == 1
    assert rec["voxels"].tolist() == [27, 0] and rec["sum"][0].tolist() == [27, 27, 27]
    keys = np.full(2, 77, np.uint32)
    xyz = np.array([[0, 0, 0], [0, 256, 0]], np.uint32)
    assert lib.dust_hip_model_island_of(model._h, xyz.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), 2) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_island_of(model._h, None, keys.ctypes.data_as(C.c_void_p), 2) == L.ERR_INVALID_ARGUMENT
    assert keys.tolist() == [77, 77]
    assert lib.dust_hip_model_island_of(model._h, None, None, 0) == L.OK


def test_model_states_empty_and_unsupported():
    pal = synth.make_palette(18)
    ctx = api.Context(device=0)
    empty = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    for connectivity in BOTH:
        n, rec = empty.find_islands(connectivity, anchor=BOTTOM)
        assert n == 0 and len(rec) == 0
    assert empty.island_of([(0, 0, 0), (255, 255, 255)]).tolist() == [L.NO_ISLAND] * 2
    assert status_of(lambda: empty.detach_islands([0])) == L.ERR_INVALID_ARGUMENT
    # detaching everything leaves an empty source, and an empty model is what a host build of no voxels uploads
    grid = np.zeros((256,) * 3, np.uint8)
    grid[250:256, 250:256, 250:256] = 9
    grid[0, 0, 0] = 1
    model = make(ctx, grid, pal)
    n, rec = model.find_islands(L.ISLANDS_CORNERS)
    assert rec["key"].tolist() == [0, key(250, 250, 250)]
    piece = model.detach_islands(rec["key"])
    assert same_bytes(piece, grid, pal) and same_bytes(model, np.zeros_like(grid), pal)
    assert len(model.read()[0]) == 0 and model.find_islands(L.ISLANDS_CORNERS)[0] == 0
    assert model.island_of([(0, 0, 0)]).tolist() == [L.NO_ISLAND]
    # unsupported exactly where set_voxels is: a 4096^3 tree
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    assert status_of(lambda: deep.find_islands()) == L.ERR_UNSUPPORTED
    assert status_of(lambda: deep.island_of([(0, 0, 0)])) == L.ERR_UNSUPPORTED
    assert status_of(lambda: deep.detach_islands([0])) == L.ERR_UNSUPPORTED
