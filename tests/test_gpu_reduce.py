"""Model reductions on the device (dust_hip_model_reduce; the contract is in include/dust_hip.h). Every comparison is exact: the new
model must read back byte for byte what a host build of the witness's grid uploads (tests/reduce_witness.py: the header's rule as
whole-array numpy, the opposite direction from the kernel's per-voxel gather), and the result record must hold the witness's counts."""
import ctypes as C

import numpy as np
import pytest

import reduce_witness as W
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
EMPTY = np.zeros((256,) * 3, np.uint8)


def host_model(grid, pal):
    return api.flatten_model(W.to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def same_bytes(model, grid, pal):
    return all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


def random_region(seed, density, lo, size, materials=(1, 256)):
    rng = np.random.default_rng(seed)
    grid = np.zeros((256,) * 3, np.uint8)
    region = tuple(slice(o, o + n) for o, n in zip(lo, size))
    grid[region] = np.where(rng.random(size) < density, rng.integers(materials[0], materials[1], size), 0)
    return grid


def counts(record):
    return [int(record[k]) for k in ("src_voxels", "voxels", "extent", "reserved")]


def check(model, grid, pal, levels=1, min_solid=1):
    """one call on the device and in the witness: the record and the bytes agree; returns the new model and the witness's grid"""
    coarse, record = model.reduce(levels, min_solid)
    want = W.reduce(grid, levels, min_solid)
    assert counts(record) == counts(W.result(grid, want, levels)), (levels, min_solid)
    assert same_bytes(coarse, want, pal), (levels, min_solid)
    return coarse, want


def ray_grid(n=8):
    """n * n rays along -x over the image of [16, 56)^3 under ROTATED, some of them beside it"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -50.0 + 50.0 * u.reshape(-1), 30.0 + 50.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def test_ties_and_thresholds():
    """materials 1..3 at density 0.6 in a 40^3 region at (12, 12, 12), across bricks and root cells: every min_solid, many ties"""
    rng = np.random.default_rng(71)
    region = np.where(rng.random((40,) * 3) < 0.6, rng.integers(1, 4, (40,) * 3), 0).astype(np.uint8)
    grid = EMPTY.copy()
    grid[12:52, 12:52, 12:52] = region
    # the conditions the case stands on, on the witness's side: at least a fifth of the solid coarse cells are ties, and every threshold matters
    kids = region.reshape(20, 2, 20, 2, 20, 2).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 8)
    per_material = np.stack([(kids == b).sum(axis=1) for b in (1, 2, 3)], axis=1)
    top = per_material.max(axis=1)
    tied = (per_material == top[:, None]).sum(axis=1) >= 2
    assert np.count_nonzero(tied & (top > 0)) >= 0.2 * np.count_nonzero(top > 0)
    voxels = [int(np.count_nonzero(W.reduce(grid, 1, k))) for k in range(1, 9)]
    assert len(set(voxels)) == 8 and min(voxels) > 0 and voxels == sorted(voxels, reverse=True)      # (26.8 % ties; 7994, 7936, 7624, 6657, 4824, 2476, 850, 133)
    pal = synth.make_palette(31)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for min_solid in range(1, 9):
        check(model, grid, pal, 1, min_solid)


def test_boundaries_and_every_material():
    """the last coarse brick, the destination's root-cell seam (coarse 63 | 64), a source root-cell corner, and byte 255"""
    rng = np.random.default_rng(72)
    grid = EMPTY.copy()
    corner = (np.arange(32 ** 3) % 255 + 1).astype(np.uint8)
    rng.shuffle(corner)
    corner[rng.random(corner.size) < 0.3] = 0
    grid[224:, 224:, 224:] = corner.reshape(32, 32, 32)
    grid[254:, 254:, 254:] = 255
    grid[127:130, 127:130, 127:130] = rng.integers(1, 256, (3, 3, 3))
    grid[15:18, 15:18, 15:18] = rng.integers(1, 256, (3, 3, 3))
    assert set(np.unique(grid).tolist()) == set(range(256))
    pal = synth.make_palette(32)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for min_solid in (1, 4):
        _, want = check(model, grid, pal, 1, min_solid)
        assert want[127, 127, 127] == 255 and want[64, 64, 64] and want[8, 8, 8]
        assert bool(want[63, 63, 63]) == bool(want[7, 7, 7]) == (min_solid == 1)      # one solid child each
        assert not want[128:].any() and not want[:, 128:].any() and not want[:, :, 128:].any()


def test_levels():
    grid = random_region(73, 0.5, (0, 0, 0), (64, 64, 64), materials=(1, 6))
    grid[200:, 200:, 200:] = 9
    grid[200:230, 200:, 240:] = 4
    pal = synth.make_palette(33)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    made = {}
    for levels, min_solid in ((1, 1), (2, 1), (3, 1), (3, 4), (4, 2), (8, 1), (8, 8)):
        made[levels, min_solid], want = check(model, grid, pal, levels, min_solid)
        side = 256 >> levels
        assert not want[side:].any() and not want[:, side:].any() and not want[:, :, side:].any()
    assert np.count_nonzero(W.reduce(grid, 8, 1)) == 1 and np.count_nonzero(W.reduce(grid, 8, 8)) == 0
    assert len(made[8, 1].read()[0]) == 1 and len(made[8, 8].read()[0]) == 0
    # levels = 2 is levels = 1 twice, on the device too
    twice, record = made[1, 1].reduce(1, 1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(twice.read(), made[2, 1].read()))
    assert int(record["src_voxels"]) == np.count_nonzero(W.reduce(grid, 1, 1)) and int(record["extent"]) == 128
    assert same_bytes(model, grid, pal)


def test_source_untouched():
    grid = random_region(74, 0.5, (16, 16, 16), (40, 40, 40), materials=(1, 30))
    pal = synth.make_palette(34)
    ctx = api.Context(device=0)
    origins, directions = ray_grid()
    points = [(16, 16, 16), (30, 31, 32), (200, 200, 200)]

    # a source that is not editable stays as it was created, and a scene committed on it keeps answering
    fixed = make(ctx, grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(fixed, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    assert np.count_nonzero(hits["instance"] != L.NO_HIT) > 10
    source_bytes = [a.tobytes() for a in fixed.read()]
    from_fixed, want = check(fixed, grid, pal, 2, 1)
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit: the source's generation has not moved
    fixed.find_islands(L.ISLANDS_FACES, capacity=0)                               # the first-edit transition happens HERE, not in reduce
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY

    # an editable source is read in place; its labelling and its fields stand, and a scene on it keeps answering
    loose = make(ctx, grid, pal)
    loose.find_islands(L.ISLANDS_FACES, capacity=0)
    loose.distance(max_radius=3)
    keys, values = loose.island_of(points), loose.distance_at(points)
    scene2 = api.Scene(ctx)
    scene2.add_instance(loose, ROTATED.reshape(12))
    scene2.commit()
    hits2 = scene2.trace_rays(origins, directions)
    from_loose, _ = check(loose, grid, pal, 2, 1)
    assert loose.island_of(points).tolist() == keys.tolist() and loose.distance_at(points).tolist() == values.tolist()
    assert scene2.trace_rays(origins, directions).tobytes() == hits2.tobytes()
    assert same_bytes(loose, grid, pal)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(from_fixed.read(), from_loose.read()))
    # an edit shows in the next reduction
    loose.set_voxels([(16, 16, 16), (17, 16, 16)], [7, -1])
    edited = grid.copy()
    edited[16, 16, 16], edited[17, 16, 16] = 8, 0
    check(loose, edited, pal, 1, 3)


def test_the_result_is_a_model_like_any_other():
    grid = random_region(75, 0.5, (16, 16, 16), (40, 40, 40), materials=(1, 30))
    pal = synth.make_palette(35)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    coarse, want = check(model, grid, pal, 1, 1)
    # shown where the source stands, it answers rays bit for bit as a model created on the host from the witness's grid does
    origins, directions = ray_grid()
    reference = make(ctx, want, pal)
    answers = []
    for m in (coarse, reference):
        scene = api.Scene(ctx)
        scene.add_instance(m, api.lod_transform(ROTATED, 1).reshape(12))
        scene.commit()
        answers.append(scene.trace_rays(origins, directions))
    assert answers[0].tobytes() == answers[1].tobytes()
    hit = answers[0]["instance"] != L.NO_HIT
    assert 10 < np.count_nonzero(hit) < len(hit)
    # it takes edits and a further reduction
    coarse.set_voxels([(8, 8, 8), (100, 3, 250)], [-1, 12])
    want[8, 8, 8], want[100, 3, 250] = 0, 13
    coarse.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [10, 10, 10], [14, 14, 14], op=L.EDIT_FILL, palette=40))
    want[10:14, 10:14, 10:14] = 41
    assert same_bytes(coarse, want, pal)
    check(coarse, want, pal, 1, 2)
    check(coarse, want, pal, 3, 1)


def test_empty_and_refused():
    pal = synth.make_palette(36)
    ctx = api.Context(device=0)
    lib = L.load()
    empty = make(ctx, EMPTY, pal)
    coarse, record = empty.reduce(1, 1)
    assert counts(record) == [0, 0, 128, 0] and len(coarse.read()[0]) == 0 and same_bytes(coarse, EMPTY, pal)
    sparse = random_region(76, 0.02, (0, 0, 0), (64, 64, 64), materials=(1, 9))
    model = make(ctx, sparse, pal)
    assert not W.reduce(sparse, 1, 8).any()
    coarse, want = check(model, sparse, pal, 1, 8)
    assert len(coarse.read()[0]) == 0

    out = C.c_void_p(0x5A5A5A5A)
    result = np.full(1, 0x5A, np.uint8).repeat(16).view(api.REDUCE_RESULT_DTYPE)
    before = result.tobytes()

    def call(m, levels, min_solid, flags=0, struct_size=C.sizeof(L.Reduce)):
        q = L.Reduce(struct_size=struct_size, levels=levels, min_solid=min_solid, flags=flags)
        return lib.dust_hip_model_reduce(m._h, C.byref(q), C.byref(out), result.ctypes.data_as(C.c_void_p))

    for levels, min_solid, flags in ((0, 1, 0), (9, 1, 0), (1, 0, 0), (1, 9, 0), (1, 1, 1), (0xFFFFFFFF, 1, 0), (1, 1, 1 << 31)):
        assert call(model, levels, min_solid, flags) == L.ERR_INVALID_ARGUMENT, (levels, min_solid, flags)
    assert call(model, 1, 1, struct_size=12) == L.ERR_INVALID_ARGUMENT and call(model, 1, 1, struct_size=0) == L.ERR_INVALID_ARGUMENT
    # unsupported exactly where set_voxels is, before the query's values are looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(sparse, pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        assert call(unsupported, 1, 1) == L.ERR_UNSUPPORTED
        assert call(unsupported, 99, 0, 7) == L.ERR_UNSUPPORTED
        assert call(unsupported, 1, 1, struct_size=12) == L.ERR_INVALID_ARGUMENT      # the struct_size comes first
    assert out.value == 0x5A5A5A5A and result.tobytes() == before
    assert same_bytes(model, sparse, pal)
    # a larger struct_size is a newer caller's: accepted; result may be NULL
    q = L.Reduce(struct_size=64, levels=2, min_solid=1, flags=0)
    h = C.c_void_p()
    assert lib.dust_hip_model_reduce(model._h, C.byref(q), C.byref(h), None) == L.OK and h.value
    lib.dust_hip_model_destroy(h)


def test_determinism():
    grid = random_region(77, 0.4, (3, 5, 7), (70, 50, 90), materials=(1, 4))
    pal = synth.make_palette(37)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    first, r1 = model.reduce(3, 2)
    second, r2 = model.reduce(3, 2)
    assert r1.tobytes() == r2.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first.read(), second.read()))
    assert same_bytes(first, W.reduce(grid, 3, 2), pal)
