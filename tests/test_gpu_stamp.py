"""Model stamps on the device (dust_hip_model_stamp; the contract is in include/dust_hip.h). Every comparison is exact: the destination
must read back byte for byte what a host build of the witness's grid uploads (tests/stamp_witness.py: the header's definitions as
whole-array numpy, the opposite direction from the kernel's per-voxel gather), and `changed` must be the witness's counts."""
import ctypes as C

import numpy as np
import pytest

import island_witness as W
import stamp_witness as S
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
BOTTOM = ((0, 0, 0), (255, 0, 255))
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


def check(model, source, stamps, grid, src_grid, pal, palette_map=None):
    """one call on the device and in the witness: the counts and the bytes agree; returns the witness's grid"""
    got = model.stamp(source, stamps, palette_map)
    want, counts = S.stamp(grid, src_grid, stamps, palette_map)
    assert got.tolist() == counts.tolist()
    assert same_bytes(model, want, pal)
    return want


def test_all_48_orientations_across_brick_and_root_cell_boundaries():
    """one call of 48 stamps of a 5 x 6 x 7 box in which every voxel has its own material and a third are empty, each image across a
    brick's and a root cell's boundary on all three axes; the destination fresh from dust_hip_model_create, the ops in turn"""
    rng = np.random.default_rng(61)
    box = (1 + np.arange(210, dtype=np.uint8)).reshape(5, 6, 7)
    box[rng.random(box.shape) < 1 / 3] = 0
    src_grid = np.zeros((256,) * 3, np.uint8)
    src_grid[3:8, 9:15, 14:21] = box
    dst_grid = random_region(62, 0.05, (0, 0, 0), (144, 144, 112))
    pal = synth.make_palette(21)
    ctx = api.Context(device=0)
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    words = S.all_orientations()
    offsets = [(13 + 32 * (k % 4), 13 + 32 * ((k // 4) % 4), 13 + 32 * (k // 16)) for k in range(48)]
    stamps = api.stamps(offsets, words, [k % 5 for k in range(48)], (3, 9, 14), (7, 14, 20))
    assert stamps.tobytes() == S.records(offsets, words, [k % 5 for k in range(48)], (3, 9, 14), (7, 14, 20)).tobytes()
    for s in stamps:    # every image box crosses a multiple of 16 on every axis
        p, _ = S.orient_fields(s["orient"])
        for r in range(3):
            assert int(s["offset"][r]) % 16 == 13 and (5, 6, 7)[p[r]] > 3
    want = check(dst, src, stamps, dst_grid, src_grid, pal)
    assert not np.array_equal(want, dst_grid)
    # the same call again on the result: deterministic, and the counts are the witness's again
    check(dst, src, stamps, want, src_grid, pal)
    assert same_bytes(src, src_grid, pal)


def test_every_op_with_overlapping_images_in_one_call():
    src_grid = random_region(63, 0.5, (8, 8, 8), (40, 40, 40))
    dst_grid = random_region(64, 0.5, (50, 50, 50), (40, 40, 40))
    pal = synth.make_palette(22)
    ctx = api.Context(device=0)
    src = make(ctx, src_grid, pal)
    lo, hi = (8, 8, 8), (47, 47, 47)
    rot = api.orientation((1, 2, 0), (True, False, False))
    offsets = [(45, 45, 45), (60, 55, 50), (52, 61, 58), (70, 70, 70), (48, 52, 66)]
    ops = [L.STAMP_CARVE, L.STAMP_PLACE, L.STAMP_PAINT, L.STAMP_REPLACE, L.STAMP_OVERWRITE]
    stamps = api.stamps(offsets, [api.ORIENT_IDENTITY, rot, api.ORIENT_IDENTITY, rot, api.ORIENT_IDENTITY], ops, lo, hi)
    together = make(ctx, dst_grid, pal)
    want = check(together, src, stamps, dst_grid, src_grid, pal)
    # one call of n stamps is n calls of one stamp
    apart = make(ctx, dst_grid, pal)
    grid = dst_grid
    for k in range(len(stamps)):
        got = apart.stamp(src, stamps[k:k + 1])
        grid, counts = S.stamp(grid, src_grid, stamps[k:k + 1])
        assert got.tolist() == counts.tolist() and counts[0] > 0
    assert np.array_equal(grid, want) and same_bytes(apart, want, pal)
    # the order matters: the swapped call differs exactly where the witness says it does
    swapped = make(ctx, dst_grid, pal)
    other = check(swapped, src, stamps[::-1].copy(), dst_grid, src_grid, pal)
    assert not np.array_equal(other, want)


def test_clipping_degenerate_boxes_and_a_whole_tree_replace():
    src_grid = random_region(65, 0.4, (0, 0, 0), (24, 24, 24))
    src_grid[250:256, 250:256, 250:256] = 77
    dst_grid = random_region(66, 0.3, (236, 0, 100), (20, 20, 20))
    pal = synth.make_palette(23)
    ctx = api.Context(device=0)
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    turn = api.orientation((2, 0, 1), (False, True, True))
    stamps = np.concatenate([
        api.stamps([(-10, -7, 95), (245, -3, 110), (240, 10, 105)], [api.ORIENT_IDENTITY, turn, turn], [L.STAMP_OVERWRITE, L.STAMP_PLACE, L.STAMP_PAINT],
                   (0, 0, 0), (23, 23, 23)),
        api.stamps([(255, 255, 255), (-5, -5, -5)], api.ORIENT_IDENTITY, L.STAMP_REPLACE, (250, 250, 250), (255, 255, 255)),
    ])
    grid = check(dst, src, stamps, dst_grid, src_grid, pal)
    assert grid[255, 255, 255] == 77 and grid[0, 0, 0] == 77
    # images entirely outside the tree, the int32 limits among the offsets, and empty source boxes: nothing changes
    lim = 2 ** 31
    outside = np.concatenate([
        api.stamps([(-lim, 0, 0), (lim - 1, 0, 0), (0, -lim, lim - 1), (256, 0, 0), (0, -24, 0), (0, 0, -lim + 23)], turn, L.STAMP_REPLACE, (0, 0, 0), (23, 23, 23)),
        api.stamps([(0, 0, 0), (10, 10, 10)], api.ORIENT_IDENTITY, L.STAMP_REPLACE, [(5, 0, 0), (0, 0, 200)], [(4, 255, 255), (255, 255, 199)]),
    ])
    before = dst.read()
    assert dst.stamp(src, outside).tolist() == [0] * 8 == S.stamp(grid, src_grid, outside)[1].tolist()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), before))
    # an offset at the limit whose image still reaches the tree: x = -2^31 + ... cannot, but y = -23 leaves one layer
    edge = api.stamps([(0, -23, 0), (255, 0, 0)], api.ORIENT_IDENTITY, L.STAMP_OVERWRITE, (0, 0, 0), (23, 23, 23))
    grid = check(dst, src, edge, grid, src_grid, pal)
    # the whole tree, mirrored along x and with y and z exchanged
    whole = api.stamps([(0, 0, 0)], api.orientation((0, 2, 1), (True, False, False)), L.STAMP_REPLACE)
    grid = check(dst, src, whole, grid, src_grid, pal)
    assert np.array_equal(grid, np.transpose(src_grid, (0, 2, 1))[::-1])


def test_snapshot_when_a_model_is_stamped_onto_itself():
    grid = random_region(67, 0.6, (40, 40, 40), (24, 24, 24))
    pal = synth.make_palette(24)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    lo, hi = (40, 40, 40), (63, 63, 63)
    for offset, op in (((41, 40, 40), L.STAMP_OVERWRITE), ((39, 42, 40), L.STAMP_REPLACE), ((41, 40, 40), L.STAMP_REPLACE), ((39, 42, 40), L.STAMP_OVERWRITE)):
        stamps = api.stamps([offset], api.ORIENT_IDENTITY, op, lo, hi)
        grid = check(model, model, stamps, grid, grid, pal)
    # two overlapping images in one call both read the model as it was when the call began
    stamps = api.stamps([(41, 40, 40), (42, 40, 40)], api.ORIENT_IDENTITY, L.STAMP_REPLACE, lo, hi)
    before = grid
    grid = check(model, model, stamps, grid, grid, pal)
    assert np.array_equal(grid[42:66, 40:64, 40:64], before[40:64, 40:64, 40:64])


def test_palette_map_and_the_source_is_left_alone():
    src_grid = random_region(68, 0.5, (16, 16, 16), (20, 20, 20), materials=(1, 40))
    dst_grid = random_region(69, 0.3, (100, 100, 100), (30, 30, 30))
    pal = synth.make_palette(25)
    ctx = api.Context(device=0)
    rng = np.random.default_rng(70)
    permutation = rng.permutation(255).astype(np.uint8)
    many_to_one = (np.arange(255) % 3 + 200).astype(np.uint8)
    lo, hi = (16, 16, 16), (35, 35, 35)
    origins = np.stack([np.full(256, 300.0), np.repeat(np.linspace(-50, -30, 16), 16), np.tile(np.linspace(55, 75, 16), 16)], axis=1).astype(np.float32)
    directions = np.tile(np.float32([-1.0, 0.01, 0.02]), (256, 1))

    # a source that is not editable: it stays as it was created, and a scene committed on it keeps answering
    fixed = make(ctx, src_grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(fixed, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    assert np.count_nonzero(hits["instance"] != L.NO_HIT) > 20
    source_bytes = [a.tobytes() for a in fixed.read()]
    dst = make(ctx, dst_grid, pal)
    grid = check(dst, fixed, api.stamps([(95, 95, 95)], api.orientation((1, 0, 2), (False, True, False)), L.STAMP_OVERWRITE, lo, hi), dst_grid, src_grid, pal, permutation)
    grid = check(dst, fixed, api.stamps([(110, 112, 114)], api.ORIENT_IDENTITY, L.STAMP_PLACE, lo, hi), grid, src_grid, pal, many_to_one)
    assert set(np.unique(grid[110:130, 112:132, 114:134])) >= {201, 202, 203}
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit: the source's generation has not moved
    assert status_of(lambda: fixed.island_of([(16, 16, 16)])) == L.ERR_NOT_READY  # ... and it was not made editable (never labelled either way)

    # an editable source is read in place: an edit between two stamps shows in the second
    loose = make(ctx, src_grid, pal)
    loose.set_voxels([(16, 16, 16)], [7])
    edited = src_grid.copy()
    edited[16, 16, 16] = 8
    scene2 = api.Scene(ctx)
    scene2.add_instance(loose, ROTATED.reshape(12))
    scene2.commit()
    hits2 = scene2.trace_rays(origins, directions)
    grid = check(dst, loose, api.stamps([(130, 95, 95)], api.ORIENT_IDENTITY, L.STAMP_REPLACE, lo, hi), grid, edited, pal, permutation)
    assert scene2.trace_rays(origins, directions).tobytes() == hits2.tobytes()
    assert same_bytes(loose, edited, pal)
    loose.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [16, 16, 16], [26, 26, 26], op=L.EDIT_FILL, palette=30))
    edited[16:26, 16:26, 16:26] = 31
    grid = check(dst, loose, api.stamps([(130, 95, 95)], api.ORIENT_IDENTITY, L.STAMP_REPLACE, lo, hi), grid, edited, pal, permutation)
    assert grid[130, 95, 95] == int(permutation[30]) + 1 and same_bytes(loose, edited, pal)


def test_round_trip_with_the_islands():
    """the floating top of the terrain's pillar is detached and stamped back lower down, until it stands on the pillar again"""
    terrain, top = W.terrain()
    pal = synth.make_palette(3)
    ctx = api.Context(device=0)
    model = api.Model(ctx, *api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal), pal)
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 96, 0], [0, 120, 0], [100, 128, 90]],
                                      [[256, 96, 256], [256, 120, 256], [256, 128, 256], [120, 200, 110]], op=L.EDIT_FILL, palette=[1, 2, 3, 4]))
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [100, 150, 90], [120, 154, 110]))
    labels = W.label(terrain, W.FACES)
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    floating = rec["key"][(rec["flags"] & L.ISLAND_ANCHORED) == 0]
    assert n == 2 and len(floating) == 1
    piece = model.detach_islands(floating)
    piece_grid, rest = W.detach(terrain, labels, floating)
    lo, hi = (100, 154, 90), (119, 199, 109)
    # two voxels lower: the carved slab was four thick, so the piece still hangs two voxels above the pillar
    stamps = api.stamps([(100, 152, 90)], api.ORIENT_IDENTITY, L.STAMP_PLACE, lo, hi)
    got = model.stamp(piece, stamps)
    grid, counts = S.stamp(rest, piece_grid, stamps)
    assert got.tolist() == counts.tolist() == [20 * 46 * 20]
    assert status_of(lambda: model.island_of([top])) == L.ERR_NOT_READY       # the stamp invalidated the labelling
    assert model.find_islands(L.ISLANDS_FACES, capacity=0)[0] == 2
    # two more: it touches the pillar, and PLACE leaves the voxels that are solid already as they are
    stamps = api.stamps([(100, 150, 90)], api.ORIENT_IDENTITY, L.STAMP_PLACE, lo, hi)
    got = model.stamp(piece, stamps)
    grid, counts = S.stamp(grid, piece_grid, stamps)
    assert got.tolist() == counts.tolist() == [20 * 2 * 20]
    assert status_of(lambda: model.island_of([top])) == L.ERR_NOT_READY
    reference = make(ctx, grid, pal)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), reference.read()))
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    assert n == 1 and rec["voxels"].tolist() == [int(np.count_nonzero(grid))] and model.island_of([top]).tolist() == [0]
    # a scene showing the result answers a ray grid as a model created from the witness's grid does
    u, v = np.meshgrid(np.linspace(0.0, 1.0, 64, dtype=np.float32), np.linspace(0.0, 1.0, 64, dtype=np.float32))
    origins = np.stack([np.full(u.size, 400.0, np.float32), 40.0 + 120.0 * u.reshape(-1), -80.0 + 140.0 * v.reshape(-1)], axis=1)
    directions = np.tile(np.float32([-1.0, -0.02, 0.01]), (u.size, 1))
    answers = []
    for m in (model, reference):
        scene = api.Scene(ctx)
        scene.add_instance(m, ROTATED.reshape(12))
        scene.commit()
        answers.append(scene.trace_rays(origins, directions))
    assert answers[0].tobytes() == answers[1].tobytes()
    hit = answers[0]["instance"] != L.NO_HIT
    assert 200 < np.count_nonzero(hit) < len(hit) and 5 in set((answers[0]["palette"][hit].astype(int) + 1).tolist())


def test_chunking_and_the_stamp_limit():
    """answers known without the witness: whole-tree REPLACE stamps that alternate the identity and an x flip of a half-solid source
    (more than 2^21 cell-list entries: at least two launches), then exactly DUST_HIP_MAX_STAMPS single-voxel stamps"""
    pal = synth.make_palette(26)
    ctx = api.Context(device=0)
    one = api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal)

    def filled(lo, hi, palette):
        m = api.Model(ctx, *one, pal)
        m.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0]] + [list(b) for b in lo], [[256, 256, 256]] + [list(b) for b in hi],
                                      op=[L.EDIT_CARVE] + [L.EDIT_FILL] * len(lo), palette=[0] + list(palette)))
        return m

    src = filled([(0, 0, 0)], [(128, 256, 256)], [9])
    dst = filled([], [], [])
    flip = api.orientation((0, 1, 2), (True, False, False))
    assert 520 * 4096 > 1 << 21
    stamps = api.stamps([(0, 0, 0)] * 520, [api.ORIENT_IDENTITY, flip] * 260, L.STAMP_REPLACE)
    changed = dst.stamp(src, stamps)
    assert changed.tolist() == [1 << 23] + [1 << 24] * 519
    want = filled([(128, 0, 0)], [(256, 256, 256)], [9])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), want.read()))
    # exactly the limit: one voxel of the source onto 65 536 distinct empty voxels
    x, y, z = np.meshgrid(np.arange(16), np.arange(64), np.arange(64), indexing="ij")
    offsets = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)
    rng = np.random.default_rng(71)
    offsets = offsets[rng.permutation(len(offsets))]
    assert len(offsets) == L.MAX_STAMPS
    single = api.stamps(offsets, api.ORIENT_IDENTITY, L.STAMP_PLACE, (5, 5, 5), (5, 5, 5))
    assert dst.stamp(src, single).tolist() == [1] * L.MAX_STAMPS
    want = filled([(128, 0, 0), (0, 0, 0)], [(256, 256, 256), (16, 64, 64)], [9, 9])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), want.read()))
    assert dst.stamp(src, single).tolist() == [0] * L.MAX_STAMPS       # PLACE over solid
    over = np.concatenate([single, single[:1]])
    assert status_of(lambda: dst.stamp(src, over)) == L.ERR_INVALID_ARGUMENT
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), want.read()))


def test_refusals_and_states():
    src_grid = random_region(72, 0.5, (0, 0, 0), (12, 12, 12), materials=(1, 100))
    dst_grid = random_region(73, 0.5, (4, 4, 4), (12, 12, 12))
    pal = synth.make_palette(27)
    ctx = api.Context(device=0)
    lib = L.load()
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    good = api.stamps([(2, 2, 2)], api.ORIENT_IDENTITY, L.STAMP_REPLACE, (0, 0, 0), (11, 11, 11))
    changed = np.full(2, 77, np.uint32)
    cp = changed.ctypes.data_as(C.c_void_p)
    fn = lib.dust_hip_model_stamp

    def call(d, s, stamps, n, palette_map=None):
        return fn(d, s, None if stamps is None else stamps.ctypes.data_as(C.c_void_p), n, None if palette_map is None else palette_map.ctypes.data_as(C.c_void_p), cp)

    bad = []
    for orient in (0, 0x15, 0x3F, api.ORIENT_IDENTITY | 1 << 9, api.ORIENT_IDENTITY | 1 << 31, 0x27):      # repeated axes, axis 3, high bits
        s = np.concatenate([good, good])
        s["orient"][1] = orient
        bad.append(s)
    for op in (5, 0xFFFFFFFF):
        s = np.concatenate([good, good])
        s["op"][1] = op
        bad.append(s)
    for s in bad:
        assert call(dst._h, src._h, s, 2) == L.ERR_INVALID_ARGUMENT
    assert call(None, src._h, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, None, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, src._h, None, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, src._h, good, L.MAX_STAMPS + 1) == L.ERR_INVALID_ARGUMENT
    palette_map = np.arange(255, dtype=np.uint8)
    palette_map[254] = 255
    assert call(dst._h, src._h, good, 1, palette_map) == L.ERR_INVALID_ARGUMENT
    other_ctx = api.Context(device=0)
    foreign = make(other_ctx, src_grid, pal)
    assert call(dst._h, foreign._h, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(foreign._h, src._h, good, 1) == L.ERR_INVALID_ARGUMENT
    assert changed.tolist() == [77, 77]
    assert same_bytes(dst, dst_grid, pal) and same_bytes(foreign, src_grid, pal)
    assert status_of(lambda: dst.island_of([(0, 0, 0)])) == L.ERR_NOT_READY

    # unsupported exactly where set_voxels is, for either model, before the stamps are looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(src_grid, pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        assert call(dst._h, unsupported._h, good, 1) == L.ERR_UNSUPPORTED
        assert call(unsupported._h, src._h, good, 1) == L.ERR_UNSUPPORTED
        assert call(dst._h, unsupported._h, bad[0], 2) == L.ERR_UNSUPPORTED
        assert call(unsupported._h, src._h, None, 0) == L.ERR_UNSUPPORTED
    assert same_bytes(dst, dst_grid, pal)

    # n == 0: a no-op that may make dst editable, and leaves a labelling alone
    dst.find_islands(L.ISLANDS_FACES, capacity=0)
    assert call(dst._h, src._h, None, 0) == L.OK and call(dst._h, src._h, good, 0, palette_map) == L.ERR_INVALID_ARGUMENT
    assert dst.stamp(src, good[:0]).tolist() == [] and same_bytes(dst, dst_grid, pal)
    assert dst.island_of([(200, 200, 200)]).tolist() == [L.NO_ISLAND]
    # changed may be NULL
    assert fn(dst._h, src._h, good.ctypes.data_as(C.c_void_p), 1, None, None) == L.OK
    grid, counts = S.stamp(dst_grid, src_grid, good)
    assert same_bytes(dst, grid, pal)
    assert status_of(lambda: dst.island_of([(200, 200, 200)])) == L.ERR_NOT_READY      # n > 0 invalidates the labelling
    # an empty source: REPLACE clears the image box, PLACE changes nothing
    empty = make(ctx, EMPTY, pal)
    assert dst.stamp(empty, api.stamps([(0, 0, 0)], op=L.STAMP_PLACE)).tolist() == [0]
    assert dst.stamp(empty, api.stamps([(0, 0, 0)], op=L.STAMP_REPLACE)).tolist() == [int(np.count_nonzero(grid))]
    assert len(dst.read()[0]) == 0 and same_bytes(dst, EMPTY, pal)
