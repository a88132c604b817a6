"""Model resampling on the device (dust_hip_model_resample; the contract is in include/dust_hip.h). Every comparison is exact: the
destination must read back byte for byte what a host build of the witness's grid uploads (tests/resample_witness.py: the header's
definitions as whole-array int64 numpy with np.floor_divide), and the four counts must be the witness's."""
import ctypes as C

import numpy as np
import pytest

import island_witness as W
import resample_witness as R
import stamp_witness as S
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
EMPTY = np.zeros((256,) * 3, np.uint8)
EYE = np.eye(3, dtype=np.int64) * R.ONE


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


def fixed(v):
    return int(round(float(v) * R.ONE))


def check(model, source, recs, grid, src_grid, pal, palette_map=None):
    """one call on the device and in the witness: the counts and the bytes agree; returns the witness's grid and counts"""
    got = model.resample(source, recs, palette_map)
    want, counts = R.resample(grid, src_grid, recs, palette_map)
    assert got.tolist() == counts.tolist()
    assert same_bytes(model, want, pal)
    return want, counts


def permutation_forward(word, offset, lo, hi):
    """the forward matrix of a stamp: the signed axis permutation `word` of the sub-box lo..hi with its image box's lowest corner at offset"""
    p, g = S.orient_fields(word)
    f = np.zeros((3, 4))
    for r in range(3):
        f[r, p[r]] = -1.0 if g[r] else 1.0
        f[r, 3] = offset[r] + (hi[p[r]] + 1 if g[r] else -lo[p[r]])
    return f


def test_the_48_orientations_agree_with_stamp():
    """test_gpu_stamp.py's 48 stamps of a 5 x 6 x 7 box, every image across a brick's and a root cell's boundary on all axes, the ops in
    turn: the resample of the signed-permutation matrix leaves the same bytes and the same `changed`"""
    rng = np.random.default_rng(61)
    box = (1 + np.arange(210, dtype=np.uint8)).reshape(5, 6, 7)
    box[rng.random(box.shape) < 1 / 3] = 0
    src_grid = np.zeros((256,) * 3, np.uint8)
    src_grid[3:8, 9:15, 14:21] = box
    dst_grid = random_region(62, 0.05, (0, 0, 0), (144, 144, 112))
    pal = synth.make_palette(21)
    ctx = api.Context(device=0)
    src, stamped, resampled = make(ctx, src_grid, pal), make(ctx, dst_grid, pal), make(ctx, dst_grid, pal)
    words = S.all_orientations()
    offsets = [(13 + 32 * (k % 4), 13 + 32 * ((k // 4) % 4), 13 + 32 * (k // 16)) for k in range(48)]
    ops = [k % 5 for k in range(48)]
    lo, hi = (3, 9, 14), (7, 14, 20)
    changed = stamped.stamp(src, api.stamps(offsets, words, ops, lo, hi))
    recs = api.resamples([permutation_forward(w, o, lo, hi) for w, o in zip(words, offsets)], ops, lo, hi)
    counts = resampled.resample(src, recs)
    assert counts["changed"].tolist() == changed.tolist() and changed.sum() > 2000
    assert counts["covered"].tolist() == [210] * 48 and counts["solid"].tolist() == [int(np.count_nonzero(box))] * 48
    assert all(x.tobytes() == y.tobytes() for x, y in zip(stamped.read(), resampled.read()))
    want, witness = R.resample(dst_grid, src_grid, recs)
    assert witness.tolist() == counts.tolist() and same_bytes(resampled, want, pal)
    assert same_bytes(src, src_grid, pal)


def general_records(ops, pivots, lo, hi):
    centre = [0.5 * (l + h + 1) for l, h in zip(lo, hi)]
    mirror = api.rotation_about("x", 63.0, centre, pivots[4])
    mirror[:, 0] *= -1.0                                       # x of the source reversed, then turned
    mirror[:, 3] = np.asarray(pivots[4]) - mirror[:, :3] @ np.asarray(centre)
    shear = np.array([[1.0, 0.5, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, -0.25, 1.0, 0.0]])
    shear[:, 3] = np.asarray(pivots[2]) - shear[:, :3] @ np.asarray(centre)
    forward = [api.rotation_about("z", 30.0, centre, pivots[0]), api.rotation_about((1, 2, 3), 37.0, centre, pivots[1]), shear,
               api.rotation_about("y", 0.0, centre, pivots[3], scale=1.5), mirror]
    return api.resamples(forward, ops, lo, hi)


def test_general_maps_against_the_witness():
    lo, hi = (20, 30, 40), (28, 39, 50)
    src_grid = np.zeros((256,) * 3, np.uint8)
    src_grid[20:29, 30:40, 40:51] = (np.arange(990) % 255 + 1).astype(np.uint8).reshape(9, 10, 11)
    src_grid[18:31, 28:42, 38:53][src_grid[18:31, 28:42, 38:53] == 0] = 255       # a shell around the sub-box: reading beyond it would show
    dst_grid = random_region(64, 0.5, (30, 46, 62), (40, 40, 40))
    pal = synth.make_palette(22)
    ctx = api.Context(device=0)
    src = make(ctx, src_grid, pal)
    ops = [L.STAMP_CARVE, L.STAMP_PLACE, L.STAMP_PAINT, L.STAMP_REPLACE, L.STAMP_OVERWRITE]
    # every image across a multiple of 16 on every axis
    apart = general_records(ops, [(48, 64, 80), (64, 64, 80), (48, 80, 80), (64, 80, 96), (48, 64, 96)], lo, hi)
    for k in range(5):
        model = make(ctx, dst_grid, pal)
        _, counts = check(model, src, apart[k:k + 1], dst_grid, src_grid, pal)
        assert counts["covered"][0] > 800 and counts["changed"][0] > 0 and 0 < counts["blocked"][0] < counts["solid"][0]
    # ... and overlapping in one call
    recs = general_records(ops, [(48, 64, 80), (52, 66, 82), (46, 62, 78), (50, 60, 84), (49, 68, 76)], lo, hi)
    together = make(ctx, dst_grid, pal)
    want, counts = check(together, src, recs, dst_grid, src_grid, pal)
    assert (counts["changed"] > 0).all() and not np.array_equal(want, dst_grid)
    # one call of n records is n calls of one record
    single = make(ctx, dst_grid, pal)
    grid = dst_grid
    for k in range(len(recs)):
        grid, c = check(single, src, recs[k:k + 1], grid, src_grid, pal)
        assert c.tolist() == counts[k:k + 1].tolist()
    assert np.array_equal(grid, want)
    # the order matters: the reversed call differs exactly where the witness says it does
    swapped = make(ctx, dst_grid, pal)
    other, _ = check(swapped, src, recs[::-1].copy(), dst_grid, src_grid, pal)
    assert not np.array_equal(other, want)


def test_answers_known_without_the_witness():
    rng = np.random.default_rng(65)
    box = rng.integers(1, 256, (16, 16, 16)).astype(np.uint8)
    box[rng.random(box.shape) < 0.3] = 0
    src_grid = np.zeros((256,) * 3, np.uint8)
    src_grid[0:16, 0:16, 0:16] = box
    pal = synth.make_palette(23)
    ctx = api.Context(device=0)
    src = make(ctx, src_grid, pal)
    for scale, t, expect in ((R.ONE // 2, 0, np.repeat(np.repeat(np.repeat(box, 2, 0), 2, 1), 2, 2)),      # m = 0.5: every source voxel eight times
                             (2 * R.ONE, 0, box[1::2, 1::2, 1::2]),                                       # m = 2.0, t = 0: source voxels 2 d + 1
                             (2 * R.ONE, -R.ONE // 2, box[0::2, 0::2, 0::2])):                            # m = 2.0, t = -0.5: source voxels 2 d
        rec = R.records([np.eye(3, dtype=np.int64) * scale], [(t, t, t)], (0, 0, 0), (255, 255, 255), L.STAMP_REPLACE, (0, 0, 0), (15, 15, 15))
        dst = make(ctx, EMPTY, pal)
        counts = dst.resample(src, rec)
        n = expect.shape[0]
        want = EMPTY.copy()
        want[0:n, 0:n, 0:n] = expect
        assert same_bytes(dst, want, pal)
        assert counts.tolist() == [(int(np.count_nonzero(expect)), n ** 3, int(np.count_nonzero(expect)), 0)]


def test_the_floor_rounds_toward_minus_infinity():
    """destination voxels that land at source position -0.25 on an axis are outside the sub-box and stay as they were under REPLACE (a
    truncating shift would read source voxel 0, which is solid); on the high side the voxel at src_hi + 0.75 is the last one inside"""
    src_grid = np.zeros((256,) * 3, np.uint8)
    src_grid[0:8, 0:8, 0:8] = 9                      # solid beyond the sub-box 0..3 too
    dst_grid = np.zeros((256,) * 3, np.uint8)
    dst_grid[0:8, 0:8, 0:8] = 200
    pal = synth.make_palette(24)
    ctx = api.Context(device=0)
    src = make(ctx, src_grid, pal)
    for axis in range(3):
        t = [0, 0, 0]
        t[axis] = fixed(-0.75)                       # destination voxel d reads source position d + 0.5 - 0.75
        rec = R.records([EYE], [t], (0, 0, 0), (7, 7, 7), L.STAMP_REPLACE, (0, 0, 0), (3, 3, 3))
        dst = make(ctx, dst_grid, pal)
        counts = dst.resample(src, rec)
        want = dst_grid.copy()
        region = [slice(0, 4)] * 3
        region[axis] = slice(1, 5)                   # voxel 0 lands at -0.25: untouched; voxel 4 at 3.75: the last inside; voxel 5 at 4.75: untouched
        want[tuple(region)] = 9
        assert same_bytes(dst, want, pal) and counts.tolist() == [(64, 64, 64, 64)]
        assert R.resample(dst_grid, src_grid, rec)[1].tolist() == counts.tolist()


def limit_record(lo, hi, op):
    """m entries of +-8.0 and t of +-2^28 with an image inside the tree: s[0] = 8 (x + y + z) + 12 - 4096 lies in 0..255 for x + y + z in
    511..542, s[1] = 4096 - 8 (x + y) - 8 for x + y in 480..511, s[2] = z"""
    m = [[R.MAX_M, R.MAX_M, R.MAX_M], [-R.MAX_M, -R.MAX_M, 0], [0, 0, R.ONE]]
    return R.records([m], [(-R.MAX_T, R.MAX_T, 0)], lo, hi, op)


def test_limits():
    src_grid = random_region(66, 0.7, (0, 0, 0), (256, 256, 64))
    dst_grid = random_region(67, 0.4, (236, 236, 0), (20, 20, 64))
    pal = synth.make_palette(25)
    ctx = api.Context(device=0)
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    recs = np.concatenate([limit_record((0, 0, 0), (255, 255, 255), L.STAMP_OVERWRITE), limit_record((236, 236, 0), (255, 255, 40), L.STAMP_REPLACE)])
    want, counts = check(dst, src, recs, dst_grid, src_grid, pal)
    assert counts["covered"][0] > 1000 and counts["covered"][1] > 500 and counts["changed"].all()
    for field, value in (("m", R.MAX_M + 1), ("m", -R.MAX_M - 1), ("t", R.MAX_T + 1), ("t", -R.MAX_T - 1)):
        bad = recs.copy()
        bad[field][1].reshape(-1)[2] = value
        assert status_of(lambda: dst.resample(src, bad)) == L.ERR_INVALID_ARGUMENT
        assert status_of(lambda: dst.resample(src, bad, dry_run=True)) == L.ERR_INVALID_ARGUMENT
    assert same_bytes(dst, want, pal)


def test_the_cull_on_a_thin_slab_turned_out_of_the_axes():
    rng = np.random.default_rng(68)
    src_grid = np.zeros((256,) * 3, np.uint8)
    src_grid[20:220, 30:230, 100:103] = rng.integers(1, 256, (200, 200, 3))
    dst_grid = random_region(69, 0.2, (96, 96, 96), (64, 64, 64))
    pal = synth.make_palette(26)
    ctx = api.Context(device=0)
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    lo, hi = (20, 30, 100), (219, 229, 102)
    recs = api.resamples(api.rotation_about("y", 45.0, (120.0, 130.0, 101.5), (128.0, 128.0, 128.0)), L.STAMP_REPLACE, lo, hi)
    recs["dst_lo"], recs["dst_hi"] = 0, 255                      # the whole tree: the bounding box says nothing
    listed, reached = R.cells_listed(recs[0])
    assert reached == 4096 and 0 < len(listed) < 2048            # the interval test rejects more than half of the root cells
    _, counts = check(dst, src, recs, dst_grid, src_grid, pal)
    assert counts["covered"][0] > 50000 and counts["blocked"][0] > 0


def test_clipping_and_degenerate_records():
    src_grid = random_region(70, 0.6, (0, 0, 0), (24, 24, 24))
    dst_grid = random_region(71, 0.3, (236, 0, 100), (20, 20, 20))
    pal = synth.make_palette(27)
    ctx = api.Context(device=0)
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    lo, hi = (0, 0, 0), (23, 23, 23)
    turn = api.rotation_about((1, 1, 0), 50.0, (12, 12, 12), (250.0, 3.0, 110.0))
    partly = api.resamples(turn, L.STAMP_OVERWRITE, lo, hi)
    assert partly["dst_lo"][0][1] < 0 and partly["dst_hi"][0][0] > 255
    grid, counts = check(dst, src, partly, dst_grid, src_grid, pal)
    assert 0 < counts["covered"][0] < 24 ** 3
    lim = 2 ** 31
    nothing = np.concatenate([
        R.records([EYE], [(0, 0, 0)], (256, 0, 0), (lim - 1, 23, 23), L.STAMP_REPLACE, lo, hi),                 # wholly outside the tree
        R.records([EYE], [(0, 0, 0)], (-lim, -lim, -lim), (-1, 300, 300), L.STAMP_REPLACE, lo, hi),
        R.records([EYE], [(0, 0, 0)], (0, 12, 0), (23, 11, 23), L.STAMP_REPLACE, lo, hi),                       # dst_lo > dst_hi
        R.records([EYE], [(0, 0, 0)], (0, 0, 0), (23, 23, 23), L.STAMP_REPLACE, (0, 0, 9), (23, 23, 8)),        # src_lo > src_hi
        R.records([EYE], [(fixed(-60), 0, 0)], (0, 0, 0), (23, 23, 23), L.STAMP_REPLACE, lo, hi),               # no voxel lands in the sub-box
    ])
    before = dst.read()
    assert not dst.resample(src, nothing).view(np.uint32).any() and not R.resample(grid, src_grid, nothing)[1].view(np.uint32).any()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), before))
    # a record the interval test passes as a whole and rules out in every root cell: s[0] = 8 x + 4, so cell 0 reads 4..124 and cell 1
    # 132..252 -- source x = 127 lies in the whole box's interval 4..252 and in neither cell's. It is live and its chunk has no cells
    gap = R.records([EYE * np.array([8, 1, 1])[:, None]], [(0, 0, 0)], (0, 0, 0), (31, 15, 15), L.STAMP_REPLACE, (127, 0, 0), (127, 15, 15))
    assert R.box_can_hold(gap[0], *R.clipped_box(gap[0])) and R.cells_listed(gap[0]) == ([], 2)
    mixed = np.concatenate([gap, nothing[:1], gap])
    for dry in (True, False):
        assert not dst.resample(src, mixed, dry_run=dry).view(np.uint32).any() and not R.resample(grid, src_grid, mixed, dry_run=dry)[1].view(np.uint32).any()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), before))
    # ... and between records that do write: the counts stay in their places
    around = np.concatenate([gap, partly, gap])
    grid, counts = check(dst, src, around, grid, src_grid, pal)
    assert counts["covered"].tolist() == [0, counts["covered"][1], 0] and counts["covered"][1] > 0
    # a singular m: every voxel of the clipped box reads one source voxel
    zero = R.records([np.zeros((3, 3))], [(fixed(3.5), fixed(4.5), fixed(5.5))], (-3, 250, 107), (2, 260, 109), L.STAMP_REPLACE, lo, hi)
    grid, counts = check(dst, src, zero, grid, src_grid, pal)
    assert (grid[0:3, 250:256, 107:110] == src_grid[3, 4, 5]).all() and counts["covered"][0] == 3 * 6 * 3
    # a rank-one m: every voxel reads the source line x = 5..
    line = R.records([[[R.ONE, 0, 0], [0, 0, 0], [0, 0, 0]]], [(0, fixed(6.5), fixed(7.5))], (0, 40, 40), (23, 44, 44), L.STAMP_REPLACE, lo, hi)
    grid, _ = check(dst, src, line, grid, src_grid, pal)
    assert (grid[0:24, 40:45, 40:45] == src_grid[0:24, 6, 7][:, None, None]).all()


def test_snapshot_when_a_model_is_resampled_onto_itself():
    grid = random_region(72, 0.6, (40, 40, 40), (24, 24, 24))
    pal = synth.make_palette(28)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    lo, hi = (40, 40, 40), (63, 63, 63)
    centre = (52.0, 52.0, 52.0)
    for degrees, at, op in ((20.0, (54.0, 52.0, 52.0), L.STAMP_OVERWRITE), (-35.0, (50.0, 55.0, 52.0), L.STAMP_REPLACE)):
        grid, _ = check(model, model, api.resamples(api.rotation_about("z", degrees, centre, at), op, lo, hi), grid, grid, pal)
    # two overlapping images in one call both read the model as it was when the call began
    recs = api.resamples([api.rotation_about("y", 15.0, centre, (53.0, 52.0, 52.0)), api.rotation_about("y", 15.0, centre, (56.0, 52.0, 54.0))], L.STAMP_REPLACE, lo, hi)
    before = grid
    grid, counts = check(model, model, recs, grid, grid, pal)
    assert counts["changed"].all() and not np.array_equal(grid, before)


def test_palette_map_and_the_source_is_left_alone():
    src_grid = random_region(73, 0.5, (16, 16, 16), (20, 20, 20), materials=(1, 40))
    dst_grid = random_region(74, 0.3, (100, 100, 100), (30, 30, 30))
    pal = synth.make_palette(29)
    ctx = api.Context(device=0)
    rng = np.random.default_rng(75)
    permutation = rng.permutation(255).astype(np.uint8)
    many_to_one = (np.arange(255) % 3 + 200).astype(np.uint8)
    lo, hi = (16, 16, 16), (35, 35, 35)
    origins = np.stack([np.full(256, 300.0), np.repeat(np.linspace(-50, -30, 16), 16), np.tile(np.linspace(55, 75, 16), 16)], axis=1).astype(np.float32)
    directions = np.tile(np.float32([-1.0, 0.01, 0.02]), (256, 1))
    # a source that is not editable: it stays as it was created, and a scene committed on it keeps answering
    fixed_source = make(ctx, src_grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(fixed_source, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    assert np.count_nonzero(hits["instance"] != L.NO_HIT) > 20
    source_bytes = [a.tobytes() for a in fixed_source.read()]
    dst = make(ctx, dst_grid, pal)
    turn = api.rotation_about("z", 30.0, (26, 26, 26), (112.0, 112.0, 112.0))
    grid, _ = check(dst, fixed_source, api.resamples(turn, L.STAMP_OVERWRITE, lo, hi), dst_grid, src_grid, pal, permutation)
    grid, _ = check(dst, fixed_source, api.resamples(api.rotation_about("x", 70.0, (26, 26, 26), (118.0, 116.0, 120.0)), L.STAMP_PLACE, lo, hi), grid, src_grid, pal, many_to_one)
    assert set(np.unique(grid[100:140, 100:140, 100:140])) >= {201, 202, 203}
    dry = dst.resample(fixed_source, api.resamples(turn, L.STAMP_REPLACE, lo, hi), permutation, dry_run=True)
    assert dry.tolist() == R.resample(grid, src_grid, api.resamples(turn, L.STAMP_REPLACE, lo, hi), permutation, dry_run=True)[1].tolist()
    assert [a.tobytes() for a in fixed_source.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit: the source's generation has not moved
    assert status_of(lambda: fixed_source.island_of([(16, 16, 16)])) == L.ERR_NOT_READY
    # an editable source is read in place: an edit between two calls shows in the second
    loose = make(ctx, src_grid, pal)
    loose.set_voxels([(26, 26, 26)], [7])
    edited = src_grid.copy()
    edited[26, 26, 26] = 8
    grid, _ = check(dst, loose, api.resamples(turn, L.STAMP_REPLACE, lo, hi), grid, edited, pal, permutation)
    assert same_bytes(loose, edited, pal)


def test_dry_run():
    """the fit test of a rotated prefab: counts per record against the untouched destination, nothing moves"""
    terrain = np.zeros((256,) * 3, np.uint8)
    terrain[:, 0:100, :] = 3
    terrain[100:120, 100:140, 90:110] = 5                                        # a pillar
    piece_grid = random_region(76, 0.8, (8, 8, 8), (24, 12, 16), materials=(10, 20))
    pal = synth.make_palette(30)
    ctx = api.Context(device=0)
    model, piece = make(ctx, terrain, pal), make(ctx, piece_grid, pal)
    lo, hi = (8, 8, 8), (31, 19, 23)
    centre = (20.0, 14.0, 16.0)
    fits = api.rotation_about("y", 30.0, centre, (60.0, 114.0, 60.0))            # well above the ground, away from the pillar
    sunk = api.rotation_about("y", 30.0, centre, (60.0, 101.0, 60.0))            # shifted into the terrain
    recs = api.resamples([fits, sunk, api.rotation_about("y", 30.0, centre, (105.0, 114.0, 100.0))], [L.STAMP_PLACE, L.STAMP_OVERWRITE, L.STAMP_REPLACE], lo, hi)
    model.find_islands(L.ISLANDS_FACES, capacity=0)
    flood = model.flood([(0, 200, 0)], max_steps=40)
    probe = [(0, 200, 0), (5, 200, 5), (60, 114, 60)]
    steps = model.flood_at(probe)
    islands = model.island_of([(50, 50, 50), (105, 120, 100)])
    origins = np.stack([np.full(64, 300.0), np.repeat(np.linspace(-50, 40, 8), 8), np.tile(np.linspace(0, 80, 8), 8)], axis=1).astype(np.float32)
    directions = np.tile(np.float32([-1.0, 0.01, 0.02]), (64, 1))
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    dry = model.resample(piece, recs, dry_run=True)
    for k in range(3):                                                           # each against the untouched destination
        assert dry[k:k + 1].tolist() == R.resample(terrain, piece_grid, recs[k:k + 1])[1].tolist()
    assert dry["blocked"][0] == 0 and dry["solid"][0] > 2000 and dry["changed"][0] == dry["solid"][0]
    assert dry["blocked"][1] > 0 and dry["blocked"][2] > 0
    assert same_bytes(model, terrain, pal)
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()     # the generation has not moved
    assert model.island_of([(50, 50, 50), (105, 120, 100)]).tolist() == islands.tolist() and model.flood_at(probe).tolist() == steps.tolist()
    assert flood["reached"] > 0
    # the real call afterwards gives the dry run's counts for a single record
    real = model.resample(piece, recs[0:1])
    assert real.tolist() == dry[0:1].tolist()
    assert status_of(lambda: model.island_of([(50, 50, 50)])) == L.ERR_NOT_READY and status_of(lambda: model.flood_at(probe)) == L.ERR_NOT_READY
    # a dry run moves a model that is not editable yet into its editable form, as cast does, and changes no voxel
    fresh = make(ctx, terrain, pal)
    assert fresh.resample(piece, recs, dry_run=True).tolist() == dry.tolist() and same_bytes(fresh, terrain, pal)
    # held against itself: read in place
    own = model.resample(model, api.resamples(api.rotation_about("y", 10.0, (60.0, 114.0, 60.0), (60.0, 114.0, 60.0)), L.STAMP_REPLACE, (40, 100, 40), (80, 130, 80)), dry_run=True)
    grid = R.resample(terrain, piece_grid, recs[0:1])[0]
    assert own.tolist() == R.resample(grid, grid, api.resamples(api.rotation_about("y", 10.0, (60.0, 114.0, 60.0), (60.0, 114.0, 60.0)), L.STAMP_REPLACE, (40, 100, 40), (80, 130, 80)),
                                      dry_run=True)[1].tolist()


def test_chunking_and_the_record_limit():
    """answers known without the witness: whole-tree REPLACE records that alternate the identity and an x mirror of a half-solid source
    (more than 2^21 cell-list entries: at least two launches), then exactly DUST_HIP_MAX_RESAMPLES single-voxel records"""
    pal = synth.make_palette(31)
    ctx = api.Context(device=0)
    one = api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal)

    def filled(lo, hi, palette):
        m = api.Model(ctx, *one, pal)
        m.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0]] + [list(b) for b in lo], [[256, 256, 256]] + [list(b) for b in hi],
                                      op=[L.EDIT_CARVE] + [L.EDIT_FILL] * len(lo), palette=[0] + list(palette)))
        return m

    src = filled([(0, 0, 0)], [(128, 256, 256)], [9])
    dst = filled([], [], [])
    assert 520 * 4096 > 1 << 21
    identity = R.records([EYE], [(0, 0, 0)], (0, 0, 0), (255, 255, 255), L.STAMP_REPLACE)
    mirror = R.records([EYE * np.array([-1, 1, 1])[:, None]], [(256 * R.ONE, 0, 0)], (0, 0, 0), (255, 255, 255), L.STAMP_REPLACE)
    recs = np.concatenate([identity, mirror] * 260)
    counts = dst.resample(src, recs)
    assert counts["changed"].tolist() == [1 << 23] + [1 << 24] * 519
    assert counts["covered"].tolist() == [1 << 24] * 520 and counts["solid"].tolist() == [1 << 23] * 520
    assert counts["blocked"].tolist() == [0] * 520                                # each image is solid exactly where the one before was empty
    want = filled([(128, 0, 0)], [(256, 256, 256)], [9])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), want.read()))
    # exactly the limit: one voxel of the source onto 65 536 distinct empty voxels
    x, y, z = np.meshgrid(np.arange(16), np.arange(64), np.arange(64), indexing="ij")
    targets = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)
    rng = np.random.default_rng(77)
    targets = targets[rng.permutation(len(targets))]
    assert len(targets) == L.MAX_RESAMPLES
    single = R.records(np.broadcast_to(EYE, (len(targets), 3, 3)), (5 - targets) * R.ONE, targets, targets, L.STAMP_PLACE, (5, 5, 5), (5, 5, 5))
    assert dst.resample(src, single).tolist() == [(1, 1, 1, 0)] * L.MAX_RESAMPLES
    want = filled([(128, 0, 0), (0, 0, 0)], [(256, 256, 256), (16, 64, 64)], [9, 9])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), want.read()))
    assert dst.resample(src, single, dry_run=True).tolist() == [(0, 1, 1, 1)] * L.MAX_RESAMPLES       # PLACE over solid
    over = np.concatenate([single, single[:1]])
    assert status_of(lambda: dst.resample(src, over)) == L.ERR_INVALID_ARGUMENT
    assert status_of(lambda: dst.resample(src, over, dry_run=True)) == L.ERR_INVALID_ARGUMENT
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dst.read(), want.read()))


def test_refusals_and_states():
    src_grid = random_region(78, 0.5, (0, 0, 0), (12, 12, 12), materials=(1, 100))
    dst_grid = random_region(79, 0.5, (4, 4, 4), (12, 12, 12))
    pal = synth.make_palette(32)
    ctx = api.Context(device=0)
    lib = L.load()
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    good = R.records([EYE], [(-2 * R.ONE,) * 3], (2, 2, 2), (13, 13, 13), L.STAMP_REPLACE, (0, 0, 0), (11, 11, 11))
    counts = np.full(8, 77, np.uint32)
    cp = counts.ctypes.data_as(C.c_void_p)
    fn = lib.dust_hip_model_resample

    def call(d, s, recs, n, palette_map=None, flags=0):
        return fn(d, s, None if recs is None else recs.ctypes.data_as(C.c_void_p), n, None if palette_map is None else palette_map.ctypes.data_as(C.c_void_p), flags, cp)

    bad = []
    for op in (5, 0xFFFFFFFF):
        r = np.concatenate([good, good])
        r["op"][1] = op
        bad.append(r)
    for field, value in (("m", R.MAX_M + 1), ("t", -R.MAX_T - 1)):
        r = np.concatenate([good, good])
        r[field][1].reshape(-1)[0] = value
        bad.append(r)
    for r in bad:
        for flags in (0, L.RESAMPLE_DRY_RUN):
            assert call(dst._h, src._h, r, 2, flags=flags) == L.ERR_INVALID_ARGUMENT
    for flags in (2, 3, 1 << 31):
        assert call(dst._h, src._h, good, 1, flags=flags) == L.ERR_INVALID_ARGUMENT
    assert call(None, src._h, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, None, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, src._h, None, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, src._h, good, L.MAX_RESAMPLES + 1) == L.ERR_INVALID_ARGUMENT
    palette_map = np.arange(255, dtype=np.uint8)
    palette_map[254] = 255
    assert call(dst._h, src._h, good, 1, palette_map) == L.ERR_INVALID_ARGUMENT
    other_ctx = api.Context(device=0)
    foreign = make(other_ctx, src_grid, pal)
    assert call(dst._h, foreign._h, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(foreign._h, src._h, good, 1) == L.ERR_INVALID_ARGUMENT
    assert counts.tolist() == [77] * 8
    assert same_bytes(dst, dst_grid, pal) and same_bytes(foreign, src_grid, pal)
    assert status_of(lambda: dst.island_of([(0, 0, 0)])) == L.ERR_NOT_READY

    # unsupported exactly where stamp is, for either model, before the records are looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(src_grid, pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        for flags in (0, L.RESAMPLE_DRY_RUN):
            assert call(dst._h, unsupported._h, good, 1, flags=flags) == L.ERR_UNSUPPORTED
            assert call(unsupported._h, src._h, good, 1, flags=flags) == L.ERR_UNSUPPORTED
            assert call(dst._h, unsupported._h, bad[0], 2, flags=flags) == L.ERR_UNSUPPORTED
            assert call(unsupported._h, src._h, None, 0, flags=flags) == L.ERR_UNSUPPORTED
    assert same_bytes(dst, dst_grid, pal) and counts.tolist() == [77] * 8

    # n == 0: a no-op that may make dst editable, and leaves a labelling alone
    dst.find_islands(L.ISLANDS_FACES, capacity=0)
    assert call(dst._h, src._h, None, 0) == L.OK and call(dst._h, src._h, good, 0, palette_map) == L.ERR_INVALID_ARGUMENT
    assert dst.resample(src, good[:0]).tolist() == [] and same_bytes(dst, dst_grid, pal)
    assert dst.island_of([(200, 200, 200)]).tolist() == [L.NO_ISLAND]
    # counts may be NULL
    assert fn(dst._h, src._h, good.ctypes.data_as(C.c_void_p), 1, None, L.RESAMPLE_DRY_RUN, None) == L.OK
    assert dst.island_of([(200, 200, 200)]).tolist() == [L.NO_ISLAND]                   # a dry run leaves the labelling alone
    assert fn(dst._h, src._h, good.ctypes.data_as(C.c_void_p), 1, None, 0, None) == L.OK
    grid, _ = R.resample(dst_grid, src_grid, good)
    assert same_bytes(dst, grid, pal)
    assert status_of(lambda: dst.island_of([(200, 200, 200)])) == L.ERR_NOT_READY      # a real call with n > 0 invalidates it
    # an empty source: REPLACE clears the image, PLACE changes nothing
    empty = make(ctx, EMPTY, pal)
    whole = R.records([EYE], [(0, 0, 0)], (0, 0, 0), (255, 255, 255), L.STAMP_PLACE)
    assert dst.resample(empty, whole).tolist() == [(0, 1 << 24, 0, 0)]
    whole["op"] = L.STAMP_REPLACE
    assert dst.resample(empty, whole).tolist() == [(int(np.count_nonzero(grid)), 1 << 24, 0, 0)]
    assert len(dst.read()[0]) == 0 and same_bytes(dst, EMPTY, pal)


def test_determinism():
    src_grid = random_region(80, 0.5, (10, 10, 10), (40, 40, 40))
    dst_grid = random_region(81, 0.5, (60, 60, 60), (60, 60, 60))
    pal = synth.make_palette(33)
    ctx = api.Context(device=0)
    src = make(ctx, src_grid, pal)
    centre = (30.0, 30.0, 30.0)
    recs = api.resamples([api.rotation_about((3, 1, 2), 10.0 + 25.0 * k, centre, (80.0 + 3 * k, 88.0, 90.0 - 2 * k), scale=1.0 + 0.2 * k) for k in range(6)],
                         [k % 5 for k in range(6)], (10, 10, 10), (49, 49, 49))
    runs = []
    for _ in range(2):
        model = make(ctx, dst_grid, pal)
        counts = model.resample(src, recs)
        runs.append((counts.tobytes(), [a.tobytes() for a in model.read()]))
    assert runs[0] == runs[1] and np.frombuffer(runs[0][0], np.uint32).reshape(-1, 4)[:, 0].all()
