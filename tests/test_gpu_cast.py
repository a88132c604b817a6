"""Model casts on the device (dust_hip_model_cast; the contract is in include/dust_hip.h). Every comparison is exact: the hits must be,
byte for byte, those of tests/cast_witness.py (the header's definitions as whole-array numpy, one placement at a time: the opposite
direction from the kernel's per-voxel walk)."""
import ctypes as C

import numpy as np
import pytest

import cast_witness as CW
import island_witness as W
import stamp_witness as S
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
BOTTOM = ((0, 0, 0), (255, 0, 255))
EMPTY = np.zeros((256,) * 3, np.uint8)
AXIS_STEPS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
DIAGONALS = [(1, 1, 0), (-1, 0, -1), (0, -1, 1)]


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


def same_hits(got, want):
    assert got.dtype.itemsize == want.dtype.itemsize == 32 and len(got) == len(want)
    if got.tobytes() != want.tobytes():
        i = next(k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes())
        raise AssertionError(f"hit {i} of {len(got)}: device {got[i]} != witness {want[i]}")


def check(dst, src, casts, dst_grid, src_grid):
    """one call on the device and in the witness: the same bytes; returns the hits"""
    got = dst.cast(src, casts)
    same_hits(got, CW.cast(dst_grid, src_grid, casts))
    return got


def orientation_casts():
    """48 orientations x (6 axis steps + 3 diagonals) of the 5 x 6 x 7 piece. Every image box begins at 13 modulo 16 on every axis, so it
    straddles a brick and a root-cell boundary on all three; a quarter begin inside the filled region (they overlap it), the others just
    outside one of its faces (stepping towards it they hit, stepping away or along it they do not)"""
    offsets, words, steps = [], [], []
    for oi, word in enumerate(S.all_orientations()):
        for si, step in enumerate(AXIS_STEPS + DIAGONALS):
            a, b = 13 + 16 * (oi % 8), 13 + 16 * ((oi // 8) % 6)
            offsets.append([(13 + 32 * (oi % 4), 13 + 32 * ((oi // 4) % 4), 13 + 32 * (oi // 16)), (157, a, b), (a, 157, b), (a, b, 125)][(oi + si) % 4])
            words.append(word)
            steps.append(step)
    return offsets, words, steps


def test_orientations_and_steps_across_brick_and_root_cell_boundaries():
    rng = np.random.default_rng(81)
    box = (1 + np.arange(210, dtype=np.uint8)).reshape(5, 6, 7)
    box[rng.random(box.shape) < 1 / 3] = 0
    src_grid = np.zeros((256,) * 3, np.uint8)
    src_grid[3:8, 9:15, 14:21] = box
    dst_grid = random_region(82, 0.05, (0, 0, 0), (144, 144, 112))
    pal = synth.make_palette(31)
    ctx = api.Context(device=0)
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)     # dst fresh from dust_hip_model_create: the call makes it editable
    offsets, words, steps = orientation_casts()
    casts = api.casts(offsets, steps, 40, words, 0, (3, 9, 14), (7, 14, 20))
    assert len(casts) == 48 * 9 and casts.tobytes() == CW.records(offsets, steps, 40, words, 0, (3, 9, 14), (7, 14, 20)).tobytes()
    for c in casts:
        p, _ = S.orient_fields(c["orient"])
        for r in range(3):
            assert int(c["offset"][r]) % 16 == 13 and (5, 6, 7)[p[r]] > 3
    want = CW.cast(dst_grid, src_grid, casts)
    hit, overlap = (want["flags"] & L.CAST_HIT) != 0, (want["flags"] & L.CAST_OVERLAP) != 0
    # the mix, on the witness's output: the cases cannot silently degenerate
    assert np.count_nonzero(~hit) >= 20 and np.count_nonzero(hit & ~overlap) >= 20 and np.count_nonzero(overlap) >= 20
    assert np.count_nonzero(want["contacts"] > 1) >= 10 and (want["voxels"] == np.count_nonzero(box)).all()
    same_hits(dst.cast(src, casts), want)
    same_hits(dst.cast(src, casts), want)          # again, dst editable now: deterministic
    assert same_bytes(src, src_grid, pal) and same_bytes(dst, dst_grid, pal)


def test_walls_and_clipping():
    src_grid = random_region(83, 0.6, (20, 20, 20), (9, 10, 11))
    src_grid[20, 20, 20] = 9
    dst_grid = random_region(84, 0.02, (60, 0, 60), (80, 80, 80))
    dst_grid[:, :, 200:] = 0
    pal = synth.make_palette(32)
    ctx = api.Context(device=0)
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    lo, hi = (20, 20, 20), (28, 29, 30)
    turn = api.orientation((2, 0, 1), (True, False, True))
    for walls in (0, L.CAST_WALLS):
        casts = np.concatenate([
            # begins entirely outside the tree and enters it: through the fill, and through the empty slab z >= 200
            api.casts([(-15, 30, 90), (-15, 30, 210), (90, 30, 270)], [(1, 0, 0), (1, 0, 0), (0, 0, -1)], 300, [api.ORIENT_IDENTITY, turn, turn], walls, lo, hi),
            # leaves the tree: +x from inside the empty slab, +z out of its far face, and diagonally through an edge
            api.casts([(230, 40, 220), (100, 40, 230), (235, 240, 225)], [(1, 0, 0), (0, 0, 1), (1, 1, 0)], 60, [turn, api.ORIENT_IDENTITY, turn], walls, lo, hi),
            # comes to rest on the floor y = 0
            api.casts([(20, 37, 215), (200, 5, 230)], (0, -1, 0), 255, [api.ORIENT_IDENTITY, turn], walls, lo, hi),
        ])
        hits = check(dst, src, casts, dst_grid, src_grid)
        if walls:
            assert (hits["flags"][:3] == (L.CAST_HIT | L.CAST_OVERLAP | L.CAST_HIT_WALL)).all()       # outside the tree is blocked at once
            assert (hits["flags"][3:] == (L.CAST_HIT | L.CAST_HIT_WALL)).all()
            assert hits["contact"][3][0] == 256 and hits["contact"][4][2] == 256 and 256 in hits["contact"][5][:2].tolist()
            assert hits["steps"][6] == 37 and hits["contact"][6][1] == -1 and hits["steps"][7] == 5   # the floor
        else:
            assert hits["flags"][0] == L.CAST_HIT and hits["steps"][0] > 15                            # entered the tree, met the fill
            assert (hits["flags"][[1, 3, 4, 5, 6, 7]] == 0).all()                                      # through the empty slab and out of the tree
    assert status_of(lambda: src.island_of([(20, 20, 20)])) == L.ERR_NOT_READY


def test_fit_tests_over_a_grid_of_offsets():
    """max_steps = 0: does the prefab fit here, and if not, how many voxels collide"""
    prefab = np.zeros((256,) * 3, np.uint8)
    prefab[0:12, 0:10, 0:12] = 6
    prefab[2:10, 0:8, 2:10] = 0                    # a hollow hut, open at the bottom
    dst_grid = np.zeros((256,) * 3, np.uint8)
    dst_grid[60:170, 30:40, 60:170] = 2
    dst_grid[100:140, 40:46, 100:140] = random_region(85, 0.3, (100, 40, 100), (40, 6, 40))[100:140, 40:46, 100:140]
    pal = synth.make_palette(33)
    ctx = api.Context(device=0)
    src, dst = make(ctx, prefab, pal), make(ctx, dst_grid, pal)
    gx, gy, gz = np.meshgrid(70 + 8 * np.arange(10), 38 + np.arange(5), 70 + 8 * np.arange(10), indexing="ij")
    offsets = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)
    hits = check(dst, src, api.casts(offsets, (0, -1, 0), 0, src_lo=(0, 0, 0), src_hi=(11, 9, 11)), dst_grid, prefab)
    fits = hits["flags"] == 0
    assert np.count_nonzero(fits) > 50 and (hits["flags"][~fits] == (L.CAST_HIT | L.CAST_OVERLAP)).all() and np.count_nonzero(~fits) > 100
    assert (hits["contacts"][fits] == 0).all() and np.count_nonzero(hits["contacts"] > 1) > 100 and (hits["steps"] == 0).all()
    buried = hits[offsets[:, 1] == 38]             # two layers into the ground: both wall courses collide, whatever stands above
    assert (buried["contacts"] >= 2 * (144 - 64)).all()


def test_degenerate_inputs():
    src_grid = random_region(86, 0.5, (8, 8, 8), (6, 6, 6))
    dst_grid = random_region(87, 0.2, (0, 0, 0), (64, 64, 64))
    pal = synth.make_palette(34)
    ctx = api.Context(device=0)
    src, dst, none = make(ctx, src_grid, pal), make(ctx, dst_grid, pal), make(ctx, EMPTY, pal)
    lo, hi = (8, 8, 8), (13, 13, 13)
    lim = 2 ** 31
    casts = np.concatenate([
        api.casts([(10, 10, 10), (70, 70, 70), (10, 10, 10)], (0, 0, 0), [500, 500, 0], flags=[0, 0, L.CAST_WALLS], src_lo=lo, src_hi=hi),     # a zero step
        api.casts([(10, 10, 10)] * 2, (0, -1, 0), 30, flags=[0, L.CAST_WALLS], src_lo=[(14, 8, 8), (8, 8, 13)], src_hi=[(13, 13, 13), (13, 13, 12)]),
        api.casts([(10, 10, 10)] * 2, (0, -1, 0), 30, flags=[0, L.CAST_WALLS], src_lo=(100, 100, 100), src_hi=(140, 140, 140)),       # an empty piece
        # the int32 limits: nothing to walk, whatever max_steps says
        api.casts([(lim - 1, 10, 10), (-lim, 10, 10), (10, -lim, lim - 1), (-lim + 70000, 10, 10), (10, 10, lim - 1)],
                  [(-1, 0, 0), (1, 0, 0), (0, 1, -1), (1, 0, 0), (0, 0, 1)], L.CAST_MAX_STEPS, api.orientation((1, 2, 0), (True, True, False)),
                  [0, L.CAST_WALLS, 0, L.CAST_WALLS, L.CAST_WALLS], lo, hi),
        # ... and a long walk that does arrive: 65 535 steps allowed, the tree is 300 away
        api.casts([(-300, 10, 10), (10, 10, 400)], [(1, 0, 0), (0, 0, -1)], L.CAST_MAX_STEPS, src_lo=lo, src_hi=hi),
    ])
    hits = check(dst, src, casts, dst_grid, src_grid)
    assert hits["flags"][0] & L.CAST_OVERLAP and hits["steps"][0] == 0 and hits["flags"][1] == 0 and hits["steps"][1] == 500
    assert (hits["voxels"][3:7] == 0).all() and (hits["flags"][3:7] == 0).all() and (hits["steps"][3:7] == 30).all()
    assert hits["flags"][7] == 0 and hits["steps"][7] == L.CAST_MAX_STEPS and hits["flags"][8] == (L.CAST_HIT | L.CAST_OVERLAP | L.CAST_HIT_WALL)
    assert (hits["flags"][-2:] == L.CAST_HIT).all() and (hits["steps"][-2:] > 230).all()
    # an empty source model, an empty destination, and no casts at all
    assert (check(dst, none, casts, dst_grid, EMPTY)["voxels"] == 0).all()
    check(none, src, casts, EMPTY, src_grid)
    assert len(dst.cast(src, casts[:0])) == 0
    assert L.load().dust_hip_model_cast(dst._h, src._h, None, 0, None) == L.OK


def test_pruning_does_not_leak():
    """a tall piece of many bricks over three root cells, cast at a staircase: its first-listed bricks hit late and its last-listed early,
    then the other way round. What another wave has published may shorten a walk but never changes an answer: two runs, the same bytes"""
    src_grid = np.zeros((256,) * 3, np.uint8)
    src_grid[8:14, 10:54, 8:14] = 3
    rng = np.random.default_rng(88)
    src_grid[8:14, 10:54, 8:14][rng.random((6, 44, 6)) < 0.2] = 0
    pal = synth.make_palette(35)
    ctx = api.Context(device=0)
    src = make(ctx, src_grid, pal)
    for rising in (True, False):
        dst_grid = np.zeros((256,) * 3, np.uint8)
        for y in range(100, 150):
            dst_grid[(60 + (y - 100) * 2 if rising else 160 - (y - 100) * 2):200, y, 90:130] = 4
        dst = make(ctx, dst_grid, pal)
        casts = api.casts([(20, 103, 100), (20, 103, 100), (20, 101, 98)], (1, 0, 0), [255, 255, 40], [api.ORIENT_IDENTITY, api.orientation((0, 1, 2), (False, True, False)),
                                                                                                     api.ORIENT_IDENTITY], 0, (8, 10, 8), (13, 53, 13))
        first = check(dst, src, casts, dst_grid, src_grid)
        assert (first["flags"][:2] == L.CAST_HIT).all() and first["steps"][0] > 20
        for _ in range(3):
            assert dst.cast(src, casts).tobytes() == first.tobytes()


def test_independence_and_chunking():
    src_grid = random_region(89, 0.3, (30, 30, 30), (10, 10, 10))
    dst_grid = random_region(90, 0.01, (0, 0, 0), (128, 128, 128))
    pal = synth.make_palette(36)
    ctx = api.Context(device=0)
    src, dst = make(ctx, src_grid, pal), make(ctx, dst_grid, pal)
    # whole-tree sub-boxes: 4 096 work items each, 300 of them pass one launch chunk (2^20 items)
    n = 300
    assert n * 4096 > 1 << 20
    rng = np.random.default_rng(91)
    words = np.array(S.all_orientations(), np.uint32)[rng.integers(0, 48, n)]
    steps = np.array(AXIS_STEPS + DIAGONALS)[rng.integers(0, 9, n)]
    casts = api.casts(rng.integers(-40, 40, (n, 3)), steps, rng.integers(0, 50, n), words, rng.integers(0, 2, n))
    together = dst.cast(src, casts)
    apart = np.concatenate([dst.cast(src, casts[k:k + 1]) for k in range(n)])
    assert together.tobytes() == apart.tobytes()
    assert len(set(together["steps"].tolist())) > 10 and (together["voxels"] == np.count_nonzero(src_grid)).all()
    same_hits(together[:2], CW.cast(dst_grid, src_grid, casts[:2]))      # (a whole-tree image is slow in the witness: two of them)
    # exactly the limit: 65 536 debris pieces of up to eight voxels
    n = L.MAX_CASTS
    corner = rng.integers(30, 39, (n, 3))
    casts = api.casts(rng.integers(-4, 132, (n, 3)), np.array(AXIS_STEPS + DIAGONALS)[rng.integers(0, 9, n)], 16,
                      np.array(S.all_orientations(), np.uint32)[rng.integers(0, 48, n)], rng.integers(0, 2, n), corner, corner + 1)
    hits = dst.cast(src, casts)
    sample = rng.choice(n, 1024, replace=False)       # 1 024 of the 65 536 in the witness: for speed, the comparison is still exact
    same_hits(hits[sample], CW.cast(dst_grid, src_grid, casts[sample]))
    assert np.count_nonzero(hits["flags"] & L.CAST_HIT) > 1000 and np.count_nonzero(hits["flags"] == 0) > 1000
    over = np.concatenate([casts, casts[:1]])
    assert status_of(lambda: dst.cast(src, over)) == L.ERR_INVALID_ARGUMENT


def test_states_and_refusals():
    src_grid = random_region(92, 0.5, (16, 16, 16), (12, 12, 12), materials=(1, 100))
    dst_grid = random_region(93, 0.1, (0, 0, 0), (48, 48, 48))
    dst_grid[200:204, 200:204, 200:204] = 5       # a second island
    pal = synth.make_palette(37)
    ctx = api.Context(device=0)
    lib = L.load()
    lo, hi = (16, 16, 16), (27, 27, 27)
    origins = np.stack([np.full(256, 300.0), np.repeat(np.linspace(-50, -30, 16), 16), np.tile(np.linspace(55, 75, 16), 16)], axis=1).astype(np.float32)
    directions = np.tile(np.float32([-1.0, 0.01, 0.02]), (256, 1))
    good = api.casts([(60, 20, 20)], (-1, 0, 0), 100, src_lo=lo, src_hi=hi)

    # a source that is not editable stays so, and a scene committed on it keeps answering without a new commit
    fixed = make(ctx, src_grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(fixed, ROTATED.reshape(12))
    scene.commit()
    traced = scene.trace_rays(origins, directions)
    assert np.count_nonzero(traced["instance"] != L.NO_HIT) > 20
    source_bytes = [a.tobytes() for a in fixed.read()]
    dst = make(ctx, dst_grid, pal)
    assert check(dst, fixed, good, dst_grid, src_grid)["flags"][0] == L.CAST_HIT
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == traced.tobytes()
    assert status_of(lambda: fixed.island_of([(16, 16, 16)])) == L.ERR_NOT_READY       # not made editable

    # on an editable dst nothing a scene reads changes, and a standing labelling and flood field still answer
    n_islands, rec = dst.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    labelled = dst.island_of([(200, 200, 200), (100, 100, 100)])
    flood = dst.flood([(100, 100, 100)], L.FLOOD_EMPTY, max_steps=20)
    probes = [(100, 100, 100), (100, 105, 102), (200, 200, 200)]
    field = dst.flood_at(probes)
    scene2 = api.Scene(ctx)
    scene2.add_instance(dst, ROTATED.reshape(12))
    scene2.commit()
    traced2 = scene2.trace_rays(origins, directions)
    check(dst, fixed, good, dst_grid, src_grid)
    assert scene2.trace_rays(origins, directions).tobytes() == traced2.tobytes()
    assert dst.island_of([(200, 200, 200), (100, 100, 100)]).tolist() == labelled.tolist() and labelled[0] != L.NO_ISLAND
    assert dst.flood_at(probes).tolist() == field.tolist() == [0, 7, L.FLOOD_UNREACHED] and flood["reached"] > 0
    assert same_bytes(dst, dst_grid, pal) and n_islands == len(rec)

    # src == dst is not special: the piece meets its own voxels
    own = api.casts([(16, 16, 16), (16, 40, 16)], (0, -1, 0), 50, src_lo=lo, src_hi=hi)
    loose = make(ctx, src_grid, pal)
    hits = check(loose, loose, own, src_grid, src_grid)
    assert hits["flags"][0] == (L.CAST_HIT | L.CAST_OVERLAP) and hits["contacts"][0] == hits["voxels"][0] == np.count_nonzero(src_grid)
    assert hits["flags"][1] == L.CAST_HIT and same_bytes(loose, src_grid, pal)

    # every refusal, with hits untouched
    out = np.full(2, 0x5A, np.uint8).repeat(32).view(api.CAST_HIT_DTYPE)
    before = out.tobytes()
    fn = lib.dust_hip_model_cast

    def call(d, s, casts, n, hits=out):
        return fn(d, s, None if casts is None else casts.ctypes.data_as(C.c_void_p), n, None if hits is None else hits.ctypes.data_as(C.c_void_p))

    bad = []
    for field_name, values in (("orient", (0, 0x15, 0x3F, api.ORIENT_IDENTITY | 1 << 9, 0x27)), ("max_steps", (L.CAST_MAX_STEPS + 1, 0xFFFFFFFF)),
                               ("flags", (2, 3, 0x80000000))):
        for v in values:
            c = np.concatenate([good, good])
            c[field_name][1] = v
            bad.append(c)
    for r in range(3):
        for v in (2, -2, 2 ** 31 - 1, -2 ** 31):
            c = np.concatenate([good, good])
            c["step"][1][r] = v
            bad.append(c)
    for c in bad:
        assert call(dst._h, fixed._h, c, 2) == L.ERR_INVALID_ARGUMENT
    assert call(None, fixed._h, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, None, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, fixed._h, None, 1) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, fixed._h, good, 1, None) == L.ERR_INVALID_ARGUMENT
    assert call(dst._h, fixed._h, good, L.MAX_CASTS + 1) == L.ERR_INVALID_ARGUMENT
    other_ctx = api.Context(device=0)
    foreign = make(other_ctx, src_grid, pal)
    assert call(dst._h, foreign._h, good, 1) == L.ERR_INVALID_ARGUMENT
    assert call(foreign._h, fixed._h, good, 1) == L.ERR_INVALID_ARGUMENT
    # unsupported exactly where set_voxels is, for either model, before the records are looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(src_grid, pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        assert call(dst._h, unsupported._h, good, 1) == L.ERR_UNSUPPORTED
        assert call(unsupported._h, fixed._h, good, 1) == L.ERR_UNSUPPORTED
        assert call(dst._h, unsupported._h, bad[0], 2) == L.ERR_UNSUPPORTED
        assert call(unsupported._h, fixed._h, None, 0) == L.ERR_UNSUPPORTED
    assert out.tobytes() == before
    assert status_of(lambda: foreign.island_of([(0, 0, 0)])) == L.ERR_NOT_READY           # a refused call made nothing editable
    # reserved and the pad bytes are ignored
    noisy = good.copy()
    noisy["reserved"], noisy["pad0"], noisy["pad1"] = 0xDEADBEEF, 7, 9
    assert dst.cast(fixed, noisy).tobytes() == dst.cast(fixed, good).tobytes()


def test_the_loop_closed():
    """dig, ask what came loose, lift it out, let it fall, put it back: the piece comes to rest on the uneven ground below it"""
    terrain = np.zeros((256,) * 3, np.uint8)
    terrain[40:100, 0:6, 40:100] = 2
    terrain[66:70, 6:9, 62:66] = 3                       # a bump under the pillar: a box cast would stop here too, but ...
    terrain[60:72, 30:60, 60:72] = 5                     # the pillar,
    terrain[63:69, 24:30, 63:69] = 5                     # its narrower foot (it reaches down past the bump's top beside the bump),
    terrain[72:80, 56:60, 60:72] = 5                     # an arm,
    terrain[60:80, 60:64, 60:72] = 4                     # and what holds it up: a beam to a post that stands on the ground
    terrain[90:94, 6:64, 60:72] = 4
    pal = synth.make_palette(38)
    ctx = api.Context(device=0)
    model = make(ctx, terrain, pal)
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [60, 60, 60], [80, 64, 72]))        # the beam is carved away
    carved = terrain.copy()
    carved[60:80, 60:64, 60:72] = 0
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    floating = rec[(rec["flags"] & L.ISLAND_ANCHORED) == 0]
    assert n == 2 and len(floating) == 1
    piece = model.detach_islands(floating["key"])
    piece_grid = np.zeros_like(carved)
    piece_grid[60:80, 24:60, 60:72] = carved[60:80, 24:60, 60:72]
    rest = np.where(piece_grid != 0, 0, carved).astype(np.uint8)
    lo, hi = tuple(int(v) for v in floating["lo"][0]), tuple(int(v) for v in floating["hi"][0])
    assert lo == (60, 24, 60) and hi == (79, 59, 71) and int(floating["voxels"][0]) == np.count_nonzero(piece_grid)
    fall = api.casts([lo], (0, -1, 0), 255, flags=L.CAST_WALLS, src_lo=lo, src_hi=hi)
    hit = check(model, piece, fall, rest, piece_grid)[0]
    assert hit["flags"] == L.CAST_HIT and hit["steps"] == 24 - 9 and hit["contacts"] == 9       # the foot lands on the bump: 3 x 3 voxels of it
    at = [lo[r] + int(hit["steps"]) * int(fall["step"][0][r]) for r in range(3)]
    stamps = api.stamps([at], api.ORIENT_IDENTITY, L.STAMP_PLACE, lo, hi)
    changed = model.stamp(piece, stamps)
    grid, counts = S.stamp(rest, piece_grid, stamps)
    assert changed.tolist() == counts.tolist() == [np.count_nonzero(piece_grid)]
    assert same_bytes(model, grid, pal)
    # from its resting place it cannot move: blocked at the first step, but not overlapping where it stands (cast against the ground alone)
    ground = make(ctx, rest, pal)
    again = check(ground, piece, api.casts([at], (0, -1, 0), 255, flags=L.CAST_WALLS, src_lo=lo, src_hi=hi), rest, piece_grid)[0]
    assert again["steps"] == 0 and again["flags"] == L.CAST_HIT
