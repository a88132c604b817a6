"""Model deltas on the device (dust_hip_model_delta, dust_hip_model_delta_apply; the contract is in include/dust_hip.h). Every
comparison is exact: the result, the list and the tables must be, byte for byte, what the witness says (tests/delta_witness.py), an
apply must leave the model a host build of the witness's grid, and a delta call must leave both models as it found them."""
import ctypes as C
import functools

import numpy as np
import pytest

import delta_witness as W
import shape_edit_witness as SW
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)


def host_model(grid, pal):
    return api.flatten_model(to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def make_editable(model):
    model.find_islands(L.ISLANDS_FACES, capacity=0)          # the first-edit transition, and nothing else
    return model


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


def full(grid):
    out = np.zeros((256,) * 3, np.uint8)
    out[tuple(slice(0, n) for n in grid.shape)] = grid
    return out


@functools.lru_cache(maxsize=None)
def hand_built_pair():
    """single voxels at the two corners of the tree, one added and one removed; per axis, pairs across the brick edge 3 | 4 and the
    root-cell edge 15 | 16, one voxel repainted and the other removed; a whole brick repainted; a whole brick identical in both; a brick
    solid only before and one solid only after"""
    before, after = np.zeros((256,) * 3, np.uint8), np.zeros((256,) * 3, np.uint8)
    after[0, 0, 0] = 1                                        # added
    before[255, 255, 255] = 2                                 # removed
    for axis in range(3):
        for edge, at in ((3, 40), (15, 48)):
            a, b = [at + 8 * axis] * 3, [at + 8 * axis] * 3
            a[axis], b[axis] = edge + 64, edge + 65           # 67 | 68 and 79 | 80: the same edges, away from the other pieces
            before[tuple(a)], after[tuple(a)] = 3 + axis, 9 + axis      # repainted
            before[tuple(b)] = 4 + axis                                 # removed
    before[100:104, 104:108, 108:112], after[100:104, 104:108, 108:112] = 7, 8       # one brick exactly, repainted: equal brick words
    before[120:124, 104:108, 108:112], after[120:124, 104:108, 108:112] = 7, 7       # ... identical in both
    before[140:144, 104:108, 108:112] = 5                                            # ... solid only before
    after[160:164, 104:108, 108:112] = 6                                             # ... solid only after
    before.setflags(write=False)
    after.setflags(write=False)
    return before, after


@functools.lru_cache(maxsize=None)
def random_pair():
    """(before, after), 64^3 each -- the rest of the tree is empty. before: about 5 000 voxels of six materials in [0, 64)^3, a sparse
    scatter and a dense block across 15 | 16 and 31 | 32 (the recipe of the census and surface tests); after: a third of a block across
    15 | 16 and 31 | 32 changed at random among add, remove and repaint"""
    rng = np.random.default_rng(82)
    before = np.where(rng.random((64,) * 3) < 0.01, rng.integers(1, 7, (64,) * 3), 0).astype(np.uint8)
    before[13:27, 26:38, 14:20] = np.where(rng.random((14, 12, 6)) < 0.85, rng.integers(1, 7, (14, 12, 6)), 0)
    assert 3000 < np.count_nonzero(before) < 6000
    rng = np.random.default_rng(95)
    after = before.copy()
    block = after[10:36, 22:40, 10:24]                        # (a view)
    hit = rng.random(block.shape) < 1.0 / 3.0
    how = rng.integers(0, 3, block.shape)
    paint = (block + rng.integers(1, 6, block.shape) - 1) % 6 + 1          # another of the six materials
    block[...] = np.where(hit & (block == 0) & (how == 0), rng.integers(1, 7, block.shape),
                          np.where(hit & (block != 0) & (how == 1), 0, np.where(hit & (block != 0) & (how == 2), paint, block)))
    before.setflags(write=False)
    after.setflags(write=False)
    return before, after


def check(mb, ma, before, after, **query):
    """one query on the device and in the witness: result, full list and tables agree; returns them"""
    result, voxels, counts = mb.delta(ma, tables=True, **query)
    want_result, want_voxels, want_counts = W.delta(before, after, **query)
    assert result.dtype == api.DELTA_RESULT_DTYPE and voxels.dtype == api.DELTA_VOXEL_DTYPE and counts.shape == (2, 256) and counts.dtype == np.uint32
    assert result.tobytes() == want_result.tobytes(), (query, result, want_result)
    assert len(voxels) == len(want_voxels), (query, len(voxels), len(want_voxels))
    bad = np.flatnonzero(voxels != want_voxels)
    assert len(bad) == 0, (query, bad[:5], voxels[bad[:5]], want_voxels[bad[:5]])
    assert voxels.tobytes() == want_voxels.tobytes()
    assert np.array_equal(counts, want_counts), (query, np.argwhere(counts != want_counts)[:5])
    assert int(counts[0].sum()) == int(counts[1].sum()) == int(result["voxels"]) == int(result["added"]) + int(result["removed"]) + int(result["repainted"])
    assert int(counts[0, 0]) == int(result["added"]) and int(counts[1, 0]) == int(result["removed"])
    # counts only, and without tables: the same result
    alone, none, no_counts = mb.delta(ma, capacity=0, **query)
    assert alone.tobytes() == result.tobytes() and len(none) == 0 and no_counts is None
    return result, voxels, counts


def test_hand_built_pair():
    before, after = hand_built_pair()
    pal = synth.make_palette(61)
    ctx = api.Context(device=0)
    mb, ma = make(ctx, before, pal), make(ctx, after, pal)
    result, voxels, counts = check(mb, ma, before, after)
    assert [int(result[n]) for n in ("added", "removed", "repainted")] == [1 + 64, 1 + 6 + 64, 6 + 64]
    assert int(result["solid_before"]) == np.count_nonzero(before) and int(result["solid_after"]) == np.count_nonzero(after)
    assert result["lo"].tolist() == [0] * 3 and result["hi"].tolist() == [255] * 3
    by_key = {int(v["key"]): (int(v["kind"]), int(v["before"]), int(v["after"])) for v in voxels}
    assert by_key[0] == (L.DELTA_ADDED, L.DELTA_NONE, 0) and by_key[(255 << 16) | (255 << 8) | 255] == (L.DELTA_REMOVED, 1, L.DELTA_NONE)
    assert by_key[(67 << 16) | (40 << 8) | 40] == (L.DELTA_REPAINTED, 2, 8) and by_key[(68 << 16) | (40 << 8) | 40] == (L.DELTA_REMOVED, 3, L.DELTA_NONE)
    assert by_key[(56 << 16) | (79 << 8) | 56] == (L.DELTA_REPAINTED, 3, 9) and by_key[(64 << 16) | (64 << 8) | 80] == (L.DELTA_REMOVED, 5, L.DELTA_NONE)
    in_x = lambda lo: [k for k in by_key if lo <= k >> 16 < lo + 4 and 104 <= (k >> 8) & 255 < 108]
    assert {by_key[k] for k in in_x(100)} == {(L.DELTA_REPAINTED, 6, 7)} and len(in_x(100)) == 64          # only grid bytes show this one
    assert in_x(120) == []                                                                                # identical: nothing
    assert {by_key[k] for k in in_x(140)} == {(L.DELTA_REMOVED, 4, L.DELTA_NONE)} and len(in_x(140)) == 64
    assert {by_key[k] for k in in_x(160)} == {(L.DELTA_ADDED, L.DELTA_NONE, 5)} and len(in_x(160)) == 64
    for kinds in range(1, 7):
        check(mb, ma, before, after, kinds=kinds)
    for palette in (6, 7, 0, 1, 3, 200):                      # the repainted brick's two sides, the corners', a pair's, one nobody has
        part, part_voxels, _ = check(mb, ma, before, after, palette=palette)
        assert np.all((part_voxels["before"] == palette) | (part_voxels["after"] == palette)) and (palette == 200) == (len(part_voxels) == 0)
    check(ma, mb, after, before)                              # the other way round: added and removed change places
    for model, grid in ((mb, before), (ma, after)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def test_random_pair_kinds_filter_regions_and_tables():
    before, after = random_pair()
    pal = synth.make_palette(62)
    ctx = api.Context(device=0)
    mb, ma = make(ctx, full(before), pal), make(ctx, full(after), pal)
    rng = np.random.default_rng(96)
    total, _, _ = check(mb, ma, before, after)
    assert min(int(total[n]) for n in ("added", "removed", "repainted")) > 50
    for kinds in range(1, 7):
        check(mb, ma, before, after, kinds=kinds)
    for palette in (0, 2, 5, 6):
        check(mb, ma, before, after, palette=palette)
    regions = [((13, 26, 14), (26, 37, 19)), ((14, 27, 15), (25, 36, 18)), ((15, 0, 0), (16, 255, 255)), ((0, 31, 17), (63, 32, 17)), ((21, 29, 15), (21, 29, 15)),
               ((0, 0, 0), (63, 63, 63)), ((32, 32, 32), (255, 255, 255))]
    for _ in range(10):
        lo = rng.integers(0, 40, 3)
        regions.append((tuple(int(v) for v in lo), tuple(int(v) for v in lo + rng.integers(0, 30, 3))))
    listed = 0
    for k, region in enumerate(regions):
        result, _, _ = check(mb, ma, before, after, region=region, kinds=(7, 4, 3, 5, 2)[k % 5], palette=(-1, -1, 2, 5)[k % 4])
        listed += int(result["voxels"])
    assert listed > 1000
    zero = W.zero_result()
    for tables in (False, True):                               # an inverted region: legal, the zero result
        result, voxels, counts = mb.delta(ma, region=((9, 9, 9), (8, 200, 200)), tables=tables)
        assert result.tobytes() == zero.tobytes() and len(voxels) == 0 and (counts is None or not counts.any())


def test_capacity():
    before, after = random_pair()
    pal = synth.make_palette(63)
    ctx = api.Context(device=0)
    lib = L.load()
    mb, ma = make(ctx, full(before), pal), make(ctx, full(after), pal)
    region = ((10, 20, 10), (30, 40, 25))
    want_result, want, _ = W.delta(before, after, region=region)
    total = len(want)
    assert total > 500
    q = L.DeltaQuery(struct_size=C.sizeof(L.DeltaQuery), kinds=L.DELTA_ALL, palette=-1)
    q.lo[:], q.hi[:] = region
    for capacity in (0, 1, total - 1, total, total + 5):
        out = np.full((total + 8) * 8, 0x5A, np.uint8).view(api.DELTA_VOXEL_DTYPE)
        result = np.zeros(1, api.DELTA_RESULT_DTYPE)
        assert lib.dust_hip_model_delta(mb._h, ma._h, C.byref(q), result.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), capacity, None) == L.OK
        written = min(capacity, total)
        assert out[:written].tobytes() == want[:written].tobytes(), capacity
        assert out[written:].tobytes() == b"\x5a" * (8 * (total + 8 - written)), capacity
        assert result[0].tobytes() == want_result.tobytes(), capacity
    # through the Python call: a given capacity truncates, None lists everything
    assert mb.delta(ma, region=region, capacity=7)[1].tobytes() == want[:7].tobytes()
    assert mb.delta(ma, region=region)[1].tobytes() == want.tobytes()


def ray_grid(n=8):
    """n * n rays along -x over the image of [0, 64)^3 under ROTATED"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def test_editable_and_not_give_the_same_bytes_and_both_models_are_only_read():
    before, after = random_pair()
    pal = synth.make_palette(64)
    ctx = api.Context(device=0)
    origins, directions = ray_grid()
    points = [(13, 26, 14), (20, 30, 16), (200, 200, 200)]
    grids = {"before": full(before), "after": full(after)}
    host = {name: [a.tobytes() for a in host_model(grid, pal)] for name, grid in grids.items()}
    answers = []
    for edit_before in (False, True):
        for edit_after in (False, True):
            models = {"before": make(ctx, grids["before"], pal), "after": make(ctx, grids["after"], pal)}
            scenes, hits, derived = {}, {}, {}
            for name, editable in (("before", edit_before), ("after", edit_after)):
                m = models[name]
                if editable:
                    make_editable(m)
                    m.distance(max_radius=3)
                    m.flood([(100, 100, 100)], max_steps=90)
                    derived[name] = [m.island_of(points).tolist(), m.distance_at(points).tolist(), m.flood_at(points).tolist()]
                scenes[name] = api.Scene(ctx)
                scenes[name].add_instance(m, ROTATED.reshape(12))
                scenes[name].commit()
                hits[name] = scenes[name].trace_rays(origins, directions)
                assert np.count_nonzero(hits[name]["instance"] != L.NO_HIT) > 5
            got = check(models["before"], models["after"], before, after)
            got += check(models["before"], models["after"], before, after, kinds=L.DELTA_ADDED | L.DELTA_REMOVED)      # (masks only: no grid is made)
            got += check(models["before"], models["after"], before, after, kinds=L.DELTA_REPAINTED, palette=2, region=((14, 27, 15), (25, 36, 18)))
            answers.append(b"".join(a.tobytes() for a in got))
            for name, m in models.items():
                assert [a.tobytes() for a in m.read()] == host[name], (name, edit_before, edit_after)
                # no commit: the generation has not moved -- a model that was not editable has not become so
                assert scenes[name].trace_rays(origins, directions).tobytes() == hits[name].tobytes()
                if name in derived:                            # an editable model's labelling and both fields stand
                    assert [m.island_of(points).tolist(), m.distance_at(points).tolist(), m.flood_at(points).tolist()] == derived[name]
            if not edit_before:                                # the first-edit transition happens HERE, not in delta
                make_editable(models["before"])
                assert status_of(lambda: scenes["before"].trace_rays(origins, directions)) == L.ERR_NOT_READY
    assert len(set(answers)) == 1


def test_same_handle_two_contexts_and_refusals():
    before, after = random_pair()
    pal = synth.make_palette(65)
    ctx, other_ctx = api.Context(device=0), api.Context(device=0)
    lib = L.load()
    mb, ma, elsewhere = make(ctx, full(before), pal), make(ctx, full(after), pal), make(other_ctx, full(after), pal)
    zero = W.zero_result()
    for model in (mb, make_editable(make(ctx, full(before), pal))):          # the same handle twice: legal, the zero result
        result, voxels, counts = model.delta(model, tables=True)
        assert result.tobytes() == zero.tobytes() and len(voxels) == 0 and not counts.any()
    assert status_of(lambda: mb.delta(elsewhere)) == L.ERR_INVALID_ARGUMENT and status_of(lambda: elsewhere.delta(mb)) == L.ERR_INVALID_ARGUMENT

    result = np.full(64, 0x5A, np.uint8).view(api.DELTA_RESULT_DTYPE)
    voxels = np.full(16 * 8, 0x5A, np.uint8).view(api.DELTA_VOXEL_DTYPE)
    counts = np.full((2, 256), 0x5A5A5A5A, np.uint32)
    changed, conflicts = C.c_uint32(0x5A5A5A5A), C.c_uint32(0x5A5A5A5A)
    untouched = result.tobytes(), voxels.tobytes(), counts.tobytes()
    rp, vp, cp = (a.ctypes.data_as(C.c_void_p) for a in (result, voxels, counts))

    def query(kinds=7, flags=0, palette=-1, lo=(0, 0, 0), hi=(255, 255, 255), size=C.sizeof(L.DeltaQuery)):
        q = L.DeltaQuery(struct_size=size, kinds=kinds, flags=flags, palette=palette)
        q.lo[:], q.hi[:] = lo, hi
        return q
    bad = [query(kinds=0), query(kinds=8), query(flags=1), query(flags=1 << 31), query(palette=-2), query(palette=255), query(lo=(0, 256, 0)),
           query(hi=(255, 255, 256)), query(lo=(1 << 31, 0, 0)), query(size=47), query(size=0)]
    for q in bad:
        assert lib.dust_hip_model_delta(mb._h, ma._h, C.byref(q), rp, vp, 16, cp) == L.ERR_INVALID_ARGUMENT
    good = query()
    assert lib.dust_hip_model_delta(mb._h, ma._h, None, rp, vp, 16, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_delta(mb._h, None, C.byref(good), rp, vp, 16, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_delta(None, ma._h, C.byref(good), rp, vp, 16, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_delta(mb._h, elsewhere._h, C.byref(good), rp, vp, 16, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_delta(mb._h, ma._h, C.byref(good), rp, None, 16, cp) == L.ERR_INVALID_ARGUMENT        # null voxels with capacity > 0
    # delta_apply: a flag bit above 0, null records with n > 0, n above 2^24, a key of 2^24 or above
    records = np.zeros(16, api.DELTA_VOXEL_DTYPE)
    records["key"] = np.arange(16)
    records["after"] = 3
    wrong_key = records.copy()
    wrong_key["key"][9] = 1 << 24
    for call in (lambda: lib.dust_hip_model_delta_apply(mb._h, vp, 16, 2, C.byref(changed), C.byref(conflicts)),
                 lambda: lib.dust_hip_model_delta_apply(mb._h, vp, 16, 1 << 31, C.byref(changed), C.byref(conflicts)),
                 lambda: lib.dust_hip_model_delta_apply(mb._h, None, 16, 0, C.byref(changed), C.byref(conflicts)),
                 lambda: lib.dust_hip_model_delta_apply(mb._h, records.ctypes.data_as(C.c_void_p), (1 << 24) + 1, 0, C.byref(changed), C.byref(conflicts)),
                 lambda: lib.dust_hip_model_delta_apply(mb._h, wrong_key.ctypes.data_as(C.c_void_p), 16, 0, C.byref(changed), C.byref(conflicts))):
        assert call() == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), voxels.tobytes(), counts.tobytes()) == untouched and changed.value == conflicts.value == 0x5A5A5A5A
    for model, grid in ((mb, before), (ma, after)):            # no refused call touched a model
        assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(full(grid), pal)))
    # every output may be null; a larger struct_size is a newer caller's; no records is a no-op
    assert lib.dust_hip_model_delta(mb._h, ma._h, C.byref(query(size=64)), None, None, 0, None) == L.OK
    assert lib.dust_hip_model_delta(mb._h, ma._h, C.byref(query(lo=(3, 0, 0), hi=(2, 255, 255))), rp, vp, 16, cp) == L.OK
    assert result[0].tobytes() == zero.tobytes() and not counts.any() and voxels.tobytes() == untouched[1]
    assert lib.dust_hip_model_delta_apply(mb._h, None, 0, 0, C.byref(changed), C.byref(conflicts)) == L.OK and changed.value == conflicts.value == 0
    assert lib.dust_hip_model_delta_apply(mb._h, records.ctypes.data_as(C.c_void_p), 16, 1, None, None) == L.OK          # (backwards: `before` is index 0)
    want, _, _ = W.apply(full(before), records, backward=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(mb.read(), host_model(want, pal)))
    # unsupported exactly where set_voxels is, for either model, before the query is looked at
    changed.value = conflicts.value = 0x5A5A5A5A
    result[...], counts[...] = np.full(64, 0x5A, np.uint8).view(api.DELTA_RESULT_DTYPE), 0x5A5A5A5A
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(full(before), pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        assert status_of(lambda: unsupported.delta(ma)) == L.ERR_UNSUPPORTED and status_of(lambda: ma.delta(unsupported)) == L.ERR_UNSUPPORTED
        assert status_of(lambda: unsupported.delta_apply(records)) == L.ERR_UNSUPPORTED
        for q in (bad[0], bad[4], bad[6]):
            assert lib.dust_hip_model_delta(unsupported._h, ma._h, C.byref(q), rp, vp, 16, cp) == L.ERR_UNSUPPORTED
            assert lib.dust_hip_model_delta(ma._h, unsupported._h, C.byref(q), rp, vp, 16, cp) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_delta(unsupported._h, ma._h, None, rp, vp, 16, cp) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_delta_apply(unsupported._h, wrong_key.ctypes.data_as(C.c_void_p), 16, 2, C.byref(changed), C.byref(conflicts)) == L.ERR_UNSUPPORTED
    assert (result.tobytes(), voxels.tobytes(), counts.tobytes()) == untouched and changed.value == conflicts.value == 0x5A5A5A5A


def test_round_trip():
    before, after = random_pair()
    pal = synth.make_palette(66)
    ctx = api.Context(device=0)
    mb, ma = make(ctx, full(before), pal), make(ctx, full(after), pal)
    host_before, host_after = ([a.tobytes() for a in host_model(full(grid), pal)] for grid in (before, after))
    _, records, _ = mb.delta(ma)
    n = len(records)
    assert n > 500 and records.tobytes() == W.delta(before, after)[1].tobytes()
    origins, directions = ray_grid()
    points = [(13, 26, 14)]
    copy = make_editable(make(ctx, full(before), pal))
    copy.distance(max_radius=3)
    copy.flood([(100, 100, 100)], max_steps=90)
    scene = api.Scene(ctx)
    scene.add_instance(copy, ROTATED.reshape(12))
    scene.commit()
    scene.trace_rays(origins, directions)
    assert copy.delta_apply(records) == (n, 0)                                     # forward: before -> after
    assert [a.tobytes() for a in copy.read()] == host_after
    # an apply is an edit: the labelling and both fields are gone, and the scene needs a commit
    assert status_of(lambda: copy.island_of(points)) == L.ERR_NOT_READY and status_of(lambda: copy.distance_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: copy.flood_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY
    scene.commit()
    assert len(scene.trace_rays(origins, directions)) == len(origins)
    assert int(copy.delta(ma, capacity=0)[0]["voxels"]) == 0 and int(mb.delta(copy, capacity=0)[0]["voxels"]) == n
    assert copy.delta_apply(records) == (0, n)                                     # forward again on `after`: nothing moves, nothing was as expected
    assert [a.tobytes() for a in copy.read()] == host_after
    assert copy.delta_apply(records, backward=True) == (n, 0)                      # backwards: after -> before
    assert [a.tobytes() for a in copy.read()] == host_before
    fresh = make(ctx, full(before), pal)                                           # a model that is not editable becomes so
    assert fresh.delta_apply(records[: n // 2]) == (n // 2, 0)
    half, changed, conflicts = W.apply(full(before), records[: n // 2])
    assert (changed, conflicts) == (n // 2, 0) and all(x.tobytes() == y.tobytes() for x, y in zip(fresh.read(), host_model(half, pal)))
    # a key named twice keeps its last record; its conflict is judged on the model as it stood when the call began
    twice = np.concatenate([records[:40], records[:20], records[10:30]])
    twice["after"][40:60] = (twice["after"][40:60].astype(np.int64) + 1) % 200     # the second naming of records 0..19 wants something else
    twice["before"][60:] = 250                                                     # the third naming of records 10..19 expects what is not there
    target = make(ctx, full(before), pal)
    want, want_changed, want_conflicts = W.apply(full(before), twice)
    assert want_conflicts == 20 and len(W.survivors(twice)) == 40
    assert target.delta_apply(twice) == (want_changed, want_conflicts)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(target.read(), host_model(want, pal)))


def test_against_edit_shapes_and_census():
    before, _ = random_pair()
    pal = synth.make_palette(67)
    ctx = api.Context(device=0)
    original, copy = make(ctx, full(before), pal), make(ctx, full(before), pal)
    sphere = SW.shapes(SW.shape(SW.SPHERE, (20.5, 32.0, 17.0), radius=6.0, op=SW.CARVE))
    asked, asked_counts = original.census(sphere)
    changed = copy.edit_shapes(sphere)
    carved = full(before)
    assert SW.apply_to_grid(carved, sphere).tolist() == changed.tolist() and int(changed[0]) > 300
    result, voxels, counts = check(original, copy, full(before), carved)
    assert int(result["removed"]) == int(result["voxels"]) == int(changed[0]) == int(asked[0]["solid"])
    assert int(result["added"]) == int(result["repainted"]) == 0
    assert counts[0, 1:].tolist() == asked_counts[0, 1:].tolist() and int(counts[0, 0]) == 0      # the census's counters, less its None bin
    assert int(counts[1, 0]) == int(changed[0]) and not counts[1, 1:].any()
    assert result["lo"].tolist() == asked[0]["lo"].tolist() and result["hi"].tolist() == asked[0]["hi"].tolist()
    assert np.all(voxels["kind"] == L.DELTA_REMOVED) and np.all(voxels["after"] == L.DELTA_NONE)


def test_determinism():
    before, after = random_pair()
    pal = synth.make_palette(68)
    ctx = api.Context(device=0)
    mb, ma = make(ctx, full(before), pal), make(ctx, full(after), pal)
    first = mb.delta(ma, tables=True)
    second = mb.delta(ma, tables=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)) and int(first[0]["voxels"]) > 500
    one, two = make(ctx, full(before), pal), make(ctx, full(before), pal)
    assert one.delta_apply(first[1]) == two.delta_apply(first[1]) and all(x.tobytes() == y.tobytes() for x, y in zip(one.read(), two.read()))
