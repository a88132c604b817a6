"""Model settling on the device (dust_hip_model_settle, dust_hip_model_settle_apply; the contract is in include/dust_hip.h). Every
comparison is exact: the result, the applied record and its per-generation rows must be what the witness says
(tests/settle_witness.py), an apply must leave the model a host build of the witness's grid, and a read-only call must leave the model
as it found it. The grids are built in the walk's own coordinates -- [v][u][position from the toward end] -- so that each of the six
sides sees the same edges."""
import ctypes as C

import numpy as np
import pytest

import settle_witness as W
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
HIERARCHY = ("root", "host_root", "mid", "dense_mask", "bmin", "bmax")
WHOLE = ((0, 0, 0), (255, 255, 255))
SAND, GRAVEL, SNOW, ROCK, STEEL = 3, 4, 9, 1, 40                                     # grid bytes: three loose materials, two fixed ones
LOOSE = W.loose_mask([SAND - 1, GRAVEL - 1, SNOW - 1])


def host_model(grid, pal):
    return api.flatten_model(to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


def same_model(model, ctx, grid, pal):
    """the model is, byte for byte, a host build of `grid`"""
    fresh = make(ctx, grid, pal)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), fresh.read()))
    got, want = model.read_hierarchy(), fresh.read_hierarchy()
    assert got["n_mid"] == want["n_mid"] and got["extent_log2"] == want["extent_log2"]
    for name in HIERARCHY:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name


def walk_view(grid, toward):
    """the whole grid as [v][u][position from the toward end]: writing the view writes the grid"""
    return W.turned(grid, (slice(None),) * 3, toward)


def region_of(toward, v, u, positions):
    """the region (lo, hi) that holds v, u and positions (inclusive pairs in the walk's coordinates) for a side"""
    axis, high = W.side(toward)
    lo, hi = [0, 0, 0], [0, 0, 0]
    lo[W.V_AXIS[axis]], hi[W.V_AXIS[axis]] = v
    lo[W.U_AXIS[axis]], hi[W.U_AXIS[axis]] = u
    lo[axis], hi[axis] = (255 - positions[1], 255 - positions[0]) if high else positions
    return tuple(lo), tuple(hi)


def check(model, grid, toward, loose, region=WHOLE):
    """one read-only query on the device and in the witness: the records agree byte for byte; returns it"""
    result = model.settle(toward, loose, *region)
    want = W.settle(grid, toward, loose, region)
    assert result.dtype == api.SETTLE_RESULT_DTYPE and result.tobytes() == want.tobytes(), (toward, region, result, want)
    return result


def check_apply(ctx, model, grid, pal, toward, loose, generations=0, region=WHOLE, rest_within=None):
    """one apply on the device and in the witness: the record, the rows and the model agree; returns the witness's answer"""
    applied, table = model.settle_apply(toward, loose, *region, generations=generations, per_generation=True)
    after, want, want_table = W.apply(grid, toward, loose, generations, region, rest_within=rest_within)
    assert applied.dtype == api.SETTLE_APPLIED_DTYPE and table.shape == (generations, 2) and table.dtype == np.uint32
    assert np.array_equal(table, want_table), (table[:16], want_table[:16])
    assert applied.tobytes() == want.tobytes(), (applied, want)
    same_model(model, ctx, after, pal)
    return after, want, want_table


def hand_built(toward):
    grid = np.zeros((256,) * 3, np.uint8)
    t = walk_view(grid, toward)
    # loose runs over fixed supports across the brick edge 3 | 4 and the root-cell edges 15 | 16 and 63 | 64, hanging and resting
    t[5, 6, 1], t[5, 6, 3:6] = ROCK, SAND
    t[5, 6, 9], t[5, 6, 14:19] = STEEL, GRAVEL
    t[5, 6, 40], t[5, 6, 41:44], t[5, 6, 60:68] = ROCK, SNOW, SAND
    # ... and across the column-word edges 63 | 64, 127 | 128 and 191 | 192
    t[17, 62, 50], t[17, 62, 62:67] = ROCK, SAND
    t[17, 62, 100], t[17, 62, 125:131] = ROCK, GRAVEL
    t[17, 62, 150], t[17, 62, 189:195] = STEEL, SNOW
    t[17, 62, 250:256] = SAND                                                        # the far end of the column comes down to 195
    t[64, 15, :] = SAND                                                              # a full column: nothing can move
    t[64, 16, :] = np.where(np.arange(256) % 2 == 0, ROCK, GRAVEL)                   # full, alternating fixed and loose: nothing can move
    t[63, 16, 1::2] = SNOW                                                           # alternating loose and empty: 128 voxels close up
    t[63, 15, 0::2] = np.where(np.arange(128) % 3 == 0, STEEL, SAND)                 # ... with a fixed voxel in every third place
    # three loose materials interleaved with two fixed ones: order and indices must survive
    pattern = [SAND, 0, GRAVEL, SNOW, 0, 0, ROCK, 0, SNOW, SAND, 0, GRAVEL, STEEL, STEEL, 0, 0, 0, GRAVEL, SAND, SNOW, SNOW, 0, SAND]
    t[200, 130, 2:2 + 9 * len(pattern)] = np.tile(np.array(pattern, np.uint8), 9)
    t[0, 0, 255], t[255, 255, 0], t[255, 0, 200], t[0, 255, 255] = SAND, GRAVEL, SNOW, SAND   # single voxels in the corners of the tree
    # a support at 99 with a run hanging over it: the region below cuts the run in the middle and ends one voxel short of the support
    t[100, 100, 99], t[100, 100, 110:131] = ROCK, SAND
    t[100, 101, 99], t[100, 101, 105:112] = ROCK, GRAVEL
    return grid


@pytest.mark.parametrize("toward", W.FACES)
def test_hand_built_columns(toward):
    grid = hand_built(toward)
    pal = synth.make_palette(81)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    result = check(model, grid, toward, LOOSE)
    assert int(result["fixed"]) > 100 and int(result["moved"]) > 300 and int(result["fall_max"]) >= 55
    cut = region_of(toward, (98, 102), (99, 103), (100, 120))
    inside = check(model, grid, toward, LOOSE, cut)
    assert int(inside["loose"]) == 11 + 7 and int(inside["fixed"]) == 0 and int(inside["fall_max"]) == 10 and int(inside["moved"]) == 18
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))       # asking changed nothing
    # the cut region first: its floor is position 100, the support at 99 and the rest of the run above 120 do not exist for the call
    after, want, _ = check_apply(ctx, model, grid, pal, toward, LOOSE, 0, cut)
    t = walk_view(after, toward)
    assert t[100, 100, 99:135].tolist() == [ROCK] + [SAND] * 11 + [0] * 10 + [SAND] * 10 + [0] * 4
    assert int(want["first_moved"]) == 18 and int(want["generations"]) == 0 and int(want["fall_sum"]) == int(inside["fall_sum"])
    # then the whole tree
    asked = check(model, after, toward, LOOSE)
    done, want, _ = check_apply(ctx, model, after, pal, toward, LOOSE, 0)
    assert int(want["first_moved"]) == int(asked["moved"]) and int(want["fall_sum"]) == int(asked["fall_sum"]) and int(want["loose"]) == int(asked["loose"])
    assert want["lo"].tolist() == asked["lo"].tolist() and want["hi"].tolist() == asked["hi"].tolist()
    t = walk_view(done, toward)
    assert t[5, 6, :20].tolist() == [0, ROCK] + [SAND] * 3 + [0] * 4 + [STEEL] + [GRAVEL] * 5 + [0] * 5
    assert t[17, 62, 150:163].tolist() == [STEEL] + [SNOW] * 6 + [SAND] * 6 and not t[17, 62, 163:].any()
    assert t[63, 16, :129].tolist() == [SNOW] * 128 + [0] and np.array_equal(t[64, 16], walk_view(grid, toward)[64, 16])
    column = t[200, 130]
    assert column[column != 0].tolist() == [b for b in np.tile(np.array([SAND, GRAVEL, SNOW, ROCK, SNOW, SAND, GRAVEL, STEEL, STEEL, GRAVEL, SAND, SNOW, SNOW, SAND]), 9)]
    assert t[0, 0, 0] == SAND and t[255, 255, 0] == GRAVEL and t[255, 0, 0] == SNOW and t[0, 255, 0] == SAND
    assert int(check(model, done, toward, LOOSE)["moved"]) == 0                      # a fall leaves nothing to fall


def test_read_only_on_a_model_that_is_not_editable():
    grid = hand_built(W.NEG_Y)
    pal = synth.make_palette(82)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    n = 8
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    directions = np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))
    hits = scene.trace_rays(origins, directions)
    source = [a.tobytes() for a in model.read()]
    first = [check(model, grid, toward, loose).tobytes() for toward in (W.NEG_Y, W.POS_X) for loose in (LOOSE, W.ALL_LOOSE, W.loose_mask([]))]
    second = [check(model, grid, toward, loose).tobytes() for toward in (W.NEG_Y, W.POS_X) for loose in (LOOSE, W.ALL_LOOSE, W.loose_mask([]))]
    assert first == second                                                           # two runs, the same bytes
    assert [a.tobytes() for a in model.read()] == source
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()         # no commit: the generation has not moved
    model.find_islands(L.ISLANDS_FACES, capacity=0)                                  # the first-edit transition happens HERE, not in settle
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY
    assert [check(model, grid, toward, loose).tobytes() for toward in (W.NEG_Y, W.POS_X) for loose in (LOOSE, W.ALL_LOOSE, W.loose_mask([]))] == first


@pytest.mark.parametrize("toward", [W.NEG_Y, W.POS_Z])
def test_all_ones_beside_a_mask_of_every_present_index(toward):
    rng = np.random.default_rng(83)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[50:82, 100:140, 110:150] = np.where(rng.random((32, 40, 40)) < 0.3, rng.choice([SAND, GRAVEL, SNOW, ROCK, STEEL, 255], (32, 40, 40)), 0)
    named = W.loose_mask([SAND - 1, GRAVEL - 1, SNOW - 1, ROCK - 1, STEEL - 1, 254])
    pal = synth.make_palette(83)
    ctx = api.Context(device=0)
    one, two = make(ctx, grid, pal), make(ctx, grid, pal)
    region = ((40, 90, 100), (90, 150, 160))
    for r in (WHOLE, region):
        assert check(one, grid, toward, W.ALL_LOOSE, r).tobytes() == check(two, grid, toward, named, r).tobytes()
    a, rows_a = one.settle_apply(toward, None, *region, generations=6, per_generation=True)
    b, rows_b = two.settle_apply(toward, named, *region, generations=6, per_generation=True)
    assert a.tobytes() == b.tobytes() and rows_a.tobytes() == rows_b.tobytes() and int(a["slid"]) > 100
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one.read(), two.read()))
    same_model(one, ctx, W.apply(grid, toward, W.ALL_LOOSE, 6, region)[0], pal)


def piles(toward):
    """the three inputs whose outcome the witness's tests pin, on a fixed floor at position 3, placed so that the piles cross 15 | 16 and
    63 | 64 in u and in v; a tower beside the region's lateral face; a tower under a fixed roof. Returns (grid, region)."""
    grid = np.zeros((256,) * 3, np.uint8)
    t = walk_view(grid, toward)
    t[0:96, 0:96, 3] = ROCK
    t[15, 64, 4:16] = SAND                                                           # the tower of 12: v across 15 | 16, u across 63 | 64
    t[62:66, 14:18, 4:12] = GRAVEL                                                   # the 4 x 8 x 4 block: v across 63 | 64, u across 15 | 16
    rng = np.random.default_rng(84)
    t[58:70, 58:70, 4:23] = np.where(rng.random((12, 12, 19)) < 0.3, rng.choice([SAND, SNOW], (12, 12, 19)), 0)   # the 30 % fill of 12 x 19 x 12
    t[40, 95, 4:12] = SNOW                                                           # beside the face u = 95 of the region: no slide across it
    t[40, 96, 3] = ROCK                                                              # (there is a floor beyond the face: only the region stops it)
    t[30, 30, 4:9], t[30, 30, 9] = SAND, STEEL                                       # under a roof: the top voxel has something above it
    t[90:96, 5, 30] = SAND                                                           # a bar in the air, ending at the face v = 95
    return grid, region_of(toward, (0, 95), (0, 95), (0, 63))


@pytest.mark.parametrize("toward", W.FACES)
def test_slides(toward):
    grid, region = piles(toward)
    pal = synth.make_palette(84)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    everything = api.edit_shapes(L.SHAPE_BOX, [0, 0, 0], [256, 256, 256])
    _, census = model.census(everything)
    after, want, rows = check_apply(ctx, model, grid, pal, toward, LOOSE, 256, region, rest_within=64)
    generations = int(want["generations"])
    assert 30 <= generations <= 64 and int(want["slid"]) > 300 and int(want["fell"]) > 100 and not rows[generations:].any()
    assert W.height_sum(grid, toward, LOOSE, W.clip(grid, region)) - W.height_sum(after, toward, LOOSE, W.clip(after, region)) == int(want["fall_sum"]) + int(want["slid"])
    t = walk_view(after, toward)
    assert t[40, 95, 4] == SNOW and not t[:, 96:, 4:].any() and not t[96:, :, 4:].any()    # nothing left the region: its faces stopped the slides
    assert t[30, 30, 8] == SAND and t[30, 30, 9] == STEEL                            # the voxel under the roof stayed; those below it had neighbours above
    assert np.array_equal(model.census(everything)[1], census)                       # every material's count
    # the early stop does not show: exactly the generations that moved something give the same bytes and the same record
    twin = make(ctx, grid, pal)
    applied, table = twin.settle_apply(toward, LOOSE, *region, generations=generations, per_generation=True)
    assert applied.tobytes() == want.tobytes() and np.array_equal(table, rows[:generations])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), twin.read()))
    # a second apply moves nothing
    again, none = model.settle_apply(toward, LOOSE, *region, generations=256, per_generation=True)
    assert int(again["generations"]) == 0 and int(again["first_moved"]) == 0 and int(again["slid"]) == 0 == int(again["fell"]) and not none.any()
    assert again["lo"].tolist() == [255] * 3 and again["hi"].tolist() == [0] * 3 and int(again["loose"]) == int(want["loose"])
    same_model(model, ctx, after, pal)


@pytest.mark.parametrize("toward", W.FACES)
def test_bounds_of_lone_slides(toward):
    """four lone voxels on fixed pillars, walled so that voxel k can only slide in the direction of generation k, each across a brick
    edge in the plane and along the fall: the brick a voxel leaves sees no arrival, the brick it enters no departure, and the fall
    behind the slide happens in the destination's column only -- the source's coordinates reach the bounds through the slide alone"""
    grid = np.zeros((256,) * 3, np.uint8)
    t = walk_view(grid, toward)
    steps = ((0, 1), (0, -1), (1, 0), (-1, 0))                                       # (dv, du) of +u, -u, +v, -v
    for k, (v, u) in enumerate(((18, 35), (38, 36), (59, 60), (80, 70))):
        t[v, u, 0:12], t[v, u, 12] = ROCK, SAND
        for dv, du in steps[:k]:
            t[v + dv, u + du, 12] = STEEL
    region = region_of(toward, (0, 95), (0, 95), (0, 63))
    pal = synth.make_palette(88)
    ctx = api.Context(device=0)
    for generations in (1, 4):
        model = make(ctx, grid, pal)
        after, want, rows = check_apply(ctx, model, grid, pal, toward, LOOSE, generations, region)
        assert rows.tolist() == [[1, 1]] * generations and int(want["first_moved"]) == 0 and int(want["fall_sum"]) == 11 * generations
    t = walk_view(after, toward)
    assert [int(t[v, u, 0]) for v, u in ((18, 36), (38, 35), (60, 60), (79, 70))] == [SAND] * 4
    assert want["lo"].tolist() == list(region_of(toward, (18, 80), (35, 70), (0, 12))[0]) and want["hi"].tolist() == list(region_of(toward, (18, 80), (35, 70), (0, 12))[1])


@pytest.mark.parametrize("generations", [1, 2, 3, 5, 9])
def test_both_grids(generations):
    """an odd and an even number of slides, and one more than the library's look-ahead, all leave the result in the model's own grid"""
    grid, region = piles(W.NEG_Y)
    pal = synth.make_palette(85)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    _, want, rows = check_apply(ctx, model, grid, pal, W.NEG_Y, LOOSE, generations, region)
    assert int(want["generations"]) == generations and rows.any(axis=1).all()


def test_empty_region_and_empty_model():
    grid, _ = piles(W.NEG_Y)
    pal = synth.make_palette(86)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    empty = ((9, 9, 9), (8, 200, 200))
    assert check(model, grid, W.NEG_Y, LOOSE, empty).tobytes() == W.zero_result().tobytes()
    q = model._settle_query(W.NEG_Y, LOOSE, *empty)
    result = np.full(64, 0x5A, np.uint8).view(api.SETTLE_RESULT_DTYPE)
    applied = np.full(64, 0x5A, np.uint8).view(api.SETTLE_APPLIED_DTYPE)
    rows = np.full(512, 0x5A5A5A5A, np.uint32)
    rp, ap, gp = (a.ctypes.data_as(C.c_void_p) for a in (result, applied, rows))
    assert lib.dust_hip_model_settle(model._h, C.byref(q), rp) == L.OK and result[0].tobytes() == W.zero_result().tobytes()
    assert lib.dust_hip_model_settle(model._h, C.byref(q), None) == L.OK             # every output may be null
    assert lib.dust_hip_model_settle_apply(model._h, C.byref(q), 256, ap, gp) == L.OK
    assert applied[0].tobytes() == W.zero_applied().tobytes() and not rows.any()
    assert lib.dust_hip_model_settle_apply(model._h, C.byref(q), 0, None, None) == L.OK
    same_model(model, ctx, grid, pal)
    # a region that holds nothing, and a model that holds nothing
    bare = ((200, 200, 200), (255, 255, 255))
    assert int(check(model, grid, W.POS_X, W.ALL_LOOSE, bare)["columns"]) == 56 * 56
    check_apply(ctx, model, grid, pal, W.POS_X, W.ALL_LOOSE, 4, bare)
    nothing = np.zeros((256,) * 3, np.uint8)
    void = make(ctx, nothing, pal)
    for toward in (W.NEG_Y, W.POS_Z):
        assert int(check(void, nothing, toward, W.ALL_LOOSE)["columns"]) == 65536
        check(void, nothing, toward, LOOSE)
    check_apply(ctx, void, nothing, pal, W.NEG_Y, LOOSE, 8)


def test_state_and_refusals():
    grid, region = piles(W.NEG_Y)
    pal = synth.make_palette(87)
    ctx = api.Context(device=0)
    lib = L.load()
    points = [(13, 3, 14), (20, 3, 16), (200, 200, 200)]
    model = make(ctx, grid, pal)
    model.find_islands(L.ISLANDS_FACES, capacity=0)
    model.distance(max_radius=3)
    model.flood([(100, 100, 100)], max_steps=90)
    keys, values, steps = model.island_of(points), model.distance_at(points), model.flood_at(points)
    # a read-only call leaves the labelling and both fields valid
    check(model, grid, W.NEG_Y, LOOSE, region)
    assert model.island_of(points).tolist() == keys.tolist() and model.distance_at(points).tolist() == values.tolist()
    assert model.flood_at(points).tolist() == steps.tolist()
    # every refusal, the outputs untouched and the model as it was
    result = np.full(64, 0x5A, np.uint8).view(api.SETTLE_RESULT_DTYPE)
    applied = np.full(64, 0x5A, np.uint8).view(api.SETTLE_APPLIED_DTYPE)
    rows = np.full(512, 0x5A5A5A5A, np.uint32)
    rp, ap, gp = (a.ctypes.data_as(C.c_void_p) for a in (result, applied, rows))

    def query(toward=4, flags=0, reserved=0, lo=(0, 0, 0), hi=(255, 255, 255), loose=LOOSE, size=C.sizeof(L.SettleQuery)):
        q = L.SettleQuery(struct_size=size, toward=toward, flags=flags, reserved=reserved)
        q.lo[:], q.hi[:], q.loose[:] = lo, hi, loose
        return q
    bad = [query(toward=0), query(toward=3), query(toward=64), query(toward=63), query(flags=1), query(flags=1 << 31), query(reserved=1), query(lo=(0, 256, 0)),
           query(hi=(255, 255, 256)), query(loose=(0,) * 7 + (1 << 31,)), query(loose=(0xFFFFFFFF,) * 8), query(size=71), query(size=0)]
    for q in bad:
        assert lib.dust_hip_model_settle(model._h, C.byref(q), rp) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_settle_apply(model._h, C.byref(q), 1, ap, gp) == L.ERR_INVALID_ARGUMENT
    for q in bad[:-2]:                                                               # ... and each of those is one the witness refuses too
        assert W.refused(q.toward, q.flags, q.reserved, tuple(q.lo), tuple(q.hi), tuple(q.loose))
    good = query()
    assert lib.dust_hip_model_settle(model._h, None, rp) == L.ERR_INVALID_ARGUMENT and lib.dust_hip_model_settle(None, C.byref(good), rp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_settle_apply(model._h, None, 1, ap, gp) == L.ERR_INVALID_ARGUMENT
    for generations in (257, 0xFFFFFFFF):
        assert lib.dust_hip_model_settle_apply(model._h, C.byref(good), generations, ap, gp) == L.ERR_INVALID_ARGUMENT
    assert result.tobytes() == b"\x5a" * 64 and applied.tobytes() == b"\x5a" * 64 and np.all(rows == 0x5A5A5A5A)
    assert model.island_of(points).tolist() == keys.tolist()                         # no refused apply touched the model or its labelling
    assert lib.dust_hip_model_settle(model._h, C.byref(query(size=80)), None) == L.OK    # a larger struct_size is a newer caller's
    # an apply is an edit, even one that moves nothing: the labelling and both fields are gone, and the scene needs a commit
    scene = api.Scene(ctx)
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    origins, directions = np.float32([[300.0, -30.0, 60.0]]), np.float32([[-1.0, 0.01, 0.02]])
    scene.trace_rays(origins, directions)
    still = model.settle_apply(W.NEG_Y, LOOSE, (200, 200, 200), (255, 255, 255))
    assert int(still["first_moved"]) == 0 and int(still["loose"]) == 0
    assert status_of(lambda: model.island_of(points)) == L.ERR_NOT_READY and status_of(lambda: model.distance_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: model.flood_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY
    scene.commit()
    assert len(scene.trace_rays(origins, directions)) == 1
    # unsupported exactly where set_voxels is, before the query is looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    assert status_of(lambda: deep.settle(W.NEG_Y)) == L.ERR_UNSUPPORTED and status_of(lambda: deep.settle_apply(W.NEG_Y)) == L.ERR_UNSUPPORTED
    assert lib.dust_hip_model_settle(deep._h, C.byref(bad[0]), rp) == L.ERR_UNSUPPORTED
