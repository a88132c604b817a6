"""Model floods on the device (dust_hip_model_flood / flood_at / flood_paths / flood_apply; the contract is in include/dust_hip.h). Every
comparison is exact: the field, the result record and the paths must be the witness's (tests/flood_witness.py: the header's definitions
in numpy), and a model a flood was applied to must read back byte for byte what a host build of the witness's voxels uploads.

The brick snake is not the Hamiltonian one of a first sketch: every voxel of a full 4^3 brick is within 9 steps of every other, and a
snake in which only consecutive voxels touch fits 22 voxels into a brick (flood_witness.brick_snake). The kernel's bound of 64 rounds
per brick is the safe side of that."""
import ctypes as C

import numpy as np
import pytest

import flood_witness as W
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
MEDIA = (L.FLOOD_EMPTY, L.FLOOD_SOLID, L.FLOOD_MATERIAL)


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


def box_coordinates(region):
    lo, hi = region
    return np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)


def field_matches(model, want, region):
    """the device field over a box, read with flood_at, against the witness's"""
    xyz = box_coordinates(region)
    return np.array_equal(model.flood_at(xyz), W.at(want, xyz))


def test_corridors_on_a_model_that_was_never_edited():
    grid, empty, solid = W.corridors()
    pal = synth.make_palette(21)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for runs, medium in ((empty, L.FLOOD_EMPTY), (solid, L.FLOOD_SOLID)):
        seeds = [r[0] for r in runs]
        r = model.flood(seeds, medium=medium)
        for run in runs:
            assert model.flood_at(run).tolist() == list(range(31)), medium
        assert model.flood_at(run + 1).tolist() == [L.FLOOD_UNREACHED] * 31         # beside the last corridor: the other medium
        want = W.steps(grid, seeds, medium)
        assert r.tobytes() == W.result(want).tobytes() and int(r["reached"]) == 93 and int(r["farthest"]) == 30
    assert same_bytes(model, grid, pal)      # the floods moved the model into its editable form and changed no voxel


def test_snake_inside_one_brick():
    grid, path = W.brick_snake()
    pal = synth.make_palette(22)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    r = model.flood([path[0]], medium=L.FLOOD_SOLID)
    assert model.flood_at(path).tolist() == list(range(22)) and int(r["farthest"]) == 21 and int(r["reached"]) == 22
    r = model.flood([path[0], path[-1]], medium=L.FLOOD_SOLID)
    assert model.flood_at(path).tolist() == [min(i, 21 - i) for i in range(22)] and int(r["farthest"]) == 10 and int(r["seeds_used"]) == 2
    r = model.flood([path[-1]], medium=L.FLOOD_MATERIAL, palette=8)      # from the other end, as a material
    assert model.flood_at(path).tolist() == list(range(21, -1, -1))
    assert int(model.flood([path[0]], medium=L.FLOOD_MATERIAL, palette=7)["reached"]) == 0


def test_late_shortcut_corrects_what_the_detour_wrote():
    grid, seed, target, detour, shortcut = W.late_shortcut()
    pal = synth.make_palette(23)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    want = W.steps(grid, [seed], W.SOLID)
    r = model.flood([seed], medium=L.FLOOD_SOLID)
    assert r.tobytes() == W.result(want).tobytes()
    assert model.flood_at(shortcut).tolist() == list(range(24))
    along = model.flood_at(detour)
    assert along.tolist() == W.at(want, detour).tolist() and along[-1] == 23 and along.max() == 31      # the far end of the detour is reached from the target
    assert field_matches(model, want, ((28, 28, 28), (52, 40, 40)))


@pytest.fixture(scope="module")
def random_case():
    """the random fill and the witness's field for each medium, computed once"""
    grid, region, seeds = W.random_fill()
    fields = {m: W.steps(grid, seeds[m], m, W.RANDOM_PALETTE, region=region) for m in MEDIA}
    return grid, region, seeds, fields


def test_random_fill_near_the_threshold(random_case):
    grid, region, seeds, fields = random_case
    r = W.result(fields[W.EMPTY], region)
    assert (int(r["reached"]), int(r["farthest"])) == (52376, 270)      # the input has not degenerated
    pal = synth.make_palette(24)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    xyz = box_coordinates(region)
    first = {}
    for again in range(2):
        for medium in MEDIA:
            got = model.flood(seeds[medium], medium=medium, palette=W.RANDOM_PALETTE, region=region)
            want = W.result(fields[medium], region)
            print(f"medium {medium}: reached {int(got['reached'])} farthest {int(got['farthest'])} boundary {int(got['boundary'])}")
            assert got.tobytes() == want.tobytes(), medium
            field = model.flood_at(xyz)
            assert np.array_equal(field, W.at(fields[medium], xyz)), medium
            assert first.setdefault(medium, field.tobytes()) == field.tobytes()
    outside = np.array(region[0]) - 1
    assert model.flood_at([outside, np.array(region[1]) + 1]).tolist() == [L.FLOOD_UNREACHED] * 2


def test_max_steps_and_region():
    grid, empty, _ = W.corridors()
    room, inside, room_region = W.room()
    grid = np.maximum(grid, room)
    pal = synth.make_palette(25)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    run = empty[0]
    r = model.flood([run[0]], max_steps=12)
    assert model.flood_at(run).tolist() == list(range(13)) + [L.FLOOD_UNREACHED] * 18 and (int(r["reached"]), int(r["farthest"])) == (13, 12)
    r = model.flood([run[0], empty[1][4]], max_steps=0)
    assert (int(r["reached"]), int(r["farthest"]), int(r["seeds_used"])) == (2, 0, 2) and model.flood_at(run[:2]).tolist() == [0, L.FLOOD_UNREACHED]
    cut = ((0, 0, 0), (25, 255, 255))             # the region ends in the middle of the corridor
    r = model.flood([run[0]], region=cut)
    assert model.flood_at(run).tolist() == list(range(16)) + [L.FLOOD_UNREACHED] * 15
    assert r.tobytes() == W.result(W.steps(grid, [run[0]], region=cut), cut).tobytes() and int(r["boundary"]) == 1
    r = model.flood([run[0]], region=((5, 0, 0), (4, 255, 255)))      # lo > hi: nothing is passable, and the field is valid
    assert r.tobytes() == bytes(32) and model.flood_at(run[:3]).tolist() == [L.FLOOD_UNREACHED] * 3
    r = model.flood([run[20]], region=((0, 0, 0), (4000, 1 << 31, 255)))      # clipped to the tree
    assert int(r["reached"]) == 31 and int(r["boundary"]) == 0
    # a sealed room, then a hole in its wall
    r = model.flood([inside], region=room_region)
    assert r.tobytes() == W.result(W.steps(grid, [inside], region=room_region), room_region).tobytes()
    assert int(r["boundary"]) == 0 and int(r["reached"]) == 16 ** 3
    wall = (room_region[1][0], inside[1], inside[2])
    changed = model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, np.array(wall) + 0.2, np.array(wall) + 0.8))
    assert changed.tolist() == [1]
    grid[wall] = 0
    assert status_of(lambda: model.flood_at([inside])) == L.ERR_NOT_READY
    r = model.flood([inside], region=room_region)
    assert r.tobytes() == W.result(W.steps(grid, [inside], region=room_region), room_region).tobytes()
    assert int(r["boundary"]) == 1 and int(r["reached"]) == 16 ** 3 + 1
    assert same_bytes(model, grid, pal)


def test_seeds_that_do_not_count():
    grid, empty, solid = W.corridors()
    pal = synth.make_palette(26)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    run = empty[0]
    region = ((0, 0, 0), (30, 255, 255))
    seeds = [run[3], run[3], (5, 5, 5), run[25], run[3], solid[0][0], (0, 255, 255), run[9]]      # duplicates; solid; outside the region; solid; far away
    r = model.flood(seeds, region=region)
    want = W.steps(grid, seeds, region=region)
    assert r.tobytes() == W.result(want, region).tobytes()
    assert int(r["seeds_used"]) == 3 and model.flood_at(run[:12]).tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert model.flood_at([(0, 255, 255), (30, 255, 255), (31, 255, 255), run[25]]).tolist() == [0, 30, L.FLOOD_UNREACHED, L.FLOOD_UNREACHED]
    r = model.flood([])
    assert r.tobytes() == bytes(32) and model.flood_at([run[3], (255, 255, 255)]).tolist() == [L.FLOOD_UNREACHED] * 2
    lengths, keys = model.flood_paths([run[3]], 2)
    assert lengths.tolist() == [0] and keys.tolist() == [[0, 0]]
    assert model.flood_apply(3) == 0 and same_bytes(model, grid, pal)
    many = np.tile(np.array(run[5], np.uint32), (L.MAX_FLOOD_SEEDS, 1))
    assert int(model.flood(many)["seeds_used"]) == 1 and int(model.flood_at([run[0]])[0]) == 5


def test_open_tree():
    """the many-pass case: an empty tree from one corner is the Manhattan distance"""
    pal = synth.make_palette(27)
    ctx = api.Context(device=0)
    model = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    r = model.flood([(0, 0, 0)])
    assert int(r["reached"]) == 1 << 24 and int(r["farthest"]) == 765 and int(r["seeds_used"]) == 1
    assert r["lo"].tolist() == [0, 0, 0] and r["hi"].tolist() == [255, 255, 255]
    assert int(r["boundary"]) == 256 ** 3 - 254 ** 3
    xyz = np.random.default_rng(28).integers(0, 256, (4000, 3))
    xyz[:4] = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (3, 4, 0)]
    assert np.array_equal(model.flood_at(xyz), xyz.sum(axis=1).astype(np.uint16))
    lengths, keys = model.flood_paths([(255, 255, 255), (2, 1, 1)], 5)
    assert lengths.tolist() == [766, 5]
    assert keys.tolist() == [[key(255 - i, 255, 255) for i in range(5)], [key(2, 1, 1), key(1, 1, 1), key(0, 1, 1), key(0, 0, 1), 0]]
    r = model.flood([(255, 255, 255), (0, 0, 0)], max_steps=100)
    assert int(r["farthest"]) == 100 and int(r["reached"]) == 2 * sum((k + 1) * (k + 2) // 2 for k in range(101))


def test_paths_follow_the_witness(random_case):
    grid, region, seeds, fields = random_case
    pal = synth.make_palette(24)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    model.flood(seeds[W.EMPTY], region=region)
    want = fields[W.EMPTY]
    rng = np.random.default_rng(29)
    o = np.array(W.RANDOM_ORIGIN)
    reached = np.argwhere(want != W.UNREACHED)
    far = reached[np.argsort(want[tuple(reached.T)], kind="stable")[-40:]]
    starts = np.concatenate([reached[rng.integers(0, len(reached), 150)], far, seeds[W.EMPTY], rng.integers(0, 64, (100, 3)) + o, rng.integers(0, 256, (10, 3))])
    for capacity in (2, 16, 300):
        sentinel = np.full((len(starts), capacity), 0xA5A5A5A5, np.uint32)
        want_lengths, want_keys = W.paths(want, starts, capacity, sentinel)
        lengths, keys = model.flood_paths(starts, capacity, keys=sentinel.copy())
        assert np.array_equal(lengths, want_lengths) and np.array_equal(keys, want_keys), capacity
        assert lengths.max() == 271 and np.count_nonzero(lengths == 0) > 30 and np.count_nonzero(lengths == 1) >= 3
        assert np.count_nonzero(keys == 0xA5A5A5A5) > 0
    lengths, keys = model.flood_paths(starts, 0)
    assert np.array_equal(lengths, want_lengths) and keys.shape == (len(starts), 0)
    # ties: a voxel with more than one neighbour one step closer takes the first in the order -x, +x, -y, +y, -z, +z
    tied = 0
    for s, k in zip(starts, want_keys):
        d = int(want[tuple(s)])
        if d in (0, W.UNREACHED):
            continue
        closer = [tuple(s + n) for n in W.NEIGHBOURS if want[tuple(np.clip(s + n, 0, 255))] == d - 1]
        tied += len(closer) > 1
        assert key(*closer[0]) == k[1]
    assert tied > 20


def ray_grid(n=48):
    """n * n rays down onto the crater's ground"""
    u, v = np.meshgrid(np.linspace(2.3, 77.7, n, dtype=np.float32), np.linspace(2.6, 77.4, n, dtype=np.float32))
    origins = np.stack([u.reshape(-1), np.full(n * n, 120.0, np.float32), v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([0.05, -1.0, 0.03]), (n * n, 1))


def test_apply_water_paint_and_vein():
    grid, pour, below = W.crater()
    pal = synth.make_palette(30)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    origins, directions = ray_grid()
    cases = (("water", dict(seeds=[pour], medium=L.FLOOD_EMPTY, region=below), 7, None),
             ("paint", dict(seeds=[(13, 39, 13)], medium=L.FLOOD_MATERIAL, palette=5), 8, None),
             ("vein", dict(seeds=[(59, 20, 50)], medium=L.FLOOD_MATERIAL, palette=9), -1, None),
             ("blast", dict(seeds=[(40, 39, 20), (41, 39, 20)], medium=L.FLOOD_SOLID, max_steps=9), -1, 6))
    for name, flood, value, limit in cases:
        scene = api.Scene(ctx)
        scene.add_instance(model, IDENTITY.reshape(12))
        if name != "water":          # (the first flood moves the model into its editable form: a scene committed before it is stale already)
            scene.commit()
        model.find_islands(L.ISLANDS_FACES)
        r = model.flood(**flood)
        field = W.steps(grid, flood["seeds"], flood["medium"], flood.get("palette", 0), flood.get("max_steps", W.MAX_STEPS), flood.get("region"))
        assert r.tobytes() == W.result(field, flood.get("region")).tobytes() and int(r["reached"]) > 20, name
        if name != "water":
            assert len(scene.trace_rays(origins, directions)) == len(origins)       # a flood of an editable model changes nothing a scene reads
        else:
            assert int(r["boundary"]) > 0 and int(r["hi"][1]) == 35                 # the water stands at the region's top face
        grid, want_changed = W.apply(grid, field, value, limit)
        changed = model.flood_apply(value, limit)
        print(f"{name}: reached {int(r['reached'])} changed {changed}")
        assert changed == want_changed > 0 and (limit is None or changed < int(r["reached"])), name
        assert same_bytes(model, grid, pal), name
        assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY
        scene.commit()
        got = scene.trace_rays(origins, directions)
        other = api.Scene(ctx)
        other.add_instance(make(ctx, grid, pal), IDENTITY.reshape(12))
        other.commit()
        assert got.tobytes() == other.trace_rays(origins, directions).tobytes(), name
        assert np.count_nonzero(got["instance"] != L.NO_HIT) > 1000
        assert status_of(lambda: model.flood_at([pour])) == L.ERR_NOT_READY
        assert status_of(lambda: model.island_of([pour])) == L.ERR_NOT_READY
    assert np.count_nonzero(grid == 9) == 56 and np.count_nonzero(grid == 6) == 0 and np.count_nonzero(grid == 10) == 0      # the whole patch, the whole vein


def test_validity_matrix():
    grid, empty, solid = W.corridors()
    pal = synth.make_palette(31)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    other = make(ctx, W.brick_snake()[0], pal)
    run = empty[0]
    xp = np.ascontiguousarray(run[:1], np.uint32)
    out16, out32 = np.zeros(1, np.uint16), np.zeros(1, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def standing():
        return lib.dust_hip_model_flood_at(model._h, None, None, 0) == L.OK

    # nothing stands before the first flood, with n == 0 as well
    assert lib.dust_hip_model_flood_at(model._h, None, None, 0) == L.ERR_NOT_READY
    assert lib.dust_hip_model_flood_at(model._h, ptr(xp), ptr(out16), 1) == L.ERR_NOT_READY
    assert lib.dust_hip_model_flood_paths(model._h, None, 0, 0, None, ptr(out32)) == L.ERR_NOT_READY
    assert lib.dust_hip_model_flood_paths(model._h, ptr(xp), 1, 1, ptr(out32), ptr(out32)) == L.ERR_NOT_READY
    assert lib.dust_hip_model_flood_apply(model._h, 5, 1, None) == L.ERR_NOT_READY
    assert same_bytes(model, grid, pal)

    def flood():
        assert int(model.flood([run[0]])["reached"]) == 31 and standing()

    flood()
    assert lib.dust_hip_model_flood_paths(model._h, None, 0, 0, None, ptr(out32)) == L.OK
    # what leaves the field standing
    n, rec = model.find_islands(L.ISLANDS_FACES)
    assert standing() and model.island_of([solid[0][0]]).tolist() == [key(*solid[0][0])]
    piece = model.detach_islands([key(*solid[0][0])], keep_source=True)
    assert standing() and piece is not None
    other.stamp(model, api.stamps([(0, 0, 0)]))          # being a stamp's source
    assert standing()
    flood()                                               # a flood leaves the island labelling
    assert model.island_of([solid[0][0]]).tolist() == [key(*solid[0][0])]
    assert model.detach_islands([]) is None and standing()          # n == 0
    model.set_voxels(np.zeros((0, 3), np.uint32), np.zeros(0, np.int32))
    model.edit_shapes(np.zeros(0, api.EDIT_SHAPE_DTYPE))
    model.stamp(other, np.zeros(0, api.STAMP_DTYPE))
    assert standing()
    assert model.flood_at(run[-1:]).tolist() == [30]
    # what invalidates it, whether or not a voxel changes
    model.set_voxels([(200, 200, 200)], [-1])
    assert not standing()
    flood()
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]))        # a shape that covers nothing
    assert not standing()
    flood()
    model.stamp(other, api.stamps([(300, 0, 0)]))        # an image outside the tree
    assert not standing()
    flood()
    model.find_islands(L.ISLANDS_FACES)
    model.detach_islands([key(*solid[1][0])], want_model=False)                                # a carving detach
    assert not standing() and model.island_of([solid[0][0]]).tolist() == [key(*solid[0][0])]  # (the labelling of the rest stands)
    flood()
    assert model.flood_apply(2, max_steps=0) == 1
    assert not standing() and status_of(lambda: model.island_of([solid[0][0]])) == L.ERR_NOT_READY
    r = model.flood([run[0], run[1]])                    # the first seed's voxel is solid now: ignored
    assert (int(r["reached"]), int(r["seeds_used"])) == (30, 1) and model.flood_at(run[:2]).tolist() == [L.FLOOD_UNREACHED, 0]


def test_refusals_and_their_order():
    grid, empty, _ = W.corridors()
    pal = synth.make_palette(32)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    run = empty[0]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = np.ascontiguousarray(run[:2], np.uint32)
    bad = good.copy()
    bad[1, 1] = 256

    def query(**kw):
        q = L.FloodQuery(struct_size=C.sizeof(L.FloodQuery), medium=L.FLOOD_EMPTY, max_steps=L.FLOOD_MAX_STEPS)
        q.hi[:] = [255, 255, 255]
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    out = np.full(1, 0x5A, np.uint8).repeat(32).view(api.FLOOD_RESULT_DTYPE)
    before = out.tobytes()
    fn = lib.dust_hip_model_flood
    refused = [(None, good, 2), (query(struct_size=39), good, 2), (query(struct_size=0), good, 2), (query(medium=3), good, 2),
               (query(medium=L.FLOOD_MATERIAL, palette=255), good, 2), (query(medium=L.FLOOD_MATERIAL, palette=-1), good, 2),
               (query(max_steps=65535), good, 2), (query(), None, 2), (query(), good, L.MAX_FLOOD_SEEDS + 1), (query(), bad, 2)]
    for stage in range(2):          # before any flood, and with a field standing: a refusal changes nothing
        for q, seeds, n in refused:
            assert fn(model._h, None if q is None else C.byref(q), None if seeds is None else ptr(seeds), n, ptr(out)) == L.ERR_INVALID_ARGUMENT
        assert out.tobytes() == before
        if stage == 0:
            assert lib.dust_hip_model_flood_at(model._h, None, None, 0) == L.ERR_NOT_READY
            assert same_bytes(model, grid, pal)
            # a coordinate is looked at before the field is
            steps = np.full(2, 77, np.uint16)
            assert lib.dust_hip_model_flood_at(model._h, ptr(bad), ptr(steps), 2) == L.ERR_INVALID_ARGUMENT
            assert lib.dust_hip_model_flood_at(model._h, ptr(good), ptr(steps), 2) == L.ERR_NOT_READY
            assert lib.dust_hip_model_flood_apply(model._h, 0, 255, None) == L.ERR_INVALID_ARGUMENT
            assert lib.dust_hip_model_flood_apply(model._h, 0, 254, None) == L.ERR_NOT_READY
            assert fn(model._h, C.byref(query(palette=255, struct_size=64)), ptr(good), 2, None) == L.OK      # palette is read under MATERIAL only; out may be NULL
        else:
            assert model.flood_at(good).tolist() == [0, 0]
    steps = np.full(2, 77, np.uint16)
    keys, lengths = np.full((2, 3), 77, np.uint32), np.full(2, 77, np.uint32)
    assert lib.dust_hip_model_flood_at(model._h, ptr(bad), ptr(steps), 2) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_flood_at(model._h, None, ptr(steps), 2) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_flood_at(model._h, ptr(good), None, 2) == L.ERR_INVALID_ARGUMENT
    paths = lib.dust_hip_model_flood_paths
    assert paths(model._h, ptr(bad), 2, 3, ptr(keys), ptr(lengths)) == L.ERR_INVALID_ARGUMENT
    assert paths(model._h, None, 2, 3, ptr(keys), ptr(lengths)) == L.ERR_INVALID_ARGUMENT
    assert paths(model._h, ptr(good), 2, 3, None, ptr(lengths)) == L.ERR_INVALID_ARGUMENT
    assert paths(model._h, ptr(good), 2, 3, ptr(keys), None) == L.ERR_INVALID_ARGUMENT
    assert paths(model._h, None, 0, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert steps.tolist() == [77, 77] and (keys == 77).all() and (lengths == 77).all()
    assert paths(model._h, ptr(good), 2, 0, None, ptr(lengths)) == L.OK and lengths.tolist() == [1, 1]      # keys may be NULL when capacity == 0
    changed = C.c_uint32(77)
    assert lib.dust_hip_model_flood_apply(model._h, 0, 255, C.byref(changed)) == L.ERR_INVALID_ARGUMENT and changed.value == 77
    assert model.flood_at(good).tolist() == [0, 0] and same_bytes(model, grid, pal)
    assert lib.dust_hip_model_flood_apply(model._h, 0xFFFFFFFF, -(1 << 31), C.byref(changed)) == L.OK and changed.value == 0      # None into empty voxels
    # unsupported exactly where set_voxels is, before anything but the model is looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(W.brick_snake()[0], pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        h = unsupported._h
        assert status_of(lambda: unsupported.set_voxels([(0, 0, 0)], [1])) == L.ERR_UNSUPPORTED
        assert fn(h, C.byref(query()), ptr(good), 2, ptr(out)) == L.ERR_UNSUPPORTED
        assert fn(h, C.byref(query(medium=9)), ptr(bad), 2, ptr(out)) == L.ERR_UNSUPPORTED
        assert fn(h, None, None, 0, None) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_flood_at(h, ptr(bad), ptr(steps), 2) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_flood_at(h, None, None, 0) == L.ERR_UNSUPPORTED
        assert paths(h, ptr(bad), 2, 3, None, None) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_flood_apply(h, 0, 255, None) == L.ERR_UNSUPPORTED
    assert out.tobytes() == before
