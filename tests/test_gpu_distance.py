"""Model distances on the device (dust_hip_model_distance / distance_at / distance_apply; the contract is in include/dust_hip.h). Every
comparison is exact: the field and the result record must be the witness's (tests/distance_witness.py: the header's definition in
numpy), and a model a distance field was applied to must read back byte for byte what a host build of the witness's voxels uploads.
The counts pinned as literals are the witness's own, computed when the tests were written: a fixture that degenerates cannot pass."""
import ctypes as C
import time

import numpy as np
import pytest

import distance_witness as W
import flood_witness as FW
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
TARGETS = (L.DISTANCE_TO_SOLID, L.DISTANCE_TO_EMPTY, L.DISTANCE_TO_MATERIAL)
METRICS = (L.DISTANCE_EUCLIDEAN, L.DISTANCE_CHEBYSHEV)
FAR = L.DISTANCE_FAR
key = W.key


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


def record(r):
    return tuple(int(r[k]) for k in ("targets", "near", "far", "largest", "largest_key"))


def wall_w(xyz):
    return np.minimum(xyz + 1, 256 - xyz).min(axis=1)


@pytest.mark.parametrize("metric", METRICS)
def test_one_voxel_in_the_corner(metric):
    grid = W.single_voxel()
    pal = synth.make_palette(41)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    r = model.distance(metric=metric, max_radius=255)
    want = W.field(grid, W.TO_SOLID, metric, 255)
    assert r.tobytes() == W.result(want).tobytes()
    box = W.box_coordinates(((0, 0, 0), (11, 11, 11)))
    got = model.distance_at(box)
    assert np.array_equal(got, W.at(want, box))
    if metric == L.DISTANCE_EUCLIDEAN:
        assert np.array_equal(got, (box ** 2).sum(axis=1))
        assert model.distance_at([(255, 0, 0), (255, 1, 0), (0, 0, 0), (100, 200, 30), (180, 180, 19)]).tolist() == [65025, FAR, 0, 50900, FAR]
        assert record(r) == (1, 8758809, 8018406, 65025, key(0, 0, 255))          # (0, 0, 255), (0, 255, 0), (255, 0, 0), ...: the lowest key
    else:
        assert np.array_equal(got, box.max(axis=1))
        assert model.distance_at([(255, 0, 0), (255, 1, 0), (255, 255, 255), (3, 200, 7)]).tolist() == [255, 255, 255, 200]
        assert record(r) == (1, (1 << 24) - 1, 0, 255, key(0, 0, 255))
    assert same_bytes(model, grid, pal)          # the call moved the model into its editable form and changed no voxel


@pytest.mark.parametrize("metric", METRICS)
def test_lines_across_brick_cell_and_tree_seams(metric):
    grid = W.seams()
    pal = synth.make_palette(42)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    r = model.distance(metric=metric)
    want = W.field(grid, W.TO_SOLID, metric, 255)
    assert r.tobytes() == W.result(want).tobytes()
    assert record(r)[:2] == (15, 16777201) and int(r["largest"]) == (33083 if metric == L.DISTANCE_EUCLIDEAN else 165)
    for axis, fixed in W.SEAM_LINES:
        line = W.seam_line(axis, fixed)
        got = model.distance_at(line)
        assert np.array_equal(got, W.at(want, line)), axis
        assert got[list(W.SEAMS)].tolist() == [0] * 5 and got[[14, 17, 62, 65, 254]].tolist() == [1] * 5, axis
        lo = [0, 0, 0]
        hi = [255, 255, 255]
        for a, c in zip([a for a in range(3) if a != axis], fixed):
            lo[a], hi[a] = c - 5, c + 5
        slab = W.box_coordinates((lo, hi))                                           # 11 x 11 x 256 around the line
        assert np.array_equal(model.distance_at(slab), W.at(want, slab)), axis


RANDOM_RECORDS = {          # (target, metric, R): the witness's (targets, near, far, largest, largest_key)
    (0, 0, 1): (1339, 7483, 16768394, 1, 461606), (0, 0, 3): (1339, 64875, 16711002, 9, 330534), (0, 0, 255): (1339, 14769761, 2006116, 65025, 121322),
    (0, 1, 1): (1339, 26880, 16748997, 1, 461349), (0, 1, 3): (1339, 85271, 16690606, 3, 329763), (0, 1, 255): (1339, 16775877, 0, 213, 16646143),
    (1, 0, 1): (16775877, 1339, 0, 1, 527142), (1, 0, 3): (16775877, 1339, 0, 1, 527142), (1, 0, 255): (16775877, 1339, 0, 1, 527142),
    (1, 1, 1): (16775877, 1339, 0, 1, 527142), (1, 1, 3): (16775877, 1339, 0, 1, 527142), (1, 1, 255): (16775877, 1339, 0, 1, 527142),
    (2, 0, 1): (450, 2647, 16774119, 1, 464666), (2, 0, 3): (450, 37359, 16739407, 9, 333594), (2, 0, 255): (450, 14741472, 2035294, 65025, 121322),
    (2, 1, 1): (450, 10728, 16766038, 1, 464409), (2, 1, 3): (450, 65587, 16711179, 3, 332823), (2, 1, 255): (450, 16776766, 0, 213, 16578815),
}


@pytest.fixture(scope="module")
def random_model():
    """one model of the random fill for all the cases: a distance call changes no voxel"""
    grid, box = W.random_fill()
    pal = synth.make_palette(43)
    ctx = api.Context(device=0)
    return grid, W.box_coordinates(box), make(ctx, grid, pal), pal


@pytest.mark.parametrize("radius", (1, 3, 255))
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("target", TARGETS)
def test_random_fill(random_model, target, metric, radius):
    grid, xyz, model, pal = random_model
    want = W.field(grid, target, metric, radius, False, W.RANDOM_PALETTE)
    wanted = W.result(want)
    assert record(wanted) == RANDOM_RECORDS[(target, metric, radius)]      # the input has not degenerated
    first = None
    for again in range(2):
        got = model.distance(target=target, metric=metric, max_radius=radius, palette=W.RANDOM_PALETTE)
        print(f"target {target} metric {metric} R {radius}: {record(got)}")
        assert got.tobytes() == wanted.tobytes()
        values = model.distance_at(xyz)
        assert np.array_equal(values, W.at(want, xyz))
        first = values.tobytes() if first is None else first
        assert first == values.tobytes()
    if radius == 3:
        walled = model.distance(target=target, metric=metric, max_radius=radius, palette=W.RANDOM_PALETTE, walls=True)
        want = W.field(grid, target, metric, radius, True, W.RANDOM_PALETTE)
        assert walled.tobytes() == W.result(want).tobytes() and np.array_equal(model.distance_at(xyz), W.at(want, xyz))
    if (target, metric, radius) == (2, 1, 255):
        assert same_bytes(model, grid, pal)


@pytest.mark.parametrize("metric", METRICS)
def test_staircase(metric):
    """most lines see many different nearest targets: a stopping rule that ends the outward scan too early shows here"""
    grid = W.staircase()
    pal = synth.make_palette(44)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    r = model.distance(metric=metric)
    want = W.field(grid, W.TO_SOLID, metric, 255)
    assert r.tobytes() == W.result(want).tobytes()
    assert record(r) == ((65, 16161428, 615723, 65025, 255) if metric == L.DISTANCE_EUCLIDEAN else (65, 16777151, 0, 225, 65505))
    rng = np.random.default_rng(45)
    xyz = np.concatenate([W.box_coordinates(((0, 0, 0), (79, 79, 5))), W.box_coordinates(((190, 20, 80), (210, 40, 100))), rng.integers(0, 256, (20000, 3))])
    assert np.array_equal(model.distance_at(xyz), W.at(want, xyz))
    r = model.distance(metric=metric, max_radius=20, walls=True)
    want = W.field(grid, W.TO_SOLID, metric, 20, True)
    assert r.tobytes() == W.result(want).tobytes() and np.array_equal(model.distance_at(xyz), W.at(want, xyz))


def test_whole_tree_empty_and_full():
    pal = synth.make_palette(46)
    ctx = api.Context(device=0)
    rng = np.random.default_rng(47)
    xyz = rng.integers(0, 256, (4000, 3))
    xyz[:4] = [(0, 0, 0), (255, 255, 255), (127, 127, 127), (128, 128, 128)]
    w = wall_w(xyz)
    empty = np.zeros((256,) * 3, np.uint8)
    model = make(ctx, empty, pal)
    r = model.distance()
    assert record(r) == (0, 0, 1 << 24, 0, L.DISTANCE_NO_KEY)
    assert (model.distance_at(xyz) == FAR).all()
    assert model.distance_apply(3, 0, 0xFFFFFFFF) == 0 and same_bytes(model, empty, pal)
    for radius in (255, 100):
        r = model.distance(max_radius=radius, walls=True)
        assert np.array_equal(model.distance_at(xyz), np.where(w <= radius, w * w, FAR))
        far = (256 - 2 * radius) ** 3 if radius < 128 else 0
        assert record(r) == (0, (1 << 24) - far, far, min(radius, 128) ** 2, key(*((radius - 1,) * 3 if radius < 128 else (127, 127, 127))))
    full = np.full((256,) * 3, 4, np.uint8)
    model = make(ctx, full, pal)
    t0 = time.perf_counter()
    r = model.distance(target=L.DISTANCE_TO_EMPTY, metric=L.DISTANCE_CHEBYSHEV, walls=True)      # the first call also makes the model editable
    t1 = time.perf_counter()
    r = model.distance(target=L.DISTANCE_TO_EMPTY, metric=L.DISTANCE_CHEBYSHEV, walls=True)
    print(f"full tree, TO_EMPTY + WALLS, CHEBYSHEV, R = 255: {(t1 - t0) * 1e3:.2f} ms with make_editable, {(time.perf_counter() - t1) * 1e3:.2f} ms again")
    assert record(r) == (0, 1 << 24, 0, 128, key(127, 127, 127))
    assert np.array_equal(model.distance_at(xyz), w)
    r = model.distance(target=L.DISTANCE_TO_EMPTY, metric=L.DISTANCE_CHEBYSHEV, max_radius=7, walls=True)
    assert np.array_equal(model.distance_at(xyz), np.where(w <= 7, w, FAR)) and int(r["far"]) == 242 ** 3
    r = model.distance(target=L.DISTANCE_TO_EMPTY)          # no target anywhere, and no walls
    assert record(r) == (0, 0, 1 << 24, 0, L.DISTANCE_NO_KEY)
    r = model.distance(target=L.DISTANCE_TO_SOLID)          # every voxel is a target
    assert record(r) == (1 << 24, 0, 0, 0, 0)


def ray_grid(n=48):
    """n * n rays down onto the crater's ground"""
    u, v = np.meshgrid(np.linspace(2.3, 77.7, n, dtype=np.float32), np.linspace(2.6, 77.4, n, dtype=np.float32))
    origins = np.stack([u.reshape(-1), np.full(n * n, 120.0, np.float32), v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([0.05, -1.0, 0.03]), (n * n, 1))


def test_apply_grow_erode_skin_and_shell():
    grid, _, _ = FW.crater()
    pour = (38, 200, 42)          # in the air above the pit: empty whatever the cases do to the ground
    pal = synth.make_palette(48)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    origins, directions = ray_grid()
    cases = (("grow by 2", dict(target=L.DISTANCE_TO_SOLID, metric=L.DISTANCE_EUCLIDEAN, max_radius=2), 7, 1, 4),
             ("erode by 1", dict(target=L.DISTANCE_TO_EMPTY, metric=L.DISTANCE_EUCLIDEAN, max_radius=1), -1, 1, 1),
             ("skin", dict(target=L.DISTANCE_TO_EMPTY, metric=L.DISTANCE_EUCLIDEAN, max_radius=2), 8, 1, 4),
             ("shell", dict(target=L.DISTANCE_TO_SOLID, metric=L.DISTANCE_CHEBYSHEV, max_radius=3), 9, 2, 3))
    for name, query, value, lo, hi in cases:
        scene = api.Scene(ctx)
        scene.add_instance(model, IDENTITY.reshape(12))
        if name != "grow by 2":      # (the first call moves the model into its editable form: a scene committed before it is stale already)
            scene.commit()
        model.find_islands(L.ISLANDS_FACES)
        model.flood([pour])
        r = model.distance(**query)
        values = W.field(grid, query["target"], query["metric"], query["max_radius"])
        assert r.tobytes() == W.result(values).tobytes() and int(r["near"]) > 1000, name
        assert model.flood_at([pour]).tolist() == [0] and len(model.island_of([(10, 5, 10)])) == 1      # distance leaves both standing
        if name != "grow by 2":
            assert len(scene.trace_rays(origins, directions)) == len(origins)       # a distance call on an editable model changes nothing a scene reads
        grid, want_changed = W.apply(grid, values, value, lo, hi)
        changed = model.distance_apply(value, lo, hi)
        print(f"{name}: near {int(r['near'])} changed {changed}")
        assert changed == want_changed > 0, name
        assert same_bytes(model, grid, pal), name
        assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY
        scene.commit()
        got = scene.trace_rays(origins, directions)
        other = api.Scene(ctx)
        other.add_instance(make(ctx, grid, pal), IDENTITY.reshape(12))
        other.commit()
        assert got.tobytes() == other.trace_rays(origins, directions).tobytes(), name
        assert np.count_nonzero(got["instance"] != L.NO_HIT) > 1000
        assert status_of(lambda: model.distance_at([pour])) == L.ERR_NOT_READY
        assert status_of(lambda: model.flood_at([pour])) == L.ERR_NOT_READY
        assert status_of(lambda: model.island_of([pour])) == L.ERR_NOT_READY
    assert [np.count_nonzero(grid == b) for b in (8, 9, 10)] == [0, 28492, 35468]      # the skin took what the erosion left of the snow; the shell (and the vein's 52)


def test_validity_matrix():
    grid, empty, solid = FW.corridors()
    pal = synth.make_palette(49)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    other = make(ctx, FW.brick_snake()[0], pal)
    run = empty[0]
    xp = np.ascontiguousarray(run[:1], np.uint32)
    out16 = np.zeros(1, np.uint16)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def standing():
        return lib.dust_hip_model_distance_at(model._h, None, None, 0) == L.OK

    # nothing stands before the first call, with n == 0 as well
    assert lib.dust_hip_model_distance_at(model._h, None, None, 0) == L.ERR_NOT_READY
    assert lib.dust_hip_model_distance_at(model._h, ptr(xp), ptr(out16), 1) == L.ERR_NOT_READY
    assert lib.dust_hip_model_distance_apply(model._h, 1, 4, 1, None) == L.ERR_NOT_READY
    assert same_bytes(model, grid, pal)      # (never edited: byte-identical)

    def distance():
        r = model.distance(max_radius=4)
        assert int(r["targets"]) == np.count_nonzero(grid) and standing()

    distance()
    assert same_bytes(model, grid, pal)      # distance on a never-edited model leaves read() as it was
    assert model.distance_at(run[:3]).tolist() == [1, 1, 1]
    # what leaves the field standing
    model.find_islands(L.ISLANDS_FACES)
    assert standing() and model.island_of([solid[0][0]]).tolist() == [key(*solid[0][0])]
    assert int(model.flood([run[0]])["reached"]) == 31 and standing()
    piece = model.detach_islands([key(*solid[0][0])], keep_source=True)
    assert standing() and piece is not None
    other.stamp(model, api.stamps([(0, 0, 0)]))          # being a stamp's source
    assert standing()
    distance()                                            # a distance call leaves the labelling and the flood field
    assert model.island_of([solid[0][0]]).tolist() == [key(*solid[0][0])] and model.flood_at(run[-1:]).tolist() == [30]
    assert model.detach_islands([]) is None and standing()          # n == 0
    model.set_voxels(np.zeros((0, 3), np.uint32), np.zeros(0, np.int32))
    model.edit_shapes(np.zeros(0, api.EDIT_SHAPE_DTYPE))
    model.stamp(other, np.zeros(0, api.STAMP_DTYPE))
    assert standing()
    assert model.distance_at(run[-1:]).tolist() == [1]
    # what invalidates it, whether or not a voxel changes
    model.set_voxels([(200, 200, 200)], [-1])
    assert not standing()
    distance()
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]))        # a shape that covers nothing
    assert not standing()
    distance()
    model.stamp(other, api.stamps([(300, 0, 0)]))        # an image outside the tree
    assert not standing()
    distance()
    model.find_islands(L.ISLANDS_FACES)
    model.detach_islands([key(*solid[1][0])], want_model=False)                                # a carving detach
    assert not standing() and model.island_of([solid[0][0]]).tolist() == [key(*solid[0][0])]  # (the labelling of the rest stands)
    grid[tuple(solid[1].T)] = 0
    distance()
    model.flood([run[0]])
    assert model.flood_apply(2, max_steps=0) == 1        # flood_apply treats the distance field as it treats the labelling
    assert not standing()
    grid[tuple(run[0])] = 3
    distance()
    model.find_islands(L.ISLANDS_FACES)
    model.flood([run[1]])
    assert model.distance_apply(-1, 5, 4) == 0           # lo > hi matches nothing, and still invalidates all three
    assert not standing() and status_of(lambda: model.island_of([solid[0][0]])) == L.ERR_NOT_READY
    assert status_of(lambda: model.flood_at([run[1]])) == L.ERR_NOT_READY
    assert same_bytes(model, grid, pal)
    # a distance call that fails leaves none (here: refused before anything changes, so the field stands; see the refusals)
    distance()
    assert status_of(lambda: model.distance(max_radius=0)) == L.ERR_INVALID_ARGUMENT and standing()


def test_refusals_and_their_order():
    grid, empty, _ = FW.corridors()
    pal = synth.make_palette(50)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    run = empty[0]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = np.ascontiguousarray(run[:2], np.uint32)
    bad = good.copy()
    bad[1, 1] = 256

    def query(**kw):
        q = L.DistanceQuery(struct_size=C.sizeof(L.DistanceQuery), target=L.DISTANCE_TO_SOLID, metric=L.DISTANCE_EUCLIDEAN, max_radius=3)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    out = np.full(1, 0x5A, np.uint8).repeat(32).view(api.DISTANCE_RESULT_DTYPE)
    before = out.tobytes()
    fn = lib.dust_hip_model_distance
    refused = [None, query(struct_size=31), query(struct_size=0), query(target=3), query(metric=2), query(flags=2), query(flags=0x80000001),
               query(target=L.DISTANCE_TO_MATERIAL, palette=255), query(target=L.DISTANCE_TO_MATERIAL, palette=-1), query(max_radius=0),
               query(max_radius=256)]
    for stage in range(2):          # before any field, and with one standing: a refusal changes nothing
        for q in refused:
            assert fn(model._h, None if q is None else C.byref(q), ptr(out)) == L.ERR_INVALID_ARGUMENT
        assert out.tobytes() == before
        if stage == 0:
            assert lib.dust_hip_model_distance_at(model._h, None, None, 0) == L.ERR_NOT_READY
            assert same_bytes(model, grid, pal)
            # a coordinate is looked at before the field is
            values = np.full(2, 77, np.uint16)
            assert lib.dust_hip_model_distance_at(model._h, ptr(bad), ptr(values), 2) == L.ERR_INVALID_ARGUMENT
            assert lib.dust_hip_model_distance_at(model._h, ptr(good), ptr(values), 2) == L.ERR_NOT_READY
            assert lib.dust_hip_model_distance_apply(model._h, 1, 4, 255, None) == L.ERR_INVALID_ARGUMENT
            assert lib.dust_hip_model_distance_apply(model._h, 1, 4, 254, None) == L.ERR_NOT_READY
            assert fn(model._h, C.byref(query(palette=255, struct_size=64)), None) == L.OK      # palette is read under TO_MATERIAL only; out may be NULL
        else:
            assert model.distance_at(good).tolist() == [1, 1]
    values = np.full(2, 77, np.uint16)
    assert lib.dust_hip_model_distance_at(model._h, ptr(bad), ptr(values), 2) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_distance_at(model._h, None, ptr(values), 2) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_distance_at(model._h, ptr(good), None, 2) == L.ERR_INVALID_ARGUMENT
    assert values.tolist() == [77, 77]
    changed = C.c_uint32(77)
    assert lib.dust_hip_model_distance_apply(model._h, 1, 4, 255, C.byref(changed)) == L.ERR_INVALID_ARGUMENT and changed.value == 77
    assert model.distance_at(good).tolist() == [1, 1] and same_bytes(model, grid, pal)
    assert lib.dust_hip_model_distance_apply(model._h, 1, 0xFFFFFFFF, -(1 << 31), C.byref(changed)) == L.OK and changed.value == 0      # None into empty voxels
    assert lib.dust_hip_model_distance_at(model._h, None, None, 0) == L.ERR_NOT_READY
    # unsupported exactly where set_voxels is, before anything but the model is looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(FW.brick_snake()[0], pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        h = unsupported._h
        assert status_of(lambda: unsupported.set_voxels([(0, 0, 0)], [1])) == L.ERR_UNSUPPORTED
        assert fn(h, C.byref(query()), ptr(out)) == L.ERR_UNSUPPORTED
        assert fn(h, C.byref(query(target=9)), ptr(out)) == L.ERR_UNSUPPORTED
        assert fn(h, None, None) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_distance_at(h, ptr(bad), ptr(values), 2) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_distance_at(h, None, None, 0) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_distance_apply(h, 1, 4, 255, None) == L.ERR_UNSUPPORTED
    assert out.tobytes() == before
