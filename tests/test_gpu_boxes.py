"""Model boxes on the device (dust_hip_model_boxes; the contract is in include/dust_hip.h). Every comparison is exact: the result and
the full list must be, byte for byte, what the witness says (tests/boxes_witness.py), and a boxes call must leave the model as it
found it."""
import ctypes as C
import functools

import numpy as np
import pytest

import boxes_witness as W
import shape_edit_witness as SW
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
PLATE = ((120, 30, 120), (149, 32, 149))
ORIGINS = ((8, 8, 8), (8, 72, 8), (56, 8, 56))       # where the stacks made for axis n stand: 40^3 each, across 15 | 16 and 31 | 32 or 63 | 64
FULL = ((0, 0, 0), (255, 255, 255))


def host_model(grid, pal):
    return api.flatten_model(to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


def stacks():
    """shapes whose merge along the stacking axis can go wrong, in slice coordinates [s, v, u]"""
    b = np.zeros((40,) * 3, np.uint8)
    b[2, 2:5, 2:8], b[3, 2:5, 2:8] = 1, 2                                        # identical rects of two materials in adjacent slices
    b[2, 10:13, 2:8], b[3, 10:13, 2:9], b[4, 10:14, 2:9] = 3, 3, 3               # the same corner: then a longer u1, then a taller v1
    b[2, 20:23, 2:8], b[3, 20:23, 3:9], b[4, 21:24, 3:9] = 3, 3, 3               # the same extents shifted by one voxel along u, then along v
    for k in range(4):
        b[8 + k, 2:5, 2:6 + k] = 4                                               # a staircase along n
    b[8:11, 10:13, 10:13] = 5
    b[10, 11, 11] = 0                                                            # three slices, the third lacks its middle voxel
    b[14:17, 20:23, 20:26], b[17:20, 20:24, 20:26] = 6, 6                        # two different stacks on one (v0, u0), one after the other
    b[14:17, 30:32, 30:34], b[17:20, 30:32, 30:34] = 6, 7                        # ... and two that differ in material only
    b[22:30, 5:9, 21:27] = 1                                                     # a stack eight deep across 31 | 32 (n = x), 95 | 96 (n = y) or 79 | 80 (n = z)
    return b


def stack_region(n, s, v, u):
    """the tree region of slice coordinates s, v, u (inclusive pairs) of the stacks made for axis n"""
    lo, hi = [0, 0, 0], [0, 0, 0]
    for axis, (a, b) in zip(W.AXES[n], (s, v, u)):
        lo[axis], hi[axis] = ORIGINS[n][axis] + a, ORIGINS[n][axis] + b
    return tuple(lo), tuple(hi)


@functools.lru_cache(maxsize=None)
def hand_built_grid():
    """the smallest shapes at which the merge can go wrong, each away from the others"""
    grid = np.zeros((256,) * 3, np.uint8)
    grid[0, 0, 0], grid[255, 255, 255] = 1, 2                   # the two corners of the tree
    grid[10:70, 200:202, 200:202], grid[204:206, 10:70, 204:206], grid[208:210, 208:210, 10:70] = 3, 4, 5      # 2 x 2 bars across 15 | 16, 31 | 32 and 63 | 64
    grid[:, 220, 100], grid[224, :, 104], grid[228, 108, :] = 6, 6, 6                  # full-length columns: the extent 256
    grid[120:150, 30:33, 120:150] = 8                           # the plate: 3 thick along y
    grid[123, 31, 124] = 0                                      # ... with a cavity in its middle layer
    grid[120:150, 30:33, 134:136] = 9                           # ... and a stripe of a second material, two voxels wide along z
    grid[100:104, 104:108, 108:112] = 7                         # one brick exactly
    grid[160:176, 60:76, 160:176] = (np.indices((16,) * 3).sum(axis=0) & 1).astype(np.uint8) * 4      # a 3-D checkerboard
    for n, (x, y, z) in enumerate(ORIGINS):
        np.transpose(grid[x:x + 40, y:y + 40, z:z + 40], W.AXES[n])[...] = stacks()
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def random_block_grid(which):
    """a 40^3 block across 15 | 16 and 31 | 32 on every axis: density 0.5 with one material, 0.9 with two, 0.97 with three"""
    density, materials = ((0.5, 1), (0.9, 2), (0.97, 3))[which]
    rng = np.random.default_rng(110 + which)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[10:50, 10:50, 10:50] = np.where(rng.random((40,) * 3) < density, rng.integers(1, materials + 1, (40,) * 3), 0)
    grid.setflags(write=False)
    return grid


def grid_of(which):
    return hand_built_grid() if which == "hand" else random_block_grid(which)


@functools.lru_cache(maxsize=None)
def whole(which, axis, any_palette):
    """the witness over the whole tree, computed once and shared: (result, boxes), never written to"""
    result, boxes = W.boxes(grid_of(which), axis=axis, any_palette=any_palette)
    boxes.setflags(write=False)
    return result, boxes


@pytest.fixture(scope="module")
def hand():
    pal = synth.make_palette(71)
    ctx = api.Context(device=0)
    return make(ctx, hand_built_grid(), pal), hand_built_grid(), pal, ctx


def check(model, grid, want=None, **query):
    """one query on the device and in the witness: result and full list agree; returns them"""
    result, boxes = model.boxes(**query)
    want_result, want_boxes = want if want is not None else W.boxes(grid, **query)
    assert result.dtype == api.BOXES_RESULT_DTYPE and boxes.dtype == api.BOX_DTYPE
    assert result.tobytes() == want_result.tobytes(), (query, result, want_result)
    assert len(boxes) == len(want_boxes), (query, len(boxes), len(want_boxes))
    bad = np.flatnonzero(boxes != want_boxes)
    assert len(bad) == 0, (query, bad[:5], boxes[bad[:5]], want_boxes[bad[:5]])
    assert boxes.tobytes() == want_boxes.tobytes()
    alone, none = model.boxes(capacity=0, **query)                                # counts only: the same result
    assert alone.tobytes() == result.tobytes() and len(none) == 0
    surface_query = {k: v for k, v in query.items() if k in ("palette", "region")}
    assert int(result["voxels"]) == int(model.surface(capacity=0, **surface_query)[0]["solid"])
    return result, boxes


def corners(boxes):
    lo, hi = api.box_bounds(boxes)
    return [tuple(a) + tuple(b) for a, b in zip(lo.tolist(), hi.tolist())]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_hand_built_grid(hand, axis):
    model, grid, pal, _ = hand
    n = axis
    for any_palette in (False, True):
        result, boxes = check(model, grid, whole("hand", axis, any_palette), axis=axis, any_palette=any_palette)
        found = corners(boxes)
        # the corners of the tree, the bars, the full-length columns (the extent 256 is stored as 255), the brick
        for box in ((0, 0, 0, 0, 0, 0), (255,) * 6, (10, 200, 200, 69, 201, 201), (204, 10, 204, 205, 69, 205), (208, 208, 10, 209, 209, 69),
                    (0, 220, 100, 255, 220, 100), (224, 0, 104, 224, 255, 104), (228, 108, 0, 228, 108, 255), (100, 104, 108, 103, 107, 111)):
            assert box in found, box
        assert result["lo"].tolist() == [0, 0, 0] and result["hi"].tolist() == [255, 255, 255]
        brick, brick_boxes = check(model, grid, axis=axis, any_palette=any_palette, region=((100, 104, 108), (103, 107, 111)))
        assert (int(brick["boxes"]), int(brick["rects"]), int(brick["voxels"])) == (1, 4, 64) and brick_boxes[0].tolist() == ((100 << 16) | (104 << 8) | 108, 6, 3, 3, 3)
        board, _ = check(model, grid, axis=axis, any_palette=any_palette, region=((160, 60, 160), (175, 75, 175)))
        assert int(board["boxes"]) == int(board["rects"]) == int(board["voxels"]) == 2048
        # the plate: the stripe cuts every run along z, the cavity the middle layer; any_palette merges the stripe back
        plate, _ = check(model, grid, axis=axis, any_palette=any_palette, region=PLATE)
        assert int(plate["voxels"]) == 30 * 3 * 30 - 1 and 6 <= int(plate["boxes"]) <= int(plate["rects"])
        if axis == 0:                                           # slices x: three runs a row, the cavity's slice in four pieces instead of one
            assert int(plate["boxes"]) == (6 if any_palette else 8)
        # the stacks made for this axis, shape by shape
        def count(s, v, u):
            part, _ = check(model, grid, axis=axis, any_palette=any_palette, region=stack_region(n, s, v, u))
            return int(part["boxes"]), int(part["rects"]), int(part["voxels"])
        assert count((2, 3), (2, 4), (2, 7)) == ((1, 2, 36) if any_palette else (2, 2, 36))       # two materials
        assert count((2, 4), (10, 13), (2, 8)) == (3, 3, 18 + 21 + 28)                            # a longer u1, a taller v1: neither stacks
        assert count((2, 4), (20, 23), (2, 8)) == (3, 3, 54)                                      # shifted by one voxel
        assert count((8, 11), (2, 4), (2, 8)) == (4, 4, 3 * (4 + 5 + 6 + 7))                      # the staircase
        assert count((8, 10), (10, 12), (10, 12)) == (5, 6, 26)                                   # the third slice lacks its middle voxel
        assert count((14, 19), (20, 23), (20, 25)) == (2, 6, 54 + 72)                             # the walk stops between two stacks on one corner
        assert count((14, 19), (30, 31), (30, 33)) == ((1, 6, 48) if any_palette else (2, 6, 48))
        assert count((22, 29), (5, 8), (21, 26)) == (1, 8, 192)
        lo, hi = stack_region(n, (14, 16), (20, 22), (20, 25))
        assert lo + hi in found and stack_region(n, (17, 19), (20, 23), (20, 25))[0] + stack_region(n, (17, 19), (20, 23), (20, 25))[1] in found
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def test_random_blocks():
    pal = synth.make_palette(72)
    ctx = api.Context(device=0)
    for which in range(3):
        model = make(ctx, random_block_grid(which), pal)
        deeper = 0
        for axis in range(3):
            for any_palette in (False, True):
                _, boxes = check(model, random_block_grid(which), whole(which, axis, any_palette), axis=axis, any_palette=any_palette)
                extent = (boxes["dx"], boxes["dy"], boxes["dz"])[axis]
                deeper += int(np.count_nonzero(extent))
        assert deeper > 0, which                                                  # some box is deeper than one slice


def test_full_tree_and_empty_model():
    pal = synth.make_palette(73)
    ctx = api.Context(device=0)
    model = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    zero = W.zero_result()
    for axis in range(3):
        result, boxes = model.boxes(axis=axis, any_palette=bool(axis & 1))
        assert result.tobytes() == zero.tobytes() and len(boxes) == 0
    assert model.edit_shapes(SW.shapes(SW.shape(SW.BOX, (-1e30,) * 3, (1e30,) * 3, op=SW.FILL, palette=254))).tolist() == [1 << 24]
    for axis in range(3):
        for any_palette in (False, True):
            result, boxes = model.boxes(axis=axis, any_palette=any_palette)
            assert (int(result["boxes"]), int(result["rects"]), int(result["voxels"])) == (1, 256, 1 << 24)
            assert result["lo"].tolist() == [0, 0, 0] and result["hi"].tolist() == [255, 255, 255] and not result["reserved"].any()
            assert boxes.tolist() == [(0, 254, 255, 255, 255)]
            assert model.boxes(axis=axis, any_palette=any_palette, capacity=0)[0].tobytes() == result.tobytes()
    assert model.boxes(region=((9, 9, 9), (8, 200, 200)))[0].tobytes() == zero.tobytes()      # lo > hi: legal and empty
    inner, inner_boxes = model.boxes(axis=1, region=((5, 3, 7), (5, 250, 9)))     # a region of the full tree is one box
    assert inner_boxes.tolist() == [((5 << 16) | (3 << 8) | 7, 254, 0, 247, 2)] and int(inner["rects"]) == 248


def test_regions(hand):
    model, grid, _, ctx = hand
    for axis in range(3):
        n = axis
        # one that cuts a box on all three axes: the 8-deep stack, and the plate
        cut, cut_boxes = check(model, grid, axis=axis, region=stack_region(n, (24, 27), (6, 7), (22, 30)))
        assert (int(cut["boxes"]), int(cut["voxels"])) == (1, 4 * 2 * 5)
        check(model, grid, axis=axis, region=((125, 31, 122), (140, 32, 140)))
        check(model, grid, axis=axis, any_palette=True, region=((125, 31, 122), (140, 32, 140)))
        # one slice thick: every rect is a box
        lo, hi = list(FULL[0]), list(FULL[1])
        lo[n] = hi[n] = ORIGINS[n][n] + 9
        thin, _ = check(model, grid, axis=axis, region=(tuple(lo), tuple(hi)))
        assert int(thin["boxes"]) == int(thin["rects"]) > 0
        # a single voxel; lo > hi
        one, one_boxes = check(model, grid, axis=axis, region=((100, 104, 108), (100, 104, 108)))
        assert one_boxes.tolist() == [((100 << 16) | (104 << 8) | 108, 6, 0, 0, 0)] and int(one["rects"]) == 1
        assert check(model, grid, axis=axis, region=((101, 0, 0), (100, 255, 255)))[0].tobytes() == W.zero_result().tobytes()
        # the region's first slice has the identical rect just outside it: the box starts inside
        late, late_boxes = check(model, grid, axis=axis, region=stack_region(n, (25, 39), (0, 19), (20, 39)))
        assert int(late["boxes"]) == 1 and corners(late_boxes) == [stack_region(n, (25, 29), (5, 8), (21, 26))[0] + stack_region(n, (25, 29), (5, 8), (21, 26))[1]]
        lo, hi = list(FULL[0]), list(FULL[1])
        lo[n] = ORIGINS[n][n] + 25
        check(model, grid, axis=axis, region=(tuple(lo), tuple(hi)))
        # a palette filter leaves holes where the other materials were
        stripe, _ = check(model, grid, axis=axis, palette=7, region=PLATE)
        assert int(stripe["voxels"]) == 30 * 3 * 28 - 1
        check(model, grid, axis=axis, palette=5, any_palette=True)
        check(model, grid, axis=axis, palette=8)
    dense = random_block_grid(2)
    block = make(ctx, dense, synth.make_palette(74))
    for k, region in enumerate([((12, 13, 14), (30, 33, 47)), ((15, 0, 0), (16, 255, 255)), ((0, 31, 0), (255, 32, 255)), ((0, 0, 20), (255, 255, 20)), ((8, 8, 8), (51, 20, 51))]):
        check(block, dense, axis=k % 3, any_palette=bool(k & 1), palette=(-1, -1, 0, 1, 2)[k], region=region)


def test_stale_scratch_between_models_of_a_context():
    """the D volume is the context's and is reused: what a call on the full tree left must not lengthen a later model's boxes"""
    pal = synth.make_palette(75)
    ctx = api.Context(device=0)
    full = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    full.edit_shapes(SW.shapes(SW.shape(SW.BOX, (-1e30,) * 3, (1e30,) * 3, op=SW.FILL, palette=3)))
    empty = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    empty.set_voxels([(200, 200, 200)], [1])
    empty.set_voxels([(200, 200, 200)], [-1])
    for axis in range(3):
        extent = [8, 8, 8]
        extent[axis] = 4
        grid = np.zeros((256,) * 3, np.uint8)
        grid[:extent[0], :extent[1], :extent[2]] = 4
        small = make(ctx, grid, pal)
        for any_palette in (False, True):
            assert full.boxes(axis=axis, any_palette=any_palette)[1].tolist() == [(0, 3, 255, 255, 255)]     # every D plane has bit (0, 0) past the first
            result, boxes = check(small, grid, axis=axis, any_palette=any_palette)
            assert boxes.tolist() == [(0, 3, extent[0] - 1, extent[1] - 1, extent[2] - 1)] and int(result["rects"]) == 4
            assert full.boxes(axis=axis, any_palette=any_palette)[0]["boxes"] == 1
            result, boxes = empty.boxes(axis=axis, any_palette=any_palette)
            assert result.tobytes() == W.zero_result().tobytes() and len(boxes) == 0
            check(small, grid, axis=axis, any_palette=any_palette)                # ... and behind the empty tree's call


def test_capacity():
    grid = random_block_grid(1)
    pal = synth.make_palette(76)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    region = ((12, 10, 14), (40, 35, 30))
    for axis in (0, 2):
        want_result, want = W.boxes(grid, axis=axis, region=region)
        total = len(want)
        assert total > 500
        q = L.BoxesQuery(struct_size=C.sizeof(L.BoxesQuery), axis=axis, palette=-1)
        q.lo[:], q.hi[:] = region
        for capacity in (0, 1, total - 1, total, total + 5):
            out = np.full((total + 8) * 8, 0x5A, np.uint8).view(api.BOX_DTYPE)
            result = np.zeros(1, api.BOXES_RESULT_DTYPE)
            assert lib.dust_hip_model_boxes(model._h, C.byref(q), result.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), capacity) == L.OK
            written = min(capacity, total)
            assert out[:written].tobytes() == want[:written].tobytes(), capacity
            assert out[written:].tobytes() == b"\x5a" * (8 * (total + 8 - written)), capacity
            assert result[0].tobytes() == want_result.tobytes(), capacity
        # through the Python call: a given capacity truncates, None lists everything
        assert model.boxes(axis=axis, region=region, capacity=7)[1].tobytes() == want[:7].tobytes()
        assert model.boxes(axis=axis, region=region)[1].tobytes() == want.tobytes()


def ray_grid(n=8):
    """n * n rays along -x over the image of [0, 64)^3 under ROTATED"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def test_the_model_is_only_read():
    grid = random_block_grid(0)
    pal = synth.make_palette(77)
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
    check(fixed, grid, axis=1, region=region)
    check(fixed, grid, whole(0, 2, True), axis=2, any_palette=True)
    fixed.boxes(capacity=0, any_palette=True)                                     # (masks only: no grid is made)
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fixed.read(), host_model(grid, pal)))
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit: the generation has not moved, the model is not editable
    fixed.find_islands(L.ISLANDS_FACES, capacity=0)                               # the first-edit transition happens HERE, not in boxes
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY

    # an editable model is read in place, edits included; its labelling and both fields stand
    loose = make(ctx, grid, pal)
    loose.set_voxels([(20, 30, 16), (21, 30, 16), (60, 60, 60)], [2, -1, 0])
    edited = grid.copy()
    edited[20, 30, 16], edited[21, 30, 16], edited[60, 60, 60] = 3, 0, 1
    loose.find_islands(L.ISLANDS_FACES, capacity=0)
    loose.distance(max_radius=3)
    loose.flood([(100, 100, 100)], max_steps=90)
    keys, values, steps = loose.island_of(points), loose.distance_at(points), loose.flood_at(points)
    scene2 = api.Scene(ctx)
    scene2.add_instance(loose, ROTATED.reshape(12))
    scene2.commit()
    hits2 = scene2.trace_rays(origins, directions)
    check(loose, edited)
    check(loose, edited, axis=2, palette=2, any_palette=True)
    assert loose.island_of(points).tolist() == keys.tolist() and loose.distance_at(points).tolist() == values.tolist()
    assert loose.flood_at(points).tolist() == steps.tolist()
    assert scene2.trace_rays(origins, directions).tobytes() == hits2.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(loose.read(), host_model(edited, pal)))


@pytest.mark.parametrize("which", ["hand", 2])
def test_round_trip_through_edit_shapes(which):
    """the boxes placed into an empty model of the same palette give the source back, byte for byte a host build"""
    grid = grid_of(which)
    pal = synth.make_palette(78)
    ctx = api.Context(device=0)
    source = make(ctx, grid, pal)
    for axis, any_palette in ((0, False), (1, False), (2, False)):
        result, boxes = check(source, grid, whole(which, axis, any_palette), axis=axis, any_palette=any_palette)
        assert 0 < len(boxes) <= L.MAX_EDIT_SHAPES
        shapes = api.box_shapes(boxes)
        assert shapes.dtype == api.EDIT_SHAPE_DTYPE and np.all(shapes["kind"] == L.SHAPE_BOX) and np.all(shapes["op"] == L.EDIT_PLACE)
        lo, hi = api.box_bounds(boxes)
        assert lo.dtype == hi.dtype == np.int32 and np.array_equal(shapes["a"], lo) and np.array_equal(shapes["b"], hi + 1)
        copy = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
        changed = copy.edit_shapes(shapes)
        assert int(changed.sum()) == int(result["voxels"]) == int(source.surface(capacity=0)[0]["solid"])
        assert np.array_equal(changed, (hi - lo + 1).prod(axis=1))                # the boxes do not overlap: each one fills its own volume
        assert all(x.tobytes() == y.tobytes() for x, y in zip(copy.read(), host_model(grid, pal)))
    repainted = api.box_shapes(whole(which, 0, False)[1][:3], op=L.EDIT_FILL, palette=9)
    assert repainted["palette"].tolist() == [9, 9, 9] and np.all(repainted["op"] == L.EDIT_FILL)


def test_determinism_and_refusals():
    grid = random_block_grid(1)
    pal = synth.make_palette(79)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    for axis in range(3):
        first, second = model.boxes(axis=axis), model.boxes(axis=axis)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)) and int(first[0]["boxes"]) > 1000

    result = np.full(64, 0x5A, np.uint8).view(api.BOXES_RESULT_DTYPE)
    boxes = np.full(16 * 8, 0x5A, np.uint8).view(api.BOX_DTYPE)
    before = result.tobytes(), boxes.tobytes()
    rp, bp = (a.ctypes.data_as(C.c_void_p) for a in (result, boxes))

    def query(axis=0, flags=0, palette=-1, lo=(0, 0, 0), hi=(255, 255, 255), size=C.sizeof(L.BoxesQuery)):
        q = L.BoxesQuery(struct_size=size, axis=axis, flags=flags, palette=palette)
        q.lo[:], q.hi[:] = lo, hi
        return q
    bad = [query(axis=3), query(axis=1 << 31), query(flags=2), query(flags=1 << 31), query(palette=-2), query(palette=255), query(lo=(0, 256, 0)),
           query(hi=(255, 255, 256)), query(lo=(1 << 31, 0, 0)), query(size=47), query(size=0)]
    for q in bad:
        assert lib.dust_hip_model_boxes(model._h, C.byref(q), rp, bp, 16) == L.ERR_INVALID_ARGUMENT
    good = query()
    assert lib.dust_hip_model_boxes(None, C.byref(good), rp, bp, 16) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_boxes(model._h, None, rp, bp, 16) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_boxes(model._h, C.byref(good), rp, None, 16) == L.ERR_INVALID_ARGUMENT      # null boxes with capacity > 0
    assert (result.tobytes(), boxes.tobytes()) == before
    # every output may be null; a larger struct_size is a newer caller's
    assert lib.dust_hip_model_boxes(model._h, C.byref(query(size=64)), None, None, 0) == L.OK
    assert lib.dust_hip_model_boxes(model._h, C.byref(query(axis=2, flags=1)), None, None, 0) == L.OK
    assert lib.dust_hip_model_boxes(model._h, C.byref(query(lo=(3, 0, 0), hi=(2, 255, 255))), rp, bp, 16) == L.OK
    assert result.tobytes() == W.zero_result().tobytes() and boxes.tobytes() == before[1]      # lo > hi: the zero result, nothing listed
    result[:] = np.frombuffer(before[0], api.BOXES_RESULT_DTYPE)
    # unsupported exactly where set_voxels is, before the query is looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(grid, pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    for unsupported in (deep, odd):
        assert status_of(lambda: unsupported.boxes()) == L.ERR_UNSUPPORTED
        for q in (bad[0], bad[2], bad[4], bad[6]):
            assert lib.dust_hip_model_boxes(unsupported._h, C.byref(q), rp, bp, 16) == L.ERR_UNSUPPORTED
        assert lib.dust_hip_model_boxes(unsupported._h, None, rp, bp, 16) == L.ERR_UNSUPPORTED
    assert (result.tobytes(), boxes.tobytes()) == before
