"""Shape edits on the device (dust_hip_model_edit_shapes; the contract is in include/dust_hip.h): after every batch of boxes, spheres
and capsules the model's device arrays must be byte for byte what a host rebuild of the witness's voxels uploads
(tests/shape_edit_witness.py: the header's float32 formulas in numpy), `changed` must equal the witness's counts exactly, a twin
model taken through the same voxels with set_voxels must read back the same bytes, and frames and queries must see the edit."""
import ctypes as C
import functools

import numpy as np
import pytest

import parity_util as P
import shape_edit_witness as W
from dust_amd import _lib as L, api, synth
from shape_edit_witness import BOX, CAPSULE, CARVE, FILL, PAINT, PLACE, SPHERE

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)


def host_model(vox, pal):
    """voxel dict {(x, y, z) tree coords: palette index} -> (blocks, materials) through the product's host flatten"""
    if not vox:
        return api.flatten_model(np.zeros((0, 4), np.uint8), (256, 256, 256), pal)
    k = np.array(list(vox.keys()), np.int64)
    v = np.array(list(vox.values()), np.int64)
    xyzi = np.stack([k[:, 0], 255 - k[:, 2], k[:, 1], v], axis=1).astype(np.uint8)  # loader.rs:248-253: engine (x, z, size.y-1-y)
    return api.flatten_model(xyzi, (256, 256, 256), pal)


def start_voxels(rng, n=6000):
    """scattered voxels plus a solid slab of full bricks"""
    vox = {}
    for c in rng.integers(20, 120, (n, 3)):
        vox[tuple(int(t) for t in c)] = int(rng.integers(0, 255))
    for x in range(40, 56):
        for y in range(40, 44):
            for z in range(40, 56):
                vox[(x, y, z)] = 7
    return vox


def random_shapes(rng, kind, n, lo, hi, size):
    """n shapes of one kind with float coordinates in [lo, hi], extents up to `size`, random ops and colours"""
    a = rng.uniform(lo, hi, (n, 3))
    if kind == BOX:
        b = a + rng.uniform(0.0, size, (n, 3))
    else:
        b = a + rng.uniform(-size, size, (n, 3))
    return api.edit_shapes(kind, a, b, radius=rng.uniform(0.0, size / 2, n), op=rng.integers(0, 4, n), palette=rng.integers(0, 255, n))


@functools.lru_cache(maxsize=None)
def batches():
    """[(name, shapes)]: the batches of the sequence tests, in order"""
    rng = np.random.default_rng(31)
    out = []
    every = []
    for kind in (BOX, SPHERE, CAPSULE):        # each kind x each op, over the slab and the scattered voxels
        for op in (CARVE, FILL, PAINT, PLACE):
            a = rng.uniform(36.0, 60.0, 3)
            b = a + rng.uniform(3.0, 14.0, 3)
            every.append(W.shape(kind, a, b, radius=float(rng.uniform(2.0, 6.0)), op=op, palette=int(rng.integers(0, 255))))
    out.append(("every kind x op", W.shapes(*every)))
    c = (100.5, 100.5, 100.5)
    lo, hi = np.nextafter(np.float32(10.5), np.float32(11)), np.nextafter(np.float32(12.5), np.float32(12))
    out.append(("boundary-exact", W.shapes(
        W.shape(SPHERE, c, radius=5.0, op=FILL, palette=11),               # 515 voxels: the 30 at distance exactly 5 are inside
        W.shape(SPHERE, c, radius=4.99, op=CARVE),                         # 485: the shell of 30 stays
        W.shape(BOX, (10.5, 20.5, 30.5), (12.5, 20.5, 31.5), op=FILL, palette=12),   # bounds on centres: 3 x 1 x 2
        W.shape(BOX, (lo, 0.0, 0.0), (hi, 1.0, 1.0), op=FILL, palette=13),           # just short of the centres: 1
        W.shape(BOX, (3.5, 4.5, 5.5), (3.5, 4.5, 5.5), op=FILL, palette=14),         # a point on a centre: 1
        W.shape(CAPSULE, (17.3, 140.9, 8.2), (17.3, 140.9, 8.2), radius=6.7, op=FILL, palette=15),   # a == b: the sphere
        W.shape(SPHERE, (17.3, 140.9, 8.2), radius=6.7, op=CARVE),                                     # ... which removes all of it
        W.shape(CAPSULE, (50.5, 160.5, 70.5), (58.5, 160.5, 70.5), radius=2.0, op=FILL, palette=16), # 137
        W.shape(CAPSULE, (-5.5, 3.5, 3.5), (2.5, 3.5, 3.5), radius=0.0, op=FILL, palette=17),        # the axis voxels alone: 3
        W.shape(CAPSULE, (80.5, 200.5, 80.5), (80.5 + 1e-20, 200.5, 80.5), radius=3.0, op=FILL, palette=18),   # b - a rounds to 0
        W.shape(CAPSULE, (1e-30, 210.5, 90.5), (3e-20, 210.5, 90.5), radius=2.5, op=FILL, palette=19),          # dot(ab, ab) underflows
        W.shape(SPHERE, (150.5, 150.5, 150.5), radius=-0.0, op=FILL, palette=20))))                             # 1
    out.append(("random boxes", random_shapes(rng, BOX, 220, 10.0, 130.0, 12.0)))
    out.append(("random spheres", random_shapes(rng, SPHERE, 220, 10.0, 130.0, 12.0)))
    out.append(("random capsules", random_shapes(rng, CAPSULE, 220, 10.0, 130.0, 12.0)))
    mixed = np.concatenate([random_shapes(rng, k, 40, 5.0, 250.0, 30.0) for k in (BOX, SPHERE, CAPSULE)])
    out.append(("random mixed, larger", mixed[rng.permutation(len(mixed))]))
    faces = [W.shape(BOX, (-5.0, -5.0, -5.0), (1.5, 1.5, 1.5), op=FILL, palette=21),
             W.shape(BOX, (254.5, 254.5, 254.5), (1e30, 300.0, 256.0), op=FILL, palette=22),
             W.shape(BOX, (256.0, 0.0, 0.0), (300.0, 10.0, 10.0), op=FILL, palette=23),        # outside: 0
             W.shape(SPHERE, (-0.5, 0.5, 0.5), radius=1.0, op=PAINT, palette=24),
             W.shape(SPHERE, (256.5, 255.5, 0.5), radius=1.0, op=FILL, palette=25),
             W.shape(SPHERE, (-3.0, 128.2, 257.9), radius=9.5, op=FILL, palette=26),
             W.shape(CAPSULE, (-20.0, 100.3, 30.1), (280.0, 110.2, 31.7), radius=1.7, op=PLACE, palette=27),   # through two faces
             W.shape(CAPSULE, (128.0, -9.0, 128.0), (128.0, 300.0, 130.0), radius=2.2, op=FILL, palette=28),
             W.shape(SPHERE, (65536.0, 30.5, 30.5), radius=65281.0, op=PLACE, palette=29),     # the coordinate limit: a near-flat disc on the x = 255 layer
             W.shape(SPHERE, (65536.0, 30.5, 30.5), radius=65280.75, op=CARVE)]                # ... and its inner part taken out again
    for k in (BOX, SPHERE, CAPSULE):
        faces += list(random_shapes(rng, k, 12, -20.0, 20.0, 25.0)) + list(random_shapes(rng, k, 12, 236.0, 276.0, 25.0))
    out.append(("straddling the faces", W.shapes(*faces)))
    nan = float("nan")
    out.append(("shapes that cover nothing among shapes that do", W.shapes(
        W.shape(BOX, (60, 60, 60), (70, 70, 70), op=FILL, palette=30), W.shape(BOX, (nan, 60, 60), (70, 70, 70), op=CARVE),
        W.shape(BOX, (65, 60, 60), (64, 70, 70), op=CARVE), W.shape(SPHERE, (65, 65, 65), radius=-1.0, op=CARVE),
        W.shape(SPHERE, (65, 65, 65), radius=float("inf"), op=CARVE), W.shape(SPHERE, (65, 65, 65), radius=65537.0, op=CARVE),
        W.shape(CAPSULE, (65, 65, 65), (1e5, 65, 65), radius=1.0, op=CARVE), W.shape(CAPSULE, (65, 65, 65), (66, nan, 65), radius=1.0, op=CARVE),
        W.shape(BOX, (60, 60, 60), (70, 70, 70), radius=nan, op=PAINT, palette=31),          # a box ignores its radius
        W.shape(SPHERE, (65.5, 65.5, 65.5), (nan, nan, nan), radius=2.0, op=CARVE))))        # a sphere ignores b
    out.append(("whole-tree carve, then a fill", W.shapes(
        W.shape(BOX, (-1e30,) * 3, (1e30,) * 3, op=CARVE), W.shape(BOX, (90.0, 100.0, 110.0), (150.0, 140.0, 170.0), op=FILL, palette=33),
        W.shape(BOX, (-1e30,) * 3, (1e30,) * 3, op=PAINT, palette=34), W.shape(SPHERE, (120.0, 120.0, 140.0), radius=10.0, op=CARVE))))
    n = 4096    # small spheres, heavy overlap: about 33 per voxel of a 32^3 region
    out.append(("4096 small spheres", api.edit_shapes(SPHERE, rng.uniform(100.0, 132.0, (n, 3)), radius=rng.uniform(1.0, 2.5, n),
                                                      op=rng.integers(0, 4, n), palette=rng.integers(0, 255, n))))
    return out


@functools.lru_cache(maxsize=None)
def witnessed():
    """the start voxels and, per batch, (name, shapes, changed, the grid after it) by the witness"""
    grid = W.to_grid(start_voxels(np.random.default_rng(30)))
    steps = []
    for name, shapes in batches():
        changed = W.apply_to_grid(grid, shapes)
        steps.append((name, shapes, changed, grid.copy()))
    return steps


def test_the_batches_cover_what_they_claim():
    names = dict(batches())
    every = names["every kind x op"]
    assert {(int(k), int(o)) for k, o in zip(every["kind"], every["op"])} == {(k, o) for k in range(3) for o in range(4)}
    for kind, name in ((BOX, "random boxes"), (SPHERE, "random spheres"), (CAPSULE, "random capsules")):
        assert len(names[name]) >= 200 and np.all(names[name]["kind"] == kind)
    assert len(names["4096 small spheres"]) == 4096
    by_name = {name: changed for name, _, changed, _ in witnessed()}
    assert by_name["boundary-exact"].tolist() == [515, 485, 6, 1, 1, by_name["boundary-exact"][5], by_name["boundary-exact"][5], 137, 3,
                                                  by_name["boundary-exact"][9], by_name["boundary-exact"][10], 1]
    assert by_name["boundary-exact"][5] > 1000 and by_name["boundary-exact"][9] == 123 and by_name["boundary-exact"][10] > 0   # r = 3 on a centre: 123 offsets
    for name, changed in by_name.items():     # no batch is idle
        assert np.count_nonzero(changed) >= 1, name
    faces = by_name["straddling the faces"].tolist()
    assert faces[:5] == [8, 8, 0, 1, 1] and faces[8] > 10000 and 0 < faces[9] < faces[8]
    assert by_name["shapes that cover nothing among shapes that do"].tolist()[1:8] == [0] * 7


def test_shape_edits_equal_a_host_rebuild():
    pal = synth.make_palette(4)
    ctx = api.Context(device=0)
    rng = np.random.default_rng(32)
    vox = start_voxels(np.random.default_rng(30))
    b0, m0 = host_model(vox, pal)
    model = api.Model(ctx, b0, m0, pal)
    assert model.edit_shapes(np.zeros(0, api.EDIT_SHAPE_DTYPE)).tolist() == []       # n == 0: a no-op
    got_b, got_m = model.read()
    assert got_b.tobytes() == b0.tobytes() and got_m.tobytes() == m0.tobytes()
    for name, shapes, want_changed, grid in witnessed():
        changed = model.edit_shapes(shapes)
        vox = W.to_dict(grid)
        assert changed.dtype == np.uint32 and len(changed) == len(shapes)
        bad = np.flatnonzero(changed != want_changed)
        print(f"{name}: {len(shapes)} shapes, {int(want_changed.sum(dtype=np.int64))} changes, {len(vox)} voxels after", flush=True)
        assert len(bad) == 0, f"{name}: changed differs at {bad[:8].tolist()}: {changed[bad[:8]].tolist()} != {want_changed[bad[:8]].tolist()} for {shapes[bad[:3]]}"
        want_b, want_m = host_model(vox, pal)
        got_b, got_m = model.read()
        assert len(got_b) == len(want_b) and len(got_m) == len(want_m), name
        assert got_b.tobytes() == want_b.tobytes(), f"{name}: Block records differ"
        assert got_m.tobytes() == want_m.tobytes(), f"{name}: material stream differs"
        nb, nm = C.c_uint32(), C.c_uint64()
        L.check(L.load().dust_hip_model_info(model._h, C.byref(nb), C.byref(nm)))
        assert nm.value == len(vox) and nb.value == len(want_b), name
        keys = list(vox.keys())
        probe = [keys[i] for i in rng.integers(0, len(keys), 200)] + [tuple(int(t) for t in c) for c in rng.integers(0, 256, (100, 3))]
        probe = np.array(probe + [(1, 2, 3), (250, 250, 250), (0, 0, 0), (255, 255, 255)], np.uint32).reshape(-1, 3)
        assert model.get_voxels(probe).tolist() == [vox.get(tuple(int(t) for t in c), -1) for c in probe], name
    # deterministic: the same sequence on a second model gives the same counts and bytes
    again = api.Model(ctx, b0, m0, pal)
    for name, shapes, want_changed, _ in witnessed():
        assert np.array_equal(again.edit_shapes(shapes), want_changed), name
    for x, y in zip(again.read(), model.read()):
        assert x.tobytes() == y.tobytes()


def test_a_twin_edited_through_set_voxels_reads_back_the_same_bytes():
    pal = synth.make_palette(4)
    ctx = api.Context(device=0)
    start = W.to_grid(start_voxels(np.random.default_rng(30)))
    b0, m0 = host_model(W.to_dict(start), pal)
    shaped, twin = api.Model(ctx, b0, m0, pal), api.Model(ctx, b0, m0, pal)
    before = start
    for name, shapes, _, grid in witnessed():
        shaped.edit_shapes(shapes)
        xyz, values = W.edit_list(before, grid)
        twin.set_voxels(xyz, values)
        (sb, sm), (tb, tm) = shaped.read(), twin.read()
        assert len(sm) == int(np.count_nonzero(grid)), name
        assert sb.tobytes() == tb.tobytes(), f"{name}: Block records differ"
        assert sm.tobytes() == tm.tobytes(), f"{name}: material stream differs"
        before = grid


def test_order_one_call_two_calls_and_swapped():
    pal = synth.make_palette(2)
    ctx = api.Context(device=0)
    vox = start_voxels(np.random.default_rng(33), 3000)
    b0, m0 = host_model(vox, pal)
    one = W.shape(BOX, (38.0, 38.0, 38.0), (52.0, 46.0, 50.0), op=FILL, palette=1)
    two = W.shape(SPHERE, (50.2, 43.1, 49.7), radius=6.3, op=PAINT, palette=2)
    want_ab, ch_ab = W.apply(vox, W.shapes(one, two))
    want_ba, ch_ba = W.apply(vox, W.shapes(two, one))
    assert want_ab != want_ba
    single, split, swapped = (api.Model(ctx, b0, m0, pal) for _ in range(3))
    assert single.edit_shapes(W.shapes(one, two)).tolist() == ch_ab.tolist()
    assert split.edit_shapes(W.shapes(one)).tolist() + split.edit_shapes(W.shapes(two)).tolist() == ch_ab.tolist()
    assert swapped.edit_shapes(W.shapes(two, one)).tolist() == ch_ba.tolist()
    for x, y in zip(single.read(), split.read()):
        assert x.tobytes() == y.tobytes()
    for model, want in ((single, want_ab), (swapped, want_ba)):
        for x, y in zip(model.read(), host_model(want, pal)):
            assert x.tobytes() == y.tobytes()
    assert single.read()[1].tobytes() != swapped.read()[1].tobytes()


def test_refusals_leave_the_model_unchanged():
    pal = synth.make_palette(1)
    ctx = api.Context(device=0)
    vox = start_voxels(np.random.default_rng(34), 500)
    model = api.Model(ctx, *host_model(vox, pal), pal)
    good = W.shape(BOX, (30.0, 30.0, 30.0), (60.0, 60.0, 60.0), op=FILL, palette=3)
    assert model.edit_shapes(W.shapes(W.shape(BOX, (0.2, 0.2, 0.2), (0.8, 0.8, 0.8), op=FILL, palette=9))).tolist() == [1]   # (editable from here on)
    b0, m0 = model.read()
    bad = [W.shapes(good, W.shape(3, (40.0,) * 3, radius=2.0)), W.shapes(good, W.shape(0xFFFFFFFF, (40.0,) * 3)),
           W.shapes(good, W.shape(BOX, (40.0,) * 3, (50.0,) * 3, op=4)),
           W.shapes(good, W.shape(BOX, (40.0,) * 3, (50.0,) * 3, op=FILL, palette=255)),
           W.shapes(good, W.shape(SPHERE, (40.0,) * 3, radius=2.0, op=PAINT, palette=-1)),
           W.shapes(good, W.shape(CAPSULE, (40.0,) * 3, radius=2.0, op=PLACE, palette=1000)),
           np.repeat(W.shapes(good), L.MAX_EDIT_SHAPES + 1)]
    for shapes in bad:
        assert W.refused(shapes)
        with pytest.raises(L.DustError) as e:
            model.edit_shapes(shapes)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        b1, m1 = model.read()
        assert b1.tobytes() == b0.tobytes() and m1.tobytes() == m0.tobytes()
    lib = L.load()
    assert lib.dust_hip_model_edit_shapes(model._h, None, 1, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_edit_shapes(model._h, None, 0, None) == L.OK                 # n == 0: a no-op, whatever the arrays
    one = W.shapes(W.shape(BOX, (0.2, 0.2, 0.2), (0.8, 0.8, 0.8), op=CARVE, palette=999))     # CARVE ignores the palette; changed may be NULL
    assert lib.dust_hip_model_edit_shapes(model._h, one.ctypes.data_as(C.c_void_p), 1, None) == L.OK
    want, _ = W.apply(vox, one)
    assert want == vox
    for x, y in zip(model.read(), host_model(vox, pal)):
        assert x.tobytes() == y.tobytes()
    # unsupported exactly where set_voxels is: a 4096^3 tree
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    with pytest.raises(L.DustError) as e:
        deep.edit_shapes(W.shapes(good))
    assert e.value.status == L.ERR_UNSUPPORTED


def test_many_whole_tree_shapes_and_the_shape_limit():
    """Answers known without the witness. 1 100 whole-tree boxes (every one listed in all 4 096 root cells: more list entries than one
    launch carries, so the call is cut into chunks that must keep the order): each FILL changes every voxel, because its colour
    differs from its predecessor's. Then exactly DUST_HIP_MAX_EDIT_SHAPES single-voxel boxes on distinct empty voxels: each changes one."""
    pal = synth.make_palette(7)
    ctx = api.Context(device=0)
    vox = start_voxels(np.random.default_rng(37), 2000)
    model = api.Model(ctx, *host_model(vox, pal), pal)
    n = 1100
    everything = api.edit_shapes(BOX, np.full((n, 3), -1e30), np.full((n, 3), 1e30), op=FILL, palette=np.arange(n) % 7)
    everything["op"][n - 2] = CARVE
    everything[n - 1] = W.shape(BOX, (200.0, 200.0, 200.0), (202.0, 202.0, 202.0), op=FILL, palette=9)
    want = np.full(n, 256 ** 3, np.int64)
    want[0] -= sum(1 for v in vox.values() if v == 0)     # already colour 0
    want[n - 1] = 8
    changed = model.edit_shapes(everything)
    assert changed.astype(np.int64).tolist() == want.tolist()
    after = {(x, y, z): 9 for x in (200, 201) for y in (200, 201) for z in (200, 201)}
    for x, y in zip(model.read(), host_model(after, pal)):
        assert x.tobytes() == y.tobytes()
    # the limit itself: 65 536 shapes in one call, ids up to 65 535
    rng = np.random.default_rng(38)
    flat = rng.choice(256 ** 3, L.MAX_EDIT_SHAPES + 64, replace=False)       # distinct voxels ...
    cells = np.stack([flat >> 16, (flat >> 8) & 255, flat & 255], axis=1)
    cells = cells[~np.all((cells >= 200) & (cells < 202), axis=1)][: L.MAX_EDIT_SHAPES]   # ... none of them one of the 8 above
    colours = rng.integers(0, 255, len(cells))
    dots = api.edit_shapes(BOX, cells + 0.25, cells + 0.75, op=PLACE, palette=colours)
    assert len(dots) == L.MAX_EDIT_SHAPES
    changed = model.edit_shapes(dots)
    assert changed.tolist() == [1] * L.MAX_EDIT_SHAPES
    after.update({tuple(int(t) for t in c): int(v) for c, v in zip(cells, colours)})
    for x, y in zip(model.read(), host_model(after, pal)):
        assert x.tobytes() == y.tobytes()


def two_instance_scene(ctx, model):
    xf = np.eye(3, 4, dtype=np.float32)
    xf[:, 3] = (-70.0, -70.0, -70.0)
    scene = api.Scene(ctx)
    scene.add_instance(model, xf.reshape(12))
    scene.add_instance(model, ROTATED.reshape(12))
    scene.commit()
    return scene


def test_pick_carve_commit_query_round_trip():
    pal = synth.make_palette(5)
    ctx = api.Context(device=0)
    vox = start_voxels(np.random.default_rng(35), 9000)
    model = api.Model(ctx, *host_model(vox, pal), pal)
    scene = two_instance_scene(ctx, model)
    origin, direction = np.float32([[-22.3, 60.0, -21.7]]), np.float32([[0.0, -1.0, 0.0]])    # down onto the slab of instance 0
    hit = scene.trace_rays(origin, direction)[0]
    assert hit["instance"] == 0 and vox[tuple(int(t) for t in hit["xyz"])] == hit["palette"]
    centre = hit["xyz"].astype(np.float32) + np.float32(0.5)
    radius = 3.0
    lo, hi = centre - np.float32(radius), centre + np.float32(radius)      # the sphere's bounds in tree coordinates, exact
    corners = np.stack([lo, hi])
    world0 = corners + np.float32(-70.0)
    world1 = np.stack([corners[:, 2] + 40.0, corners[:, 1] - 60.0, 90.0 - corners[:, 0]], axis=1)
    q_lo = np.stack([world0.min(0), world1.min(0)]).astype(np.float32)
    q_hi = np.stack([world0.max(0), world1.max(0)]).astype(np.float32)
    before, _ = scene.overlap_boxes(q_lo, q_hi, capacity=0)
    crater = api.edit_shapes(L.SHAPE_SPHERE, centre, radius=radius)
    want, want_changed = W.apply(vox, crater)
    changed = model.edit_shapes(crater)
    assert changed.tolist() == want_changed.tolist() and changed[0] >= 1
    with pytest.raises(L.DustError) as e:      # the scene holds the model as it was: it must be committed again
        scene.trace_rays(origin, direction)
    assert e.value.status == L.ERR_NOT_READY
    with pytest.raises(L.DustError) as e:
        scene.overlap_boxes(q_lo, q_hi, capacity=0)
    assert e.value.status == L.ERR_NOT_READY
    scene.commit()
    after_hit = scene.trace_rays(origin, direction)[0]
    assert after_hit["instance"] == L.NO_HIT or after_hit["t"] > hit["t"]
    if after_hit["instance"] != L.NO_HIT:
        assert tuple(int(t) for t in after_hit["xyz"]) in want
    after, _ = scene.overlap_boxes(q_lo, q_hi, capacity=0)
    assert (before.astype(np.int64) - after.astype(np.int64)).tolist() == [int(changed[0])] * 2    # the model is shared: both instances lost them


def test_frames_after_shape_edits_equal_frames_of_a_rebuilt_model():
    rng = np.random.default_rng(36)
    pal = synth.make_palette(6)
    ctx = api.Context(device=0)
    vox = start_voxels(rng, 9000)
    edited = api.Model(ctx, *host_model(vox, pal), pal)
    scene = two_instance_scene(ctx, edited)
    n0, n5 = synth.stbn_scalar(layers=4), synth.stbn_unitvec3_cosine(layers=4)
    cam, sky = P.camera_for((150.0, 120.0, 160.0)), P.sky_state()
    passes = L.PASS_PRIMARY | L.PASS_AMBIENT_OCCLUSION | L.PASS_FINAL_GATHER | L.PASS_SURFEL | L.PASS_GI_ORDERED

    def frames(sc):
        pipe = api.StandardPipeline(ctx, 320, 200)
        pipe.set_noise(0, n0)
        pipe.set_noise(5, n5)
        pipe.configure_gi(1 << 16, 8192)
        for f in (1, 2, 3):
            pipe.render(sc, cam, sky, passes, frame_index=f, rand=synth.frame_rand(3, f))
        h, sp = pipe.read_gi()
        return P.read_hip_gbuffer(pipe), h, sp.view(np.uint32).copy()

    frames(scene)
    shapes = np.concatenate([random_shapes(rng, k, 30, 15.0, 125.0, 20.0) for k in (BOX, SPHERE, CAPSULE)])
    shapes = shapes[rng.permutation(len(shapes))]
    vox, want_changed = W.apply(vox, shapes)
    assert edited.edit_shapes(shapes).tolist() == want_changed.tolist()
    with pytest.raises(L.DustError) as e:  # bounds and the staged root may have changed: the scene must be committed again
        frames(scene)
    assert e.value.status == L.ERR_NOT_READY
    scene.commit()
    got = frames(scene)
    fresh = api.Model(ctx, *host_model(vox, pal), pal)
    want = frames(two_instance_scene(ctx, fresh))
    for k in want[0]:
        assert want[0][k].tobytes() == got[0][k].tobytes(), k
    assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])
    assert np.isfinite(want[0]["depth"]).mean() > 0.05
