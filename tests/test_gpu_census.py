"""Model censuses on the device (dust_hip_model_census; the contract is in include/dust_hip.h). Every comparison is exact: the records
and the per-material rows must be, byte for byte, what the witness counts (tests/census_witness.py, on top of the shape edits'
witness), the counts must be the ones the edit of the same shapes reports, and the model must come out of the call as it went in."""
import ctypes as C
import functools

import numpy as np
import pytest

import census_witness as W
import shape_edit_witness as SW
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi
from shape_edit_witness import BOX, CAPSULE, SPHERE

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
WHOLE = SW.shape(BOX, (0.0, 0.0, 0.0), (256.0, 256.0, 256.0))


def host_model(grid, pal):
    return api.flatten_model(to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


@functools.lru_cache(maxsize=None)
def every_material_grid():
    """about 2 000 voxels holding all 255 palette indices: a block across the brick edge 11 | 12 and the root-cell edge 15 | 16 on every
    axis, the two corners of the tree (faces 0 and 255), and a plate with each index once"""
    rng = np.random.default_rng(81)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[10:22, 10:22, 10:22] = np.where(rng.random((12,) * 3) < 0.7, rng.integers(1, 256, (12,) * 3), 0)
    grid[0:6, 0:6, 0:6] = np.where(rng.random((6,) * 3) < 0.7, rng.integers(1, 256, (6,) * 3), 0)
    grid[250:, 250:, 250:] = np.where(rng.random((6,) * 3) < 0.7, rng.integers(1, 256, (6,) * 3), 0)
    grid[40:56, 40:56, 47] = (np.arange(256) % 255 + 1).reshape(16, 16)
    grid[4:8, 8:12, 12:16] = 3      # one brick exactly, of one material
    assert set(np.unique(grid).tolist()) == set(range(256)) and 1500 < np.count_nonzero(grid) < 5000
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def six_material_grid():
    """about 5 000 voxels of six materials in [0, 64)^3: a sparse scatter and a dense block across 15 | 16 and 31 | 32"""
    rng = np.random.default_rng(82)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[:64, :64, :64] = np.where(rng.random((64,) * 3) < 0.01, rng.integers(1, 7, (64,) * 3), 0)
    grid[13:27, 26:38, 14:20] = np.where(rng.random((14, 12, 6)) < 0.85, rng.integers(1, 7, (14, 12, 6)), 0)
    assert 3000 < np.count_nonzero(grid) < 6000
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def whole_tree_answer():
    """the witness's record and row of the whole-tree box over every_material_grid()"""
    return W.census_one(every_material_grid(), WHOLE)


def check(model, grid, shapes, tables=True):
    """one call on the device and in the witness: every record and every row agree; returns them"""
    records, counts = model.census(shapes, tables=tables)
    want_records, want_counts = W.census(grid, shapes, tables=tables)
    assert records.dtype == api.CENSUS_DTYPE and len(records) == len(shapes)
    for i in range(len(shapes)):
        assert records[i].tobytes() == want_records[i].tobytes(), (i, shapes[i], records[i], want_records[i])
    if tables:
        assert counts.shape == (len(shapes), 256) and counts.dtype == np.uint32
        bad = np.argwhere(counts != want_counts)
        assert len(bad) == 0, (bad[:5], counts[tuple(bad[0])], want_counts[tuple(bad[0])])
        assert np.array_equal(counts.sum(axis=1), records["covered"]) and np.array_equal(counts[:, 1:].sum(axis=1), records["solid"])
    else:
        assert counts is None
    return records, counts


def random_shapes(rng, n, lo, hi, size):
    a = rng.uniform(lo, hi, (n, 3))
    kind = rng.integers(0, 3, n)
    b = a + np.where((kind == BOX)[:, None], rng.uniform(0.0, size, (n, 3)), rng.uniform(-size, size, (n, 3)))
    return SW.shapes(*[SW.shape(int(k), p, q, radius=float(r), op=int(op), palette=int(pal)) for k, p, q, r, op, pal in
                       zip(kind, a, b, rng.uniform(0.0, size / 2, n), rng.integers(0, 4, n), rng.integers(0, 255, n))])


def test_hand_built_shapes_records_and_tables():
    grid = every_material_grid()
    pal = synth.make_palette(41)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    nan = float("nan")
    shapes = SW.shapes(
        SW.shape(BOX, (13.0, 14.0, 15.0), (14.0, 15.0, 16.0)),                                  # one voxel
        SW.shape(BOX, (4.0, 8.0, 12.0), (8.0, 12.0, 16.0)),                                     # one brick exactly
        SW.shape(BOX, (12.0, 13.0, 14.0), (19.0, 18.0, 17.0)),                                  # across 15 | 16 on all three axes
        SW.shape(CAPSULE, (9.0, 10.0, 11.0), (52.0, 50.0, 47.5), radius=2.5),                   # a diagonal through three root cells
        SW.shape(SPHERE, (-2.0, 3.0, 2.5), radius=6.0),                                         # partly outside: a negative centre
        SW.shape(SPHERE, (258.0, 253.0, 252.5), radius=7.0),                                    # ... and one beyond 256
        SW.shape(BOX, (300.0, 10.0, 10.0), (310.0, 20.0, 20.0)),                                # wholly outside
        SW.shape(SPHERE, (nan, 10.0, 10.0), radius=3.0),
        SW.shape(BOX, (15.0, 10.0, 10.0), (14.0, 20.0, 20.0)),                                  # a > b
        SW.shape(BOX, (40.0, 40.0, 47.0), (56.0, 56.0, 48.0)))                                  # the plate: every index once (palette 0 twice)
    check(model, grid, shapes)
    shapes = np.concatenate([shapes, SW.shapes(WHOLE)])      # the whole-tree box: the witness's answer is shared with test_chunks_and_limits
    records, counts = model.census(shapes)
    assert records[:10].tobytes() == W.census(grid, shapes[:10])[0].tobytes()
    assert [int(v) for v in records["covered"][:3]] == [1, 64, 7 * 5 * 3] and int(records["solid"][1]) == 64 and int(counts[1, 3]) == 64
    for i in (6, 7, 8):
        assert records[i].tobytes() == W.zero_record().tobytes() and not counts[i].any()
    assert np.count_nonzero(counts[9]) == 255 and int(records["covered"][10]) == 1 << 24 and int(records["solid"][10]) == np.count_nonzero(grid)
    assert int(records["solid"][3]) > 0 and int(records["solid"][4]) > 0 and int(records["solid"][5]) > 0
    assert records[10].tobytes() == whole_tree_answer()[0].tobytes() and np.array_equal(counts[10], whole_tree_answer()[1])
    # records alone say the same
    alone, none = model.census(shapes, tables=False)
    assert alone.tobytes() == records.tobytes() and none is None


def test_random_shapes_against_the_witness():
    grid = six_material_grid()
    pal = synth.make_palette(42)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    shapes = random_shapes(np.random.default_rng(83), 200, -4.0, 68.0, 16.0)
    assert {int(k) for k in shapes["kind"]} == {BOX, SPHERE, CAPSULE}
    records, counts = check(model, grid, shapes)
    assert np.count_nonzero(records["solid"]) > 100 and np.count_nonzero(counts[:, 1:7].all(axis=1)) > 10 and not counts[:, 7:].any()


def test_ties_to_the_edit():
    grid = six_material_grid()
    pal = synth.make_palette(43)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    rng = np.random.default_rng(84)
    centres = np.array([(16 + 32 * i, 16 + 32 * j, 16 + 32 * k) for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64) + rng.uniform(-3, 3, (8, 3))
    kinds = [BOX, SPHERE, CAPSULE, BOX, SPHERE, CAPSULE, SPHERE, CAPSULE]
    shapes = SW.shapes(*[SW.shape(k, c - (5.0 if k != SPHERE else 0.0), c + 5.0, radius=(0.0 if k == BOX else 9.0 if k == SPHERE else 4.0))
                         for k, c in zip(kinds, centres)])      # each within 12 voxels of its centre: pairwise disjoint
    covered = [SW.covered_voxels(s) for s in shapes]
    assert all(covered[i].isdisjoint(covered[j]) for i in range(8) for j in range(i)) and all(len(c) > 100 for c in covered)
    records, counts = check(model, grid, shapes)
    assert np.all(records["solid"] > 0) and np.all(counts[:, 0] > 0)
    carve, place = shapes.copy(), shapes.copy()
    carve["op"], place["op"], place["palette"] = SW.CARVE, SW.PLACE, 9
    carved, placed = make(ctx, grid, pal), make(ctx, grid, pal)
    assert carved.edit_shapes(carve).tolist() == records["solid"].tolist()
    assert placed.edit_shapes(place).tolist() == counts[:, 0].tolist()
    after, after_counts = carved.census(shapes)
    assert not after["solid"].any() and after["covered"].tolist() == records["covered"].tolist()
    assert np.all(after["lo"] == 255) and np.all(after["hi"] == 0) and not after["sum"].any()
    assert after_counts[:, 0].tolist() == records["covered"].tolist() and not after_counts[:, 1:].any()
    full, full_counts = placed.census(shapes)
    assert full["solid"].tolist() == records["covered"].tolist() and full_counts[:, 10].tolist() == (counts[:, 0] + counts[:, 10]).tolist()
    # the model the census ran on is as it was
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def test_crowded_cell():
    grid = every_material_grid()
    pal = synth.make_palette(44)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    rng = np.random.default_rng(85)
    crowd = random_shapes(rng, 70, 17.0, 24.0, 9.0)      # every one's bounds reach root cell (1, 1, 1): voxels 16..31 on each axis
    same = SW.shapes(*[SW.shape(SPHERE, (16.5, 15.5, 16.0), radius=5.5)] * 5)
    shapes = np.concatenate([crowd[:30], same[:2], crowd[30:], same[2:]])
    assert len({s.tobytes() for s in crowd}) == 70
    assert all(np.all(np.minimum(s["a"], s["b"]) < 32.0) and np.all(np.maximum(s["a"], s["b"]) >= 16.0) for s in crowd)
    records, counts = check(model, grid, shapes)
    five = [30, 31, 72, 73, 74]
    assert len({records[i].tobytes() for i in five}) == 1 and len({counts[i].tobytes() for i in five}) == 1 and int(records["solid"][30]) > 100
    assert np.count_nonzero(records["solid"]) > 40 and np.count_nonzero(records["covered"]) > 60


def ray_grid(n=8):
    """n * n rays along -x over the image of [0, 64)^3 under ROTATED"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def test_the_model_is_only_read():
    grid = six_material_grid()
    pal = synth.make_palette(45)
    ctx = api.Context(device=0)
    shapes = random_shapes(np.random.default_rng(86), 24, 0.0, 64.0, 20.0)
    origins, directions = ray_grid()
    points = [(13, 26, 14), (20, 30, 16), (200, 200, 200)]

    # a model that was never edited stays as it was created, and a scene committed on it keeps answering
    fixed = make(ctx, grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(fixed, ROTATED.reshape(12))
    scene.commit()
    hits = scene.trace_rays(origins, directions)
    assert np.count_nonzero(hits["instance"] != L.NO_HIT) > 5
    source_bytes = [a.tobytes() for a in fixed.read()]
    records, counts = check(fixed, grid, shapes)
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit: the generation has not moved
    fixed.find_islands(L.ISLANDS_FACES, capacity=0)                               # the first-edit transition happens HERE, not in census
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY

    # an editable model is read in place, edits included; its labelling and both fields stand
    loose = make(ctx, grid, pal)
    loose.set_voxels([(20, 30, 16), (21, 30, 16), (60, 60, 60)], [5, -1, 0])
    edited = grid.copy()
    edited[20, 30, 16], edited[21, 30, 16], edited[60, 60, 60] = 6, 0, 1
    loose.find_islands(L.ISLANDS_FACES, capacity=0)
    loose.distance(max_radius=3)
    loose.flood([(100, 100, 100)], max_steps=90)
    keys, values, steps = loose.island_of(points), loose.distance_at(points), loose.flood_at(points)
    scene2 = api.Scene(ctx)
    scene2.add_instance(loose, ROTATED.reshape(12))
    scene2.commit()
    hits2 = scene2.trace_rays(origins, directions)
    both = np.concatenate([shapes, SW.shapes(SW.shape(BOX, (20.0, 30.0, 16.0), (22.0, 31.0, 17.0)), SW.shape(SPHERE, (60.5, 60.5, 60.5), radius=0.0))])
    records2, counts2 = check(loose, edited, both)
    assert (int(records2["solid"][-2]), int(counts2[-2, 6]), int(counts2[-2, 0]), int(counts2[-1, 1])) == (1, 1, 1, 1)
    assert loose.island_of(points).tolist() == keys.tolist() and loose.distance_at(points).tolist() == values.tolist()
    assert loose.flood_at(points).tolist() == steps.tolist()
    assert scene2.trace_rays(origins, directions).tobytes() == hits2.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(loose.read(), host_model(edited, pal)))


def test_chunks_and_limits():
    grid = every_material_grid()
    pal = synth.make_palette(46)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    record, row = whole_tree_answer()
    # 513 whole-tree boxes are 513 * 4096 cell entries: one more than a launch carries
    many = SW.shapes(*[WHOLE] * 513)
    records, counts = model.census(many)
    assert records.tobytes() == record.tobytes() * 513 and counts.tobytes() == row.tobytes() * 513
    # 65 536 one-voxel boxes, records only: half of them on solid voxels
    rng = np.random.default_rng(87)
    solid = np.argwhere(grid != 0)
    xyz = np.concatenate([solid[rng.integers(0, len(solid), 32768)], rng.integers(0, 256, (32768, 3))])
    xyz = xyz[rng.permutation(65536)]
    boxes = np.zeros(65536, SW.SHAPE_DTYPE)
    boxes["kind"], boxes["a"], boxes["b"] = BOX, xyz, xyz + 1
    records, none = model.census(boxes, tables=False)
    value = grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]]
    want = np.zeros(65536, W.RECORD_DTYPE)
    want["covered"], want["solid"] = 1, value != 0
    want["lo"], want["hi"] = np.where((value != 0)[:, None], xyz, 255), np.where((value != 0)[:, None], xyz, 0)
    want["sum"] = np.where((value != 0)[:, None], xyz, 0)
    assert none is None and records.tobytes() == want.tobytes() and 32768 <= np.count_nonzero(value) < 40000
    # the limits: 65 537 shapes, and 4 097 with tables, are refused with the outputs untouched; 4 097 without tables are counted
    out_records = np.full(4097 * 40, 0x5A, np.uint8).view(api.CENSUS_DTYPE)
    out_counts = np.full((4097, 256), 0x5A5A5A5A, np.uint32)
    before = out_records.tobytes(), out_counts.tobytes()
    rp, cp = out_records.ctypes.data_as(C.c_void_p), out_counts.ctypes.data_as(C.c_void_p)

    def call(shapes, n, records, counts):
        return lib.dust_hip_model_census(model._h, shapes.ctypes.data_as(C.c_void_p), n, records, counts)
    assert call(boxes, 4097, rp, cp) == L.ERR_INVALID_ARGUMENT and call(boxes, 4097, None, cp) == L.ERR_INVALID_ARGUMENT
    assert call(np.zeros(65537, SW.SHAPE_DTYPE), 65537, rp, None) == L.ERR_INVALID_ARGUMENT
    odd = boxes[:3].copy()
    odd["kind"][2] = 3
    assert call(odd, 3, rp, cp) == L.ERR_INVALID_ARGUMENT and lib.dust_hip_model_census(model._h, None, 3, rp, cp) == L.ERR_INVALID_ARGUMENT
    assert (out_records.tobytes(), out_counts.tobytes()) == before
    assert call(boxes, 4097, rp, None) == L.OK and out_records.tobytes() == want[:4097].tobytes() and out_counts.tobytes() == before[1]
    # only records, only counts, neither; op, palette and reserved are not looked at
    few = SW.shapes(WHOLE, SW.shape(BOX, (4.0, 8.0, 12.0), (8.0, 12.0, 16.0), op=77, palette=-3), SW.shape(SPHERE, (300.0, 0.0, 0.0), radius=2.0))
    few["reserved"] = 0xFFFFFFFF
    want_records, want_counts = W.census(grid, few[1:])
    want_records, want_counts = np.concatenate([np.array([record], W.RECORD_DTYPE), want_records]), np.concatenate([row[None, :], want_counts])
    out_records[:], out_counts[:] = np.zeros(1, api.CENSUS_DTYPE)[0], 0x5A5A5A5A
    assert call(few, 3, None, cp) == L.OK and np.array_equal(out_counts[:3], want_counts) and np.all(out_counts[3:] == 0x5A5A5A5A)
    assert not out_records.tobytes().strip(b"\0")
    assert call(few, 3, rp, None) == L.OK and out_records[:3].tobytes() == want_records.tobytes() and not out_records[3:].tobytes().strip(b"\0")
    assert call(few, 3, None, None) == L.OK and call(odd, 3, None, None) == L.ERR_INVALID_ARGUMENT
    assert call(few, 0, rp, cp) == L.OK and lib.dust_hip_model_census(model._h, None, 0, None, None) == L.OK
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def test_extremes():
    pal = synth.make_palette(47)
    ctx = api.Context(device=0)
    model = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    fill = SW.shapes(SW.shape(BOX, (-1e30,) * 3, (1e30,) * 3, op=SW.FILL, palette=254))
    assert model.edit_shapes(fill).tolist() == [1 << 24]
    records, counts = model.census(SW.shapes(WHOLE, SW.shape(BOX, (0.0, 0.0, 0.0), (256.0, 256.0, 1.0))))
    assert int(records["covered"][0]) == int(records["solid"][0]) == 1 << 24
    assert records["sum"][0].tolist() == [(1 << 24) * 255 // 2] * 3 and records["lo"][0].tolist() == [0] * 3 and records["hi"][0].tolist() == [255] * 3
    assert int(counts[0, 255]) == 1 << 24 and np.count_nonzero(counts[0]) == 1
    assert int(records["solid"][1]) == 1 << 16 and records["sum"][1].tolist() == [(1 << 16) * 255 // 2, (1 << 16) * 255 // 2, 0]
    assert records["hi"][1].tolist() == [255, 255, 0] and int(counts[1, 255]) == 1 << 16


def test_determinism_and_unsupported():
    grid = six_material_grid()
    pal = synth.make_palette(48)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    shapes = np.concatenate([random_shapes(np.random.default_rng(88), 150, -10.0, 80.0, 40.0), SW.shapes(WHOLE)])
    first, first_counts = model.census(shapes)
    second, second_counts = model.census(shapes)
    assert first.tobytes() == second.tobytes() and first_counts.tobytes() == second_counts.tobytes() and np.count_nonzero(first["solid"]) > 60
    # unsupported exactly where set_voxels is, before the shapes are looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    blocks, mats = host_model(grid, pal)
    mats = mats.copy()
    mats[0] = 255
    odd = api.Model(ctx, blocks, mats, pal)
    bad = shapes[:2].copy()
    bad["kind"][1] = 9
    for unsupported in (deep, odd):
        assert status_of(lambda: unsupported.census(shapes[:2])) == L.ERR_UNSUPPORTED
        assert status_of(lambda: unsupported.census(bad)) == L.ERR_UNSUPPORTED
    assert status_of(lambda: model.census(bad)) == L.ERR_INVALID_ARGUMENT
