"""Model columns on the device (dust_hip_model_columns, dust_hip_model_columns_apply; the contract is in include/dust_hip.h). Every
comparison is exact: the result, the map and the table must be, byte for byte, what the witness says (tests/column_witness.py), an
apply must leave the model a host build of the witness's grid, and a columns call must leave the model as it found it."""
import ctypes as C
import functools

import numpy as np
import pytest

import column_witness as W
import surface_witness as SW
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi

pytestmark = pytest.mark.gpu

ROTATED = np.array([[0, 0, 1, 40], [0, 1, 0, -60], [-1, 0, 0, 90]], np.float32)
HIERARCHY = ("root", "host_root", "mid", "dense_mask", "bmin", "bmax")


def host_model(grid, pal):
    return api.flatten_model(to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


@functools.lru_cache(maxsize=None)
def hand_built_grid():
    """single voxels at the two corners of the tree; on each axis runs across the brick edge 3 | 4 and the root-cell edges 15 | 16 and
    63 | 64, a full column 0..255 and an alternating column (128 runs); a 3-thick plate with a cavity; an overhang over a floor; a
    block of mixed materials across 15 | 16"""
    rng = np.random.default_rng(101)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[0, 0, 0], grid[255, 255, 255] = 1, 2
    for axis in range(3):
        for k, edge in enumerate((3, 15, 63)):
            at = [70 + 10 * axis + 3 * k] * 3                # away from the other pieces, a column of its own per run
            box = [slice(c, c + 1) for c in at]
            box[axis] = slice(edge - 1 - k, edge + 3)        # 2..5, 13..17, 60..65: each across its edge
            grid[tuple(box)] = 3 + axis + k
        full, alternating = [slice(200 + axis, 201 + axis)] * 3, [slice(210 + axis, 211 + axis)] * 3
        full[axis], alternating[axis] = slice(0, 256), slice(axis & 1, 256, 2)
        grid[tuple(full)], grid[tuple(alternating)] = 9 + axis, 12 + axis
    grid[120:150, 30:33, 120:150] = 8                        # the plate: 3 thick along y
    grid[123, 31, 124] = 0                                   # ... with a cavity in its middle layer
    grid[160:180, 10, 160:180] = 15                          # a floor
    grid[165:175, 20:22, 165:175] = 16                       # ... and an overhang above its middle
    grid[10:22, 10:22, 10:22] = np.where(rng.random((12,) * 3) < 0.8, rng.integers(1, 7, (12,) * 3), 0)
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def six_material_grid():
    """about 5 000 voxels of six materials in [0, 64)^3: a sparse scatter and a dense block across 15 | 16 and 31 | 32 (the recipe of the
    census and surface tests)"""
    rng = np.random.default_rng(82)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[:64, :64, :64] = np.where(rng.random((64,) * 3) < 0.01, rng.integers(1, 7, (64,) * 3), 0)
    grid[13:27, 26:38, 14:20] = np.where(rng.random((14, 12, 6)) < 0.85, rng.integers(1, 7, (14, 12, 6)), 0)
    assert 3000 < np.count_nonzero(grid) < 6000
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def random_fill(density):
    """a fill of [0, 64)^3 and one of [112, 144)^3, across 127 | 128, three materials"""
    rng = np.random.default_rng(int(density * 1000))
    grid = np.zeros((256,) * 3, np.uint8)
    grid[:64, :64, :64] = np.where(rng.random((64,) * 3) < density, rng.integers(1, 4, (64,) * 3), 0)
    grid[112:144, 112:144, 112:144] = np.where(rng.random((32,) * 3) < density, rng.integers(1, 4, (32,) * 3), 0)
    grid.setflags(write=False)
    return grid


def check(model, grid, face, **query):
    """one query on the device and in the witness: result, map and table agree; returns them"""
    result, cells, counts = model.columns(face, tables=True, **query)
    want_result, want_cells, want_counts = W.columns(grid, face, **query)
    assert result.dtype == api.COLUMNS_RESULT_DTYPE and cells.dtype == api.COLUMN_CELL_DTYPE and counts.shape == (256,) and counts.dtype == np.uint32
    assert result.tobytes() == want_result.tobytes(), (face, query, result, want_result)
    assert cells.shape == want_cells.shape, (face, query, cells.shape, want_cells.shape)
    bad = np.argwhere(cells != want_cells)
    assert len(bad) == 0, (face, query, bad[:5], [(cells[tuple(b)], want_cells[tuple(b)]) for b in bad[:5]])
    assert cells.tobytes() == want_cells.tobytes()
    assert np.array_equal(counts, want_counts), (face, query, np.flatnonzero(counts != want_counts)[:5])
    assert int(counts.sum()) == int(result["columns"]) == cells.size and int(counts[0]) == int(result["columns"]) - int(result["hit"])
    # counts only, and without the table: the same result
    alone, none, no_counts = model.columns(face, cells=False, **query)
    assert alone.tobytes() == result.tobytes() and none is None and no_counts is None
    return result, cells, counts


def test_hand_built_grid():
    grid = hand_built_grid()
    pal = synth.make_palette(61)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for d, face in enumerate(W.FACES):
        axis = d >> 1
        top, cells, counts = check(model, grid, face)
        assert int(cells["runs"].max()) == 128 and int(top["columns"]) == 65536
        for layer in (1, 2, 127, 128):                       # 128: one past the deepest
            result, _, layer_counts = check(model, grid, face, layer=layer)
            assert (int(result["hit"]) == 0) == (layer == 128) and (layer < 128 or int(layer_counts[0]) == 65536)
        u, v = 200 + axis, 200 + axis                        # the full column: one run of 256
        assert cells[v, u].tolist() == (255 if d & 1 else 0, 8 + axis, 255, 1)
        end = [200 + axis] * 3                               # ... whose near end is the nearest voxel of the high sides; of the low sides, the corner
        end[axis] = 255
        assert int(top["nearest_key"]) == ((end[0] << 16) | (end[1] << 8) | end[2] if d & 1 else 0)
    # from above: the plate's top, the cavity's floor behind it; the overhang, then the floor under it
    _, cells, _ = check(model, grid, L.FACE_POS_Y)
    assert cells[123, 124].tolist() == (32, 7, 0, 2) and cells[130, 130].tolist() == (32, 7, 2, 1)
    assert cells[170, 170].tolist() == (21, 15, 1, 2) and cells[162, 162].tolist() == (10, 14, 0, 1)
    _, second, _ = check(model, grid, L.FACE_POS_Y, layer=1)
    assert second[123, 124].tolist() == (30, 7, 0, 2) and second[170, 170].tolist() == (10, 14, 0, 2) and second[162, 162].tolist() == (0, 255, 0, 1)
    # ... and from below the floor hides the overhang
    _, cells, _ = check(model, grid, L.FACE_NEG_Y)
    assert cells[170, 170].tolist() == (10, 14, 0, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def test_regions():
    grid = hand_built_grid()
    pal = synth.make_palette(62)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    # the full y column cut at its near and at its far face; the same through the x and z columns
    for d, face in enumerate(W.FACES):
        axis = d >> 1
        lo, hi = [198] * 3, [204] * 3
        lo[axis], hi[axis] = 50, 100
        result, cells, _ = check(model, grid, face, region=(tuple(lo), tuple(hi)))
        assert cells[2 + axis, 2 + axis].tolist() == (100 if d & 1 else 50, 8 + axis, 50, 1) and int(result["hit"]) == 1 and int(result["depth_sum"]) == 0
        lo[axis], hi[axis] = 77, 77                              # a single slice along the axis
        check(model, grid, face, region=(tuple(lo), tuple(hi)))
        check(model, grid, face, region=((9, 11, 10), (22, 21, 19)), layer=d % 3)      # aligned to bricks on no axis, through the mixed block
        check(model, grid, face, region=((13, 13, 13), (13, 13, 13)))                  # a single voxel
        single_lo, single_hi = [14, 15, 16], [14, 15, 16]
        single_lo[axis], single_hi[axis] = 0, 255                                      # a single column: lo == hi on u and on v
        result, cells, _ = check(model, grid, face, region=(tuple(single_lo), tuple(single_hi)), layer=1)
        assert cells.shape == (1, 1) and int(result["columns"]) == 1
        check(model, grid, face, region=((0, 0, 0), (255, 255, 255)), palette=7)       # the plate alone, everything else see-through
    # lo > hi: the zero result, bounds 255 / 0, the cells and the table's words as the call would leave an empty region
    zero = W.zero_result()
    for region in (((9, 9, 9), (8, 200, 200)), ((0, 0, 300), (255, 255, 400))):
        q = model._columns_query(L.FACE_POS_Y, -1, region, 0)
        result = np.full(64, 0x5A, np.uint8).view(api.COLUMNS_RESULT_DTYPE)
        cells = np.full(64, 0x5A, np.uint8).view(api.COLUMN_CELL_DTYPE)
        counts = np.full(256, 0x5A5A5A5A, np.uint32)
        assert lib.dust_hip_model_columns(model._h, C.byref(q), result.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p), 16,
                                          counts.ctypes.data_as(C.c_void_p)) == L.OK
        assert result[0].tobytes() == zero.tobytes() and cells.tobytes() == b"\x5a" * 64 and not counts.any()
        assert result[0]["lo"].tolist() == [255] * 3 and result[0]["hi"].tolist() == [0] * 3
        got, none, table = model.columns(L.FACE_POS_Y, region=region, tables=True)
        assert got.tobytes() == zero.tobytes() and none.shape == (0, 0) and not table.any()
    # a capacity one short is refused and nothing is written; the exact capacity is enough
    region = ((10, 0, 10), (14, 255, 16))                                              # 5 x 7 columns from above
    q = model._columns_query(L.FACE_POS_Y, -1, region, 0)
    want_result, want_cells, _ = W.columns(grid, W.POS_Y, region=region)
    for capacity in (34, 0, 35, 40):
        result = np.full(64, 0x5A, np.uint8).view(api.COLUMNS_RESULT_DTYPE)
        cells = np.full(40 * 4, 0x5A, np.uint8).view(api.COLUMN_CELL_DTYPE)
        status = lib.dust_hip_model_columns(model._h, C.byref(q), result.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p), capacity, None)
        if capacity < 35:
            assert status == L.ERR_INVALID_ARGUMENT and result.tobytes() == b"\x5a" * 64 and cells.tobytes() == b"\x5a" * 160, capacity
        else:
            assert status == L.OK and result[0].tobytes() == want_result.tobytes(), capacity
            assert cells[:35].tobytes() == want_cells.tobytes() and cells[35:].tobytes() == b"\x5a" * 20, capacity
    assert lib.dust_hip_model_columns(model._h, C.byref(q), None, None, 0, None) == L.OK                    # every output may be null


def test_palette_filter():
    grid = six_material_grid()
    pal = synth.make_palette(63)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    whole, _, _ = check(model, grid, L.FACE_POS_Y)
    hits = 0
    for k, palette in enumerate((0, 3, 5, 200)):
        for face in (W.FACES[k], W.FACES[k + 2]):
            for layer in (0, 1):
                result, cells, counts = check(model, grid, face, palette=palette, layer=layer)
                assert set(np.unique(cells["palette"]).tolist()) <= {palette, 255} and not np.delete(counts, [0, 1 + palette]).any()
                assert int(counts[1 + palette]) == int(result["hit"]) and (palette != 200 or int(result["runs"]) == 0)
                hits += int(result["hit"])
        check(model, grid, L.FACE_NEG_Z, palette=palette, region=((14, 27, 15), (25, 36, 18)), layer=1)
    assert hits > 1000 and int(whole["hit"]) > 1000
    # a voxel of another material between two of the filter's splits nothing and joins nothing: it is a gap like air
    probe = np.zeros((256,) * 3, np.uint8)
    probe[40, 10:20, 40] = [2, 2, 5, 2, 0, 2, 5, 5, 2, 2]
    model = make(ctx, probe, pal)
    _, cells, _ = check(model, probe, L.FACE_NEG_Y, palette=1, layer=1)
    assert cells[40, 40].tolist() == (13, 1, 0, 4)
    _, cells, _ = check(model, probe, L.FACE_NEG_Y, layer=1)
    assert cells[40, 40].tolist() == (15, 1, 4, 2)


@pytest.mark.parametrize("density", [0.02, 0.5])
def test_random_fills(density):
    grid = random_fill(density)
    pal = synth.make_palette(64)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    hits = 0
    for face in W.FACES:
        for layer in (0, 3):
            result, _, _ = check(model, grid, face, layer=layer)
            hits += int(result["hit"])
            check(model, grid, face, layer=layer, region=((0, 0, 0), (63, 63, 63)))
            check(model, grid, face, layer=layer, region=((113, 120, 126), (142, 129, 140)), palette=(-1, 1)[layer & 1])
    assert hits > 5000


def ray_grid(n=8):
    """n * n rays along -x over the image of [0, 64)^3 under ROTATED"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n, dtype=np.float32), np.linspace(0.0, 1.0, n, dtype=np.float32))
    origins = np.stack([np.full(u.size, 300.0, np.float32), -55.0 + 60.0 * u.reshape(-1), 30.0 + 60.0 * v.reshape(-1)], axis=1)
    return origins, np.tile(np.float32([-1.0, 0.01, 0.02]), (u.size, 1))


def test_the_model_is_only_read():
    grid = six_material_grid()
    pal = synth.make_palette(65)
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
    check(fixed, grid, L.FACE_POS_Y, region=region)
    check(fixed, grid, L.FACE_NEG_X, palette=2, layer=1)
    fixed.columns(L.FACE_POS_Z, cells=False)                                      # (masks only: no grid is made)
    assert [a.tobytes() for a in fixed.read()] == source_bytes
    assert scene.trace_rays(origins, directions).tobytes() == hits.tobytes()      # no commit: the generation has not moved
    fixed.find_islands(L.ISLANDS_FACES, capacity=0)                               # the first-edit transition happens HERE, not in columns
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
    first = check(loose, edited, L.FACE_POS_Y)
    second = check(loose, edited, L.FACE_POS_Y)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))         # two calls, the same bytes
    check(loose, edited, L.FACE_NEG_Z, palette=5, layer=1)
    assert loose.island_of(points).tolist() == keys.tolist() and loose.distance_at(points).tolist() == values.tolist()
    assert loose.flood_at(points).tolist() == steps.tolist()
    assert scene2.trace_rays(origins, directions).tobytes() == hits2.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(loose.read(), host_model(edited, pal)))

    # columns_apply is an edit: the labelling and both fields are gone, and the scene needs a commit
    assert loose.columns_apply(3, L.FACE_POS_Z, region=region) > 0
    assert status_of(lambda: loose.island_of(points)) == L.ERR_NOT_READY and status_of(lambda: loose.distance_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: loose.flood_at(points)) == L.ERR_NOT_READY
    assert status_of(lambda: scene2.trace_rays(origins, directions)) == L.ERR_NOT_READY
    scene2.commit()
    assert len(scene2.trace_rays(origins, directions)) == len(hits2)


APPLIES = [  # (value, face, where, depth, palette, region, layer)
    (29, W.POS_Y, W.RUN, 1, -1, None, 0),                                         # grass on every top voxel
    (30, W.POS_Y, W.RUN, 3, 7, None, 0),                                          # three deep, under a filter: the plate through and through
    (-1, W.POS_Y, W.RUN, 256, -1, None, 0),                                       # peel the top layer off
    (-1, W.NEG_X, W.RUN, 256, -1, None, 1),                                       # ... the second one from the -x side
    (17, W.POS_Y, W.GAP, 1, -1, None, 0),                                         # snow under open sky
    (18, W.POS_Y, W.GAP, 256, -1, ((100, 0, 100), (190, 40, 190)), 1),            # fill under the plate's cavity roof and under the overhang
    (19, W.NEG_X, W.GAP, 256, -1, ((5, 5, 5), (60, 60, 60)), 0),                  # from -x up to the mixed block
    (-1, W.NEG_X, W.GAP, 1, 2, ((5, 5, 5), (60, 60, 60)), 1),                     # one voxel in front of a filter's second run: may clear other materials
    (3, W.NEG_X, W.RUN, 3, 3, None, 0),                                           # a filter's own index: nothing changes
    (-1, W.POS_Y, W.GAP, 256, -1, None, 0),                                       # clearing air: nothing changes
]


@pytest.mark.parametrize("case", range(len(APPLIES)))
def test_columns_apply(case):
    grid = hand_built_grid()
    pal = synth.make_palette(66)
    ctx = api.Context(device=0)
    value, face, where, depth, palette, region, layer = APPLIES[case]
    model = make(ctx, grid, pal)
    hit = int(model.columns(face, palette=palette, region=region, layer=layer, cells=False)[0]["hit"])
    changed = model.columns_apply(value, face, where=where, depth=depth, palette=palette, region=region, layer=layer)
    after, want_changed = W.apply(grid, value, face, where, depth, palette, region, layer)
    assert changed == want_changed and hit > 0 and (changed > 0) == (case < 8)
    fresh = make(ctx, after, pal)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), fresh.read()))
    got, want = model.read_hierarchy(), fresh.read_hierarchy()
    assert got["n_mid"] == want["n_mid"] and got["extent_log2"] == want["extent_log2"]
    for name in HIERARCHY:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    check(model, after, face, palette=palette, region=region, layer=layer)
    if case == 0:                                                                  # grass over dirt: the second call sees the first one's grass as see-through
        assert np.count_nonzero(after == 30) == changed and after[130, 32, 130] == 30 and after[130, 31, 130] == 8 and after[170, 21, 170] == 30
        assert model.columns_apply(20, W.POS_Y, depth=4, palette=7) == W.apply(after, 20, W.POS_Y, W.RUN, 4, 7)[1] > 0
        assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(W.apply(after, 20, W.POS_Y, W.RUN, 4, 7)[0], pal)))
    if case == 4:                                                                  # snow lies on the overhang and round it on the floor, not under it
        assert after[170, 22, 170] == 18 and after[170, 11, 170] == 0 and after[162, 11, 162] == 18 and after[123, 33, 124] == 18 and after[123, 31, 124] == 0
    if case == 5:                                                                  # ... and the water of case 5 is exactly what the snow cannot reach
        assert after[170, 11, 170] == after[170, 19, 170] == 19 and after[123, 31, 124] == 19 and after[162, 11, 162] == 0


def test_runs_are_the_exposed_faces_and_refusals():
    grid = six_material_grid()
    pal = synth.make_palette(67)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    surface = model.surface(capacity=0)[0]
    exposed = SW.exposure(grid)
    for d, face in enumerate(W.FACES):
        runs = int(model.columns(face, cells=False)[0]["runs"])
        assert runs == int(surface["by_face"][d]) == int(model.surface(faces=face, capacity=0)[0]["by_face"][d]) == np.count_nonzero(exposed & (1 << d)) > 1000

    result = np.full(64, 0x5A, np.uint8).view(api.COLUMNS_RESULT_DTYPE)
    cells = np.full(65536 * 4, 0x5A, np.uint8).view(api.COLUMN_CELL_DTYPE)
    counts = np.full(256, 0x5A5A5A5A, np.uint32)
    changed = C.c_uint32(0x5A5A5A5A)
    rp, vp, cp = (a.ctypes.data_as(C.c_void_p) for a in (result, cells, counts))

    def query(face=L.FACE_POS_Y, flags=0, palette=-1, layer=0, reserved=0, size=C.sizeof(L.ColumnsQuery)):
        q = L.ColumnsQuery(struct_size=size, face=face, flags=flags, palette=palette, layer=layer, reserved=reserved)
        q.hi[:] = [255, 255, 255]
        return q
    bad = [query(face=0), query(face=3), query(face=64), query(face=1 << 31), query(flags=1), query(flags=1 << 31), query(reserved=1), query(palette=-2),
           query(palette=255), query(layer=256), query(size=47), query(size=0)]
    for q in bad:
        assert lib.dust_hip_model_columns(model._h, C.byref(q), rp, vp, 65536, cp) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_columns_apply(model._h, C.byref(q), L.COLUMNS_RUN, 1, 3, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    good = query()
    assert lib.dust_hip_model_columns(model._h, None, rp, vp, 65536, cp) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_columns(model._h, C.byref(good), rp, vp, 65535, cp) == L.ERR_INVALID_ARGUMENT
    for where, depth, value in ((2, 1, 3), (0, 0, 3), (0, 257, 3), (1, 1, 255), (1, 1, -2)):
        assert lib.dust_hip_model_columns_apply(model._h, C.byref(good), where, depth, value, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_columns_apply(model._h, None, 0, 1, 3, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert result.tobytes() == b"\x5a" * 64 and cells.tobytes() == b"\x5a" * (65536 * 4) and np.all(counts == 0x5A5A5A5A) and changed.value == 0x5A5A5A5A
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))      # no refused apply touched the model
    # a larger struct_size is a newer caller's; an apply on an empty region is legal and changes nothing
    assert lib.dust_hip_model_columns(model._h, C.byref(query(size=64)), None, None, 0, None) == L.OK
    empty = query()
    empty.lo[0], empty.hi[0] = 3, 2
    assert lib.dust_hip_model_columns_apply(model._h, C.byref(empty), L.COLUMNS_GAP, 256, -1, C.byref(changed)) == L.OK and changed.value == 0
    # unsupported exactly where set_voxels is, before the query is looked at
    blocks, mats = synth.procedural_deep_blocks(occupancy=2e-6, sample=True)
    deep = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    assert status_of(lambda: deep.columns(L.FACE_POS_Y)) == L.ERR_UNSUPPORTED and status_of(lambda: deep.columns_apply(-1, L.FACE_POS_Y)) == L.ERR_UNSUPPORTED
    assert lib.dust_hip_model_columns(deep._h, C.byref(bad[0]), rp, vp, 65536, cp) == L.ERR_UNSUPPORTED
