"""Model fracture on the device (dust_hip_model_fracture / fracture_at / fracture_detach / fracture_apply; the contract is in
include/dust_hip.h). Every comparison is exact: the labels, the cell records and the result must be the witness's
(tests/fracture_witness.py: brute force over all seeds, no pruning), and a model that cells were detached from or that was applied to
must read back byte for byte what a host build of the witness's voxels uploads. The content sits at (9, 118, 201): it straddles brick
and root-cell boundaries on every axis."""
import ctypes as C

import numpy as np
import pytest

import fracture_witness as W
import island_witness as IW
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

ORIGIN = (9, 118, 201)


def host_model(grid, pal):
    """(blocks, materials) of a grid through the product's host flatten: what dust_hip_model_create is given for those voxels"""
    return api.flatten_model(W.to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def same_bytes(model, grid, pal):
    return all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), host_model(grid, pal)))


def same_hierarchy(model, grid, pal, ctx):
    """the upper levels, array for array, against a model created from the same voxels"""
    a, b = model.read_hierarchy(), make(ctx, grid, pal).read_hierarchy()
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("n_mid", "root", "host_root", "mid", "dense_mask", "bmin", "bmax"))


def status_of(call):
    with pytest.raises(L.DustError) as e:
        call()
    return e.value.status


def box_coordinates(lo, hi):
    return np.stack(np.meshgrid(*[np.arange(max(a, 0), min(b, 255) + 1) for a, b in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)


def around(grid, shell=5):
    """the coordinates of the content's bounding box and a shell around it"""
    xyz = np.argwhere(grid != 0)
    return box_coordinates(xyz.min(axis=0) - shell, xyz.max(axis=0) + shell)


def check(model, grid, seeds, want=None, **query):
    """one fracture against the witness: result, cells, and the labels over the content and a shell; returns the witness's labels"""
    r, cells = model.fracture(seeds, **query)
    lab, far = W.labels(grid, seeds, query.get("region"), query.get("palette"), query.get("scale", (1, 1, 1)), query.get("max_distance2"))
    xyz = around(grid)
    assert np.array_equal(model.fracture_at(xyz), W.at(lab, xyz))
    assert r.tobytes() == W.result(grid, lab, far, query.get("region"), query.get("palette"), len(seeds)).tobytes()
    assert cells.tobytes() == W.cells(lab, len(seeds)).tobytes()
    assert int(cells["voxels"].sum()) == int(r["labelled"]) and int(cells["cut_faces"].sum()) == 2 * int(r["cut_faces"])
    return lab, r, cells


def random_block(seed, size=(41, 37, 45), density=0.5, materials=4):
    rng = np.random.default_rng(seed)
    grid = np.zeros((256,) * 3, np.uint8)
    x, y, z = ORIGIN
    grid[x:x + size[0], y:y + size[1], z:z + size[2]] = np.where(rng.random(size) < density, rng.integers(1, materials + 1, size), 0)
    return rng, grid


def test_random_block_seeds_inside_outside_and_a_duplicate():
    rng, grid = random_block(1)
    pal = synth.make_palette(41)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    inside = rng.integers(0, 37, (7, 3)) + np.array(ORIGIN)
    seeds = np.concatenate([inside, [(-40, 130, 300), (300, -1024, 1279)], inside[2:3]])
    lab, r, cells = check(model, grid, seeds)
    assert int(r["solid"]) == int(r["labelled"]) == np.count_nonzero(grid) and int(r["cells"]) >= 7 and int(cells["voxels"][9]) == 0
    assert same_bytes(model, grid, pal)


def test_tie_lattice():
    grid = np.zeros((256,) * 3, np.uint8)
    x, y, z = ORIGIN
    grid[x:x + 24, y:y + 24, z:z + 24] = 3
    seeds = np.array([(x + 3 + 8 * i, y + 3 + 8 * j, z + 3 + 8 * k) for i in range(3) for j in range(3) for k in range(3)])   # spacing 8: planes at +7, +15
    pal = synth.make_palette(42)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for order in (np.arange(27), np.arange(27)[::-1], np.random.default_rng(2).permutation(27)):
        lab, r, cells = check(model, grid, seeds[order])
        tied = W.nearest([(x + 7, y + 7, z + 7), (x + 7, y + 7, z + 3), (x + 7, y + 3, z + 3)], seeds[order])[1]
        assert W.at(lab, [(x + 7, y + 7, z + 7)])[0] == tied[0] and int(r["cells"]) == 27 and int(r["cut_faces"]) > 0
        # the point equidistant from 8 seeds goes to the lowest index of the 8
        eight = [i for i, s in enumerate(seeds[order]) if all(abs(int(c) - o - 7) == 4 for c, o in zip(s, ORIGIN))]
        assert len(eight) == 8 and tied[0] == min(eight)


def test_a_full_candidate_list_of_duplicates():
    rng = np.random.default_rng(3)
    grid = np.zeros((256,) * 3, np.uint8)
    x, y, z = 10, 120, 203                                     # a 12^3 blob across root cells on every axis
    grid[x:x + 12, y:y + 12, z:z + 12] = np.where(rng.random((12, 12, 12)) < 0.8, 2, 0)
    positions = np.array([(x + dx, y + dy, z + dz) for dx in (1, 10) for dy in (1, 10) for dz in (1, 10)])
    seeds = positions[rng.integers(0, 8, L.MAX_FRACTURE_SEEDS)]
    pal = synth.make_palette(43)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    lab, r, cells = check(model, grid, seeds)
    firsts = sorted(int(np.flatnonzero((seeds == p).all(axis=1))[0]) for p in positions)
    assert int(r["cells"]) == 8 and np.flatnonzero(cells["voxels"]).tolist() == firsts


def test_region_filter_metric_and_limit_together():
    rng = np.random.default_rng(4)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[5:48, 112:140, 236:256] = np.where(rng.random((43, 28, 20)) < 0.7, rng.integers(1, 4, (43, 28, 20)), 0)     # reaches the tree's +z face
    region = ((11, 119, 250), (40, 130, 255))
    seeds = np.concatenate([rng.integers((8, 115, 245), (44, 135, 256), (9, 3)), [(20, 125, 270), (-5, 119, 252)]])
    pal = synth.make_palette(44)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    for limit in (None, 40, 0):
        for region_hi in (region[1], (40, 130, 4000)):         # a coordinate past 255 is cut back
            lab, r, cells = check(model, grid, seeds, region=(region[0], region_hi), palette=1, scale=(1, 16, 3), max_distance2=limit)
            inside = np.zeros(grid.shape, bool)
            inside[11:41, 119:131, 250:256] = True
            assert (lab[~inside] == W.NO_CELL).all() and (lab[grid != 2] == W.NO_CELL).all() and int(r["solid"]) == np.count_nonzero(inside & (grid == 2))
            assert (int(r["labelled"]) < int(r["solid"])) == (limit is not None) and (limit is None or int(r["max_d2"]) <= limit)
    assert int(check(model, grid, seeds, region=((30, 0, 0), (29, 255, 255)))[1]["solid"]) == 0        # the empty region
    assert same_bytes(model, grid, pal)


def test_a_model_that_is_not_editable_and_no_seeds():
    rng, grid = random_block(5, size=(20, 20, 20))
    pal = synth.make_palette(45)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    before = [a.tobytes() for a in model.read()]
    scene = api.Scene(ctx)
    scene.add_instance(model, np.eye(3, 4, dtype=np.float32).reshape(12))
    scene.commit()
    origins = np.float32([[15.0, 300.0, 210.0]])
    directions = np.float32([[0.0, -1.0, 0.0]])
    assert len(scene.trace_rays(origins, directions)) == 1
    lab, r, cells = check(model, grid, np.zeros((0, 3), np.int64))              # the call makes the model editable: flood's rule
    assert int(r["solid"]) == np.count_nonzero(grid) and int(r["labelled"]) == 0 and int(r["largest_cell"]) == 0xFFFFFFFF and len(cells) == 0
    assert [a.tobytes() for a in model.read()] == before and same_hierarchy(model, grid, pal, ctx)
    assert status_of(lambda: scene.trace_rays(origins, directions)) == L.ERR_NOT_READY     # the first call moved the arrays: commit again
    scene.commit()
    check(model, grid, [(15, 125, 210), (20, 130, 215)])
    assert len(scene.trace_rays(origins, directions)) == 1                      # on an editable model a fracture changes nothing a scene reads
    assert model.fracture([(15, 125, 210)], records=False) is None and model.fracture_at([(0, 0, 0)]).tolist() == [L.NO_CELL]


def test_detach_copies_carves_and_keeps_the_labelling():
    rng, grid = random_block(6, size=(30, 26, 33), density=0.7)
    pal = synth.make_palette(46)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    seeds = rng.integers(0, 26, (9, 3)) + np.array(ORIGIN)
    lab, r, cells = check(model, grid, seeds)
    xyz = around(grid)
    # a KEEP_SOURCE copy of two cells (each named twice: duplicates are legal) equals a model created from those voxels
    piece = model.fracture_detach([1, 4, 4, 1], keep_source=True)
    want_piece, want_rest, want_lab = W.detach(grid, lab, [1, 4])
    assert same_bytes(piece, want_piece, pal) and same_hierarchy(piece, want_piece, pal, ctx)
    assert same_bytes(model, grid, pal) and np.array_equal(model.fracture_at(xyz), W.at(lab, xyz))
    # an index of n_seeds is refused with nothing changed
    bad = np.array([0, len(seeds)], np.uint32)
    out = C.c_void_p(0x5A5A)
    assert lib.dust_hip_model_fracture_detach(model._h, bad.ctypes.data_as(C.c_void_p), 2, 0, C.byref(out)) == L.ERR_INVALID_ARGUMENT and out.value == 0x5A5A
    assert lib.dust_hip_model_fracture_detach(model._h, bad.ctypes.data_as(C.c_void_p), 2, 2, C.byref(out)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_fracture_detach(model._h, bad.ctypes.data_as(C.c_void_p), 1, L.DETACH_KEEP_SOURCE, None) == L.ERR_INVALID_ARGUMENT
    assert same_bytes(model, grid, pal) and np.array_equal(model.fracture_at(xyz), W.at(lab, xyz))
    assert model.fracture_detach([]) is None
    # the carving detach removes exactly those voxels; the detached voxels answer NO_CELL and the other labels stand
    carved = model.fracture_detach([1, 4])
    assert same_bytes(carved, want_piece, pal) and same_bytes(model, want_rest, pal) and same_hierarchy(model, want_rest, pal, ctx)
    assert np.array_equal(want_piece + want_rest, grid) and np.count_nonzero(want_piece) == int(cells["voxels"][1]) + int(cells["voxels"][4]) > 0
    assert np.array_equal(model.fracture_at(xyz), W.at(want_lab, xyz))
    # a second detach of another cell works without labelling again; out == NULL deletes
    second, rest2, lab2 = W.detach(want_rest, want_lab, [0])
    assert same_bytes(model.fracture_detach([0], keep_source=True), second, pal)
    assert model.fracture_detach([0, 1], receive=False) is None
    assert same_bytes(model, rest2, pal) and np.array_equal(model.fracture_at(xyz), W.at(lab2, xyz))
    # the recipe: a copy per remaining piece, then one deleting detach of all of them
    left = [i for i in range(len(seeds)) if i not in (0, 1, 4) and cells["voxels"][i]]
    assert len(left) >= 4
    for i in left:
        assert same_bytes(model.fracture_detach([i], keep_source=True), W.detach(rest2, lab2, [i])[0], pal)
    model.fracture_detach(left, receive=False)
    assert same_bytes(model, np.zeros_like(grid), pal) and (model.fracture_at(xyz) == L.NO_CELL).all()


def test_apply_seams_open_the_pieces_and_labelled_paints_within_reach():
    grid = np.zeros((256,) * 3, np.uint8)
    x, y, z = ORIGIN
    grid[x:x + 24, y:y + 24, z:z + 24] = 3
    seeds = np.array([(x + 3 + 8 * i, y + 3 + 8 * j, z + 3 + 8 * k) for i in range(3) for j in range(3) for k in range(3)])
    pal = synth.make_palette(47)
    ctx = api.Context(device=0)
    model = make(ctx, grid, pal)
    lab, r, cells = check(model, grid, seeds)
    want, want_changed = W.apply(grid, lab, W.SEAMS, -1)
    assert model.fracture_apply(-1, L.FRACTURE_SEAMS) == want_changed == np.count_nonzero(W.seams(lab)) > 0
    assert same_bytes(model, want, pal) and same_hierarchy(model, want, pal, ctx)
    assert status_of(lambda: model.fracture_at([ORIGIN])) == L.ERR_NOT_READY          # the labelling is invalid afterwards
    assert status_of(lambda: model.fracture_apply(1)) == L.ERR_NOT_READY and status_of(lambda: model.fracture_detach([0])) == L.ERR_NOT_READY
    n, _ = model.find_islands(L.ISLANDS_FACES)
    assert n == len(IW.records(IW.label(want, IW.FACES))) == 27                        # 7^3, 7 x 7 x 8 ... pieces between one-voxel gaps
    # paint within reach of an impact
    model = make(ctx, grid, pal)
    impact = seeds[[13, 14, 16]]
    lab, r, cells = check(model, grid, impact, max_distance2=36)
    want, want_changed = W.apply(grid, lab, W.LABELLED, 9)
    assert model.fracture_apply(9, L.FRACTURE_LABELLED) == want_changed == int(r["labelled"]) and 0 < want_changed < 24 ** 3
    assert same_bytes(model, want, pal)
    lab, r, cells = check(model, want, impact, palette=9)                              # the painted voxels, and only they
    assert int(r["solid"]) == want_changed
    assert model.fracture_apply(9, L.FRACTURE_SEAMS) == 0 and same_bytes(model, want, pal)   # nothing differs: still a rebuild, still invalid
    assert status_of(lambda: model.fracture_at([ORIGIN])) == L.ERR_NOT_READY


def test_validity_matrix_and_refusals():
    rng, grid = random_block(8, size=(18, 18, 18), density=0.8)
    pal = synth.make_palette(48)
    ctx = api.Context(device=0)
    lib = L.load()
    model = make(ctx, grid, pal)
    other = make(ctx, grid, pal)
    seeds = np.array([(12, 120, 205), (20, 130, 212)])
    solid = [tuple(int(c) for c in np.argwhere(grid != 0)[0])]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def standing():
        return lib.dust_hip_model_fracture_at(model._h, None, None, 0) == L.OK

    def fracture():
        model.fracture(seeds)
        assert standing()

    assert not standing() and lib.dust_hip_model_fracture_apply(model._h, 0, 1, None) == L.ERR_NOT_READY
    assert same_bytes(model, grid, pal)
    fracture()
    # what leaves it usable
    model.find_islands(L.ISLANDS_FACES)
    assert standing()
    model.flood(solid, medium=L.FLOOD_SOLID)
    model.distance(max_radius=8)
    model.census(api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [255.0, 255.0, 255.0]))
    assert standing() and model.fracture_at(solid).tolist() == W.at(W.labels(grid, seeds)[0], solid).tolist()
    fracture()                                                            # a second fracture replaces it and leaves the others
    assert model.flood_at(solid).tolist() == [0] and int(model.distance_at(solid)[0]) == 0 and model.island_of(solid)[0] != L.NO_ISLAND
    model.set_voxels(np.zeros((0, 3), np.uint32), np.zeros(0, np.int32))
    assert standing()
    # what invalidates it, whether or not a voxel changes
    model.set_voxels([(200, 200, 200)], [-1])
    assert not standing()
    fracture()
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]))
    assert not standing()
    fracture()
    model.stamp(other, api.stamps([(300, 0, 0)]))
    assert not standing()
    fracture()
    other.stamp(model, api.stamps([(0, 0, 0)]))                           # being a stamp's source
    assert standing()
    model.flood(solid, medium=L.FLOOD_SOLID)
    model.flood_apply(2, max_steps=0)
    assert not standing()
    # a fracture that is refused changes nothing; one that is accepted makes the labelling again
    fracture()
    q = L.FractureQuery(struct_size=C.sizeof(L.FractureQuery), palette=-1, max_distance2=L.FRACTURE_NO_LIMIT)
    q.scale[:] = (1, 1, 1)
    q.hi[:] = (255, 255, 255)
    recs = api.fracture_seeds(seeds)
    fn = lib.dust_hip_model_fracture
    assert fn(model._h, C.byref(q), ptr(recs), 2, None, None) == L.OK
    bad_seed, bad_word = recs.copy(), recs.copy()
    bad_seed["y"][1] = 1280
    bad_word["reserved"][0] = 1
    refusals = [(None, recs, 2), (q, None, 2), (q, recs, L.MAX_FRACTURE_SEEDS + 1), (q, bad_seed, 2), (q, bad_word, 2)]
    for field, value in (("struct_size", 47), ("palette", 255), ("palette", -2), ("flags", 1), ("reserved0", 1), ("reserved", 1)):
        r = L.FractureQuery.from_buffer_copy(q)
        setattr(r, field, value)
        refusals.append((r, recs, 2))
    for axis, value in ((0, 0), (2, 17)):
        r = L.FractureQuery.from_buffer_copy(q)
        r.scale[axis] = value
        refusals.append((r, recs, 2))
    out = np.full(64, 0x5A, np.uint8).view(api.FRACTURE_RESULT_DTYPE)
    for query, s, n in refusals:
        assert fn(model._h, None if query is None else C.byref(query), None if s is None else ptr(s), n, ptr(out), None) == L.ERR_INVALID_ARGUMENT
    assert out.tobytes() == bytes([0x5A]) * 64 and standing()
    xyz = np.array([[1, 2, 256]], np.uint32)
    cells = np.zeros(1, np.uint16)
    assert lib.dust_hip_model_fracture_at(model._h, ptr(xyz), ptr(cells), 1) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_fracture_at(model._h, None, ptr(cells), 1) == L.ERR_INVALID_ARGUMENT
    for where, value in ((2, 0), (0, 255), (1, -2)):
        assert lib.dust_hip_model_fracture_apply(model._h, where, value, None) == L.ERR_INVALID_ARGUMENT
    assert standing()


def test_two_runs_give_the_same_bytes():
    rng, grid = random_block(9, size=(33, 29, 35))
    pal = synth.make_palette(49)
    seeds = np.concatenate([rng.integers(0, 30, (40, 3)) + np.array(ORIGIN), rng.integers(-200, 400, (20, 3))])
    xyz = around(grid, 2)
    runs = []
    for _ in range(2):
        ctx = api.Context(device=0)
        model = make(ctx, grid, pal)
        r, cells = model.fracture(seeds, scale=(2, 1, 5))
        runs.append((model.fracture_at(xyz).tobytes(), r.tobytes(), cells.tobytes()))
    assert runs[0] == runs[1]
    lab, far = W.labels(grid, seeds, scale=(2, 1, 5))
    assert runs[0][0] == W.at(lab, xyz).tobytes()
