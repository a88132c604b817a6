"""Model voxelisation on the device (dust_hip_model_edit_triangles, dust_hip_model_fill_mesh; the contract is in include/dust_hip.h).
Every comparison is exact: `changed` and the result record must be what the witness says (tests/triangle_witness.py), and after every
edit the model must be, byte for byte, a host build of the witness's grid, the upper levels included (dust_hip_model_read_hierarchy).
The inputs are small and placed where the kernels can go wrong: the brick edge 3 | 4, the root-cell edges 15 | 16 and 63 | 64, the
faces of the tree, the range limit, the 65 536-record chunk."""
import ctypes as C

import numpy as np
import pytest

import triangle_witness as W
from dust_amd import _lib as L, api, synth
from flood_witness import to_xyzi

pytestmark = pytest.mark.gpu

HIERARCHY = ("root", "host_root", "mid", "dense_mask", "bmin", "bmax")
U = W.UNIT
M = W.MAX_COORD


def host_model(grid, pal):
    return api.flatten_model(to_xyzi(grid), (256, 256, 256), pal)


def make(ctx, grid, pal):
    return api.Model(ctx, *host_model(grid, pal), pal)


def same_model(model, ctx, grid, pal):
    """the model is, byte for byte, a host build of `grid`"""
    fresh = make(ctx, grid, pal)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), fresh.read()))
    got, want = model.read_hierarchy(), fresh.read_hierarchy()
    assert got["n_mid"] == want["n_mid"] and got["extent_log2"] == want["extent_log2"]
    for name in HIERARCHY:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name


def start_grid(seed=0):
    """a few scattered voxels and a slab of full bricks across 15 | 16 and 63 | 64"""
    rng = np.random.default_rng(seed)
    grid = np.zeros((256,) * 3, np.uint8)
    at = rng.integers(0, 80, (3000, 3))
    grid[at[:, 0], at[:, 1], at[:, 2]] = rng.integers(1, 256, 3000)
    grid[12:20, 60:68, 12:20] = 8
    return grid


def edit(ctx, model, grid, pal, tris):
    """one call on the device and in the witness: `changed` agrees per triangle and the model is a host build of the grid"""
    want = W.edit_triangles(grid, tris)
    got = model.edit_triangles(tris)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist(), (got[:8], want[:8])
    same_model(model, ctx, grid, pal)
    return want


def fill(ctx, model, grid, pal, tris, op=W.FILL, palette=0, region=None):
    """one fill_mesh on the device and in the witness: the result record agrees byte for byte, the model is a host build of the grid"""
    lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
    want = W.fill_mesh(grid, tris, op, palette, lo, hi)
    got = model.fill_mesh(tris, op, palette, region)
    assert got.dtype == api.FILL_MESH_RESULT_DTYPE == W.RESULT_DTYPE and got.tobytes() == want.tobytes(), (got, want)
    same_model(model, ctx, grid, pal)
    return want


def single_triangles():
    """[(name, vertices, covers something)]"""
    out = [("inside one brick", [(4 * U + 30, 4 * U + 40, 5 * U + 50), (7 * U + 200, 5 * U + 10, 6 * U + 20), (5 * U + 90, 7 * U + 220, 4 * U + 70)], True)]
    for axis in range(3):
        for edge in (4, 16, 64):                                              # 3 | 4, 15 | 16, 63 | 64 on every axis
            a, b, c = [100 * U + 77] * 3, [101 * U + 13] * 3, [100 * U + 201] * 3
            a[axis], b[axis], c[axis] = edge * U - 300, edge * U + 290, edge * U + 10
            b[(axis + 1) % 3] += 2 * U
            c[(axis + 2) % 3] -= 3 * U
            out.append((f"across {edge - 1} | {edge} on axis {axis}", [tuple(a), tuple(b), tuple(c)], True))
        flat = [[30 * U + 20, 30 * U + 20], [36 * U + 100, 31 * U], [31 * U, 35 * U + 50]]
        for k in range(3):
            flat[k].insert(axis, (4, 16, 64)[axis] * U)                       # exactly on a voxel face: both sides
        out.append((f"on a voxel face across axis {axis}", [tuple(p) for p in flat], True))
    out += [("meets a cube at a corner", [(40 * U, 40 * U, 40 * U), (40 * U - 300, 40 * U - 10, 40 * U - 200), (40 * U - 20, 40 * U - 310, 40 * U - 100)], True),
            ("an edge along a cube edge", [(48 * U, 16 * U, 64 * U + 100), (48 * U, 16 * U, 64 * U + 200), (48 * U - 500, 16 * U - 300, 64 * U + 150)], True),
            ("a one-unit sliver", [(10 * U + 1, 3 * U + 7, 2 * U + 5), (40 * U + 1, 9 * U + 7, 5 * U + 5), (40 * U + 2, 9 * U + 7, 5 * U + 5)], True),
            ("a needle through the tree", [(-3 * U, 200 * U + 17, 33), (300 * U, 203 * U + 17, 5 * U + 34), (300 * U, 203 * U + 18, 5 * U + 33)], True),
            ("partly outside, negative coordinates", [(-20 * U - 5, -7 * U, 3 * U), (9 * U, 5 * U + 1, -2 * U - 9), (3 * U, -4 * U, 8 * U + 3)], True),
            ("partly above the tree", [(250 * U, 250 * U, 250 * U), (270 * U, 251 * U, 252 * U), (251 * U, 266 * U, 300 * U)], True),
            ("touches the tree from outside", [(256 * U, 10 * U, 10 * U), (256 * U, 12 * U, 10 * U + 5), (256 * U, 10 * U, 13 * U)], True),
            ("wholly outside", [(256 * U + 1, 10 * U, 10 * U), (290 * U, 12 * U, 10 * U + 5), (256 * U + 1, 10 * U, 13 * U)], False),
            ("wholly below", [(5 * U, 5 * U, -1), (9 * U, 5 * U, -1), (5 * U, 9 * U, -U)], False),
            ("at the range limit", [(-M, 3 * U, 7 * U), (-M, 9 * U, 7 * U + 50), (6 * U, 5 * U, 12 * U)], True),
            ("at the range limit, the far side", [(M, 250 * U, M), (M, 255 * U, 251 * U), (250 * U, 252 * U, 250 * U)], True),
            ("beyond the range limit", [(-M - 1, 3 * U, 7 * U), (-M, 9 * U, 7 * U + 50), (6 * U, 5 * U, 12 * U)], False),
            ("beyond the range limit, negative", [(5 * U, 5 * U, 5 * U), (9 * U, 5 * U, 5 * U), (5 * U, -M - 1, 5 * U)], False),
            ("zero normal: a point", [(5 * U, 5 * U, 5 * U)] * 3, False),
            ("zero normal: collinear", [(5 * U, 5 * U, 5 * U), (7 * U, 7 * U, 7 * U), (11 * U, 11 * U, 11 * U)], False)]
    return out


def test_single_triangles():
    pal = synth.make_palette(91)
    ctx = api.Context(device=0)
    grid = start_grid(91)
    model = make(ctx, grid, pal)
    ops = (W.FILL, W.PLACE, W.PAINT, W.CARVE)
    for i, (name, v, covers) in enumerate(single_triangles()):
        before = grid.copy()
        tri = W.triangles([v], ops[i % 4] if covers else W.FILL, 20 + i)
        changed = edit(ctx, model, grid, pal, tri)
        assert (len(W.covered_voxels(v)) > 0) == covers, name
        if not covers:
            assert changed.tolist() == [0] and np.array_equal(before, grid), name
    # FILL of each again on an empty model: every covered voxel changes
    empty = np.zeros((256,) * 3, np.uint8)
    model = make(ctx, empty, pal)
    tris = W.triangles([v for _, v, _ in single_triangles()], W.FILL, 5)
    changed = edit(ctx, model, empty, pal, tris)
    assert all((c > 0) == covers for c, (_, _, covers) in zip(changed.tolist(), single_triangles()))
    assert changed[0] == len(W.covered_voxels(single_triangles()[0][1]))


def test_a_triangle_through_all_4096_root_cells_bounds():
    pal = synth.make_palette(92)
    ctx = api.Context(device=0)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[100:108, 100:108, 100:108] = 3
    model = make(ctx, grid, pal)
    whole = W.triangles([[(0, 0, 0), (256 * U, 256 * U, 256 * U), (256 * U, 0, 256 * U)]], W.PLACE, 7)   # the plane x = z where y <= x
    changed = edit(ctx, model, grid, pal, whole)
    assert changed[0] > 40000 and grid[0, 0, 0] == grid[255, 255, 255] == grid[255, 0, 255] == 8 and grid[103, 101, 103] == 3


def test_order_and_operations_one_call_equals_n_calls():
    rng = np.random.default_rng(93)
    pal = synth.make_palette(93)
    ctx = api.Context(device=0)
    grid = start_grid(93)
    one, many = make(ctx, grid, pal), make(ctx, grid, pal)
    v = (rng.integers(8 * U, 24 * U, (48, 1, 3)) + rng.integers(-6 * U, 6 * U, (48, 3, 3))).astype(np.int64)   # overlapping, across 15 | 16
    v[:, :, 1] += 52 * U                                                                                          # ... and 63 | 64
    tris = W.triangles(v, rng.integers(0, 4, 48), rng.integers(0, 255, 48))
    twin = grid.copy()
    want = edit(ctx, one, grid, pal, tris)
    assert np.count_nonzero(want) >= 24 and len(set(tris["op"].tolist())) == 4
    each = [int(many.edit_triangles(tris[i:i + 1])[0]) for i in range(len(tris))]
    assert each == want.tolist()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one.read(), many.read()))
    again = make(ctx, twin, pal)                                              # two runs: the same bytes and the same counts
    assert again.edit_triangles(tris).tolist() == want.tolist() and all(x.tobytes() == y.tobytes() for x, y in zip(one.read(), again.read()))


def test_65536_tiny_triangles_null_changed_and_n_zero():
    rng = np.random.default_rng(94)
    pal = synth.make_palette(94)
    ctx = api.Context(device=0)
    n = L.MAX_EDIT_TRIANGLES
    voxel = rng.integers(0, 256, (n, 3))
    voxel[:4096] = np.indices((16, 16, 16)).reshape(3, -1).T * 16 + 7          # one in every root cell; the rest anywhere, many per voxel
    inner = rng.integers(20, 236, (n, 3, 3))                                  # strictly inside its voxel: it covers that voxel alone
    inner[:, 1, 0] += 1
    inner[:, 2, 1] += 1                                                       # (never collinear: v1 and v2 leave v0 along x and y... mostly)
    v = voxel[:, None, :] * U + np.clip(inner, 1, 255)
    palette = (np.arange(n) % 255).astype(np.int32)
    tris = W.triangles(v, W.FILL, palette)
    live = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).any(axis=1)        # (products below 2^16: exact)
    assert live.mean() > 0.9
    grid = np.zeros((256,) * 3, np.uint8)
    sample = W.edit_triangles(grid.copy(), tris[:600])                        # the witness on a sample: one voxel each, its own
    assert all(W.covered_voxels(W.verts(t)) == ({tuple(int(c) for c in p)} if a else set()) for t, p, a in zip(tris[:100], voxel[:100], live[:100]))
    # the whole call by its definition, given that: in order, a live triangle sets its voxel to its byte and counts where that differs
    want = np.zeros(n, np.uint32)
    for i in np.flatnonzero(live):
        x, y, z = voxel[i]
        byte = palette[i] + 1
        want[i] = grid[x, y, z] != byte
        grid[x, y, z] = byte
    assert want[:600].tolist() == sample.tolist()
    model = make(ctx, np.zeros((256,) * 3, np.uint8), pal)
    assert model.edit_triangles(tris).tolist() == want.tolist()
    same_model(model, ctx, grid, pal)
    assert model.edit_triangles(tris, count=False) is None                    # changed == NULL: the same edit again, nothing changes
    same_model(model, ctx, grid, pal)
    assert model.edit_triangles(np.zeros(0, api.TRIANGLE_DTYPE)).tolist() == []
    assert L.load().dust_hip_model_edit_triangles(model._h, None, 0, None) == L.OK
    same_model(model, ctx, grid, pal)
    with pytest.raises(L.DustError) as e:
        model.edit_triangles(np.zeros(n + 1, api.TRIANGLE_DTYPE))
    assert e.value.status == L.ERR_INVALID_ARGUMENT


def solids():
    c = 40 * U + 128                                                          # vertices on column centres
    o = [(c - 9 * U, c, c), (c + 9 * U, c, c), (c, c - 9 * U, c), (c, c + 9 * U, c), (c, c, c - 9 * U), (c, c, c + 9 * U)]
    octahedron = [[o[i], o[2 + j], o[4 + k]] for i in range(2) for j in range(2) for k in range(2)]
    t = [(10 * U + 128, 58 * U + 128, 10 * U + 128), (22 * U + 128, 60 * U + 128, 11 * U + 128), (13 * U + 128, 70 * U + 128, 12 * U + 128), (15 * U + 128, 63 * U + 128, 25 * U + 128)]
    tetrahedron = [[t[0], t[1], t[2]], [t[0], t[3], t[1]], [t[1], t[3], t[2]], [t[2], t[3], t[0]]]
    return W.triangles(octahedron), W.triangles(tetrahedron)


def box_mesh(lo, hi):
    """the twelve triangles of an axis-aligned box, corners in units"""
    p = [[(lo[0], hi[0])[i], (lo[1], hi[1])[j], (lo[2], hi[2])[k]] for i in range(2) for j in range(2) for k in range(2)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return W.triangles([[p[a], p[b], p[c]] for q in quads for a, b, c in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])


def test_fill_mesh_solids_ops_regions_and_records():
    pal = synth.make_palette(95)
    ctx = api.Context(device=0)
    grid = start_grid(95)
    model = make(ctx, grid, pal)
    octahedron, tetrahedron = solids()
    r = fill(ctx, model, grid, pal, octahedron, W.FILL, 11)
    assert int(r["covered"]) > 800 and int(r["live"]) == int(r["crossing"]) == 8
    r = fill(ctx, model, grid, pal, tetrahedron, W.PLACE, 12)
    assert int(r["covered"]) > 100 and 0 < int(r["changed"]) <= int(r["covered"])
    fill(ctx, model, grid, pal, tetrahedron, W.PAINT, 13, ((12, 60, 0), (15, 63, 255)))     # regions that cut the mesh
    fill(ctx, model, grid, pal, octahedron, W.CARVE, 0, ((40, 0, 0), (255, 40, 300)))       # (a coordinate past 255 is cut back)
    fill(ctx, model, grid, pal, octahedron, W.PAINT, 14, ((31, 31, 31), (31, 49, 49)))      # one slice
    before = grid.copy()
    r = fill(ctx, model, grid, pal, octahedron, W.FILL, 15, ((50, 50, 50), (49, 60, 60)))   # lo > hi: the zero result, nothing changes
    assert r.tobytes() == W.zero_result().tobytes() and np.array_equal(before, grid)
    r = fill(ctx, model, grid, pal, octahedron, W.FILL, 15, ((256, 0, 0), (300, 9, 9)))
    assert r.tobytes() == W.zero_result().tobytes() and np.array_equal(before, grid)
    assert model.fill_mesh(np.zeros(0, api.TRIANGLE_DTYPE)).tobytes() == W.zero_result().tobytes()   # n == 0
    # partly above 256 and below 0 in z, outside in x and y
    box = box_mesh((-3 * U - 128, 250 * U + 64, -10 * U), (9 * U + 64, 300 * U, 300 * U))
    r = fill(ctx, model, grid, pal, box, W.FILL, 16)
    assert int(r["covered"]) == 9 * 6 * 256 and r["lo"].tolist() == [0, 250, 0] and r["hi"].tolist() == [8, 255, 255]
    beyond = box_mesh((20 * U, 20 * U, 256 * U + 1), (30 * U, 30 * U, 400 * U))                        # wholly above: every centre below has two crossings
    r = fill(ctx, model, grid, pal, beyond, W.FILL, 17)
    assert int(r["covered"]) == 0 and int(r["crossing"]) == 4 and int(r["live"]) == 12
    # vertical-only and n.z == 0 triangles, dead triangles: crossing < live < n
    walls = np.concatenate([box[[i for i in range(12) if W.normal(W.verts(box[i]))[2] == 0]], W.triangles([[(0, 0, 0)] * 3, [(M + 1, 0, 0), (0, U, 0), (U, 0, 0)]])])
    r = fill(ctx, model, grid, pal, walls, W.FILL, 18)
    assert int(r["covered"]) == 0 and int(r["crossing"]) == 0 and int(r["live"]) == 8 and len(walls) == 10
    # an open mesh: the witness's parity, and twice the same bytes
    twin_grid = grid.copy()
    twin = make(ctx, twin_grid, pal)
    r = fill(ctx, model, grid, pal, octahedron[:5], W.FILL, 19)
    assert int(r["covered"]) > 0
    again = twin.fill_mesh(octahedron[:5][::-1], W.FILL, 19)
    assert again.tobytes() == r.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), twin.read()))


def test_fill_mesh_round_trips():
    rng = np.random.default_rng(96)
    pal = synth.make_palette(96)
    ctx = api.Context(device=0)
    blob = rng.random((24, 24, 24)) < 0.5
    offset = (5, 52, 2)                                                       # x 5..28 across 15 | 16, y 52..75 across 63 | 64
    tri = W.triangles(W.face_triangles(blob, offset, rng))                    # shuffled order, random winding and diagonals
    want = np.zeros((256,) * 3, np.uint8)
    want[5:29, 52:76, 2:26][blob] = 31
    grid = np.zeros((256,) * 3, np.uint8)
    model = make(ctx, grid, pal)
    r = fill(ctx, model, grid, pal, tri, W.FILL, 30)
    assert np.array_equal(grid, want) and int(r["covered"]) == int(blob.sum()) == int(r["changed"])
    twin = make(ctx, np.zeros((256,) * 3, np.uint8), pal)                     # two runs: the same record and the same bytes
    again = twin.fill_mesh(tri, W.FILL, 30)
    assert again.tobytes() == r.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(model.read(), twin.read()))


def test_fill_mesh_of_a_models_own_mesh_gives_the_model_back():
    """a hand-built model through its own mesh: Model.mesh -> quads_to_triangles -> fill_mesh of an empty model"""
    pal = synth.make_palette(96)
    ctx = api.Context(device=0)
    built = start_grid(96)
    built[200:256, 0:9, 250:256] = 4
    source = make(ctx, built, pal)
    _, quads = source.mesh(any_palette=True)
    triangles = api.quads_to_triangles(quads)
    assert triangles.dtype == api.TRIANGLE_DTYPE == W.TRIANGLE_DTYPE and len(triangles) == 2 * len(quads)
    copy_grid = np.zeros((256,) * 3, np.uint8)
    copy = make(ctx, copy_grid, pal)
    got = copy.fill_mesh(triangles, W.FILL, 6)
    assert int(got["covered"]) == int(got["changed"]) == int(np.count_nonzero(built)) and int(got["live"]) == len(triangles)
    same_model(copy, ctx, np.where(built != 0, 7, 0).astype(np.uint8), pal)


def test_fill_mesh_of_more_than_65536_crossing_triangles():
    """The call lists only the crossing triangles (n.z != 0) that reach a column of the region, 65 536 records per launch: a mesh with
    more of those than that takes the chunk path -- later launches XOR into the volume the earlier ones wrote, with ids and records
    counted from the chunk's first. Thin slabs stacked along z: every column has 24 crossings, and after the shuffle both chunks hold
    crossings of every tile."""
    pal = synth.make_palette(97)
    ctx = api.Context(device=0)
    rng = np.random.default_rng(97)
    slabs = np.zeros((40, 40, 24), bool)
    slabs[:, :, ::2] = True                                                   # twelve one-voxel slabs with air between
    slabs &= rng.random(slabs.shape) > 0.03                                   # ... and a few holes
    offset = (5, 50, 3)                                                       # x 5..44 across 15 | 16, y 50..89 across 63 | 64
    v = W.face_triangles(slabs, offset, rng)                                  # shuffled order, random winding and diagonals
    tri = W.triangles(v)
    crossing = int(np.count_nonzero(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])[:, 2]))
    assert crossing > 65536 and crossing == 4 * int(slabs.sum())              # (here, on the CPU: more than one chunk of records;
    inside_x = (v[:, :, 0] >= 5 * U).all(axis=1) & (v[:, :, 0] <= 45 * U).all(axis=1)   # every one of them reaches a column of the tree)
    assert inside_x.all()
    # the witness's triangle loop over all of them would take longer than the rest of the file: the round trip's identity
    # (tests/test_triangle_witness.py) gives the answer -- the voxels themselves -- and the witness confirms it on one slab of columns
    want = np.zeros((256,) * 3, np.uint8)
    want[5:45, 50:90, 3:27][slabs] = 41
    slab = (v[:, :, 0] >= 15 * U).all(axis=1) & (v[:, :, 0] <= 17 * U).all(axis=1)
    assert np.array_equal(W.inside(W.triangles(v[slab]), (15, 50, 3), (16, 89, 26)), slabs[10:12])
    grid = np.zeros((256,) * 3, np.uint8)
    model = make(ctx, grid, pal)
    r = model.fill_mesh(tri, W.FILL, 40)
    at = np.argwhere(slabs)
    assert int(r["covered"]) == int(r["changed"]) == int(slabs.sum()) and int(r["live"]) == len(tri) and int(r["crossing"]) == crossing
    assert r["lo"].tolist() == (at.min(axis=0) + offset).tolist() and r["hi"].tolist() == (at.max(axis=0) + offset).tolist()
    same_model(model, ctx, want, pal)
    # a region that cuts it: fewer records than a chunk again, the same voxels inside the region
    cut = make(ctx, grid, pal)
    r = cut.fill_mesh(tri, W.FILL, 40, ((10, 60, 0), (20, 70, 255)))
    assert int(r["covered"]) == int(slabs[5:16, 10:21].sum()) and int(r["crossing"]) == crossing
    part = np.zeros((256,) * 3, np.uint8)
    part[10:21, 60:71] = want[10:21, 60:71]
    same_model(cut, ctx, part, pal)


def test_refused_calls_leave_everything_alone_and_scenes_wait_for_a_commit():
    pal = synth.make_palette(98)
    ctx = api.Context(device=0)
    grid = start_grid(98)
    model = make(ctx, grid, pal)
    scene = api.Scene(ctx)
    scene.add_instance(model, np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32).reshape(12))
    scene.commit()
    origin, direction = np.float32([[16.5, 64.5, 300.0]]), np.float32([[0.0, 0.0, -1.0]])
    hit = scene.trace_rays(origin, direction)[0]
    assert hit["instance"] == 0
    lib = L.load()
    octahedron, _ = solids()
    source = [a.tobytes() for a in model.read()]
    changed = np.full(8, 0x5A5A5A5A, np.uint32)
    result = np.full(48, 0x5A, np.uint8)
    bad_op, bad_palette = octahedron.copy(), octahedron.copy()
    bad_op["op"][7], bad_palette["palette"][3] = 4, 255
    for tris in (bad_op, bad_palette):
        assert lib.dust_hip_model_edit_triangles(model._h, tris.ctypes.data_as(C.c_void_p), 8, changed.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_edit_triangles(model._h, None, 8, changed.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID_ARGUMENT

    def query(op=W.FILL, palette=0, flags=0, reserved=(0, 0), size=48):
        q = L.FillMeshQuery(struct_size=size, op=op, palette=palette, flags=flags)
        q.hi[:], q.reserved[:] = (255, 255, 255), reserved
        return q
    for q in (query(op=4), query(palette=255), query(palette=-1), query(flags=1), query(reserved=(0, 1)), query(size=47)):
        assert lib.dust_hip_model_fill_mesh(model._h, bad_op.ctypes.data_as(C.c_void_p), 8, C.byref(q), result.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID_ARGUMENT
    q = query()
    assert lib.dust_hip_model_fill_mesh(model._h, None, 8, C.byref(q), result.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_fill_mesh(model._h, bad_op.ctypes.data_as(C.c_void_p), L.MAX_MESH_TRIANGLES + 1, C.byref(q), None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_fill_mesh(model._h, bad_op.ctypes.data_as(C.c_void_p), 8, None, None) == L.ERR_INVALID_ARGUMENT
    assert (changed == 0x5A5A5A5A).all() and (result == 0x5A).all() and [a.tobytes() for a in model.read()] == source
    assert scene.trace_rays(origin, direction)[0]["t"] == hit["t"]            # nothing happened: the scene still answers
    # an edit: the scene answers NOT_READY until it is committed again, as after edit_shapes
    lid = W.triangles([[(10 * U, 58 * U, 30 * U + 128), (24 * U, 58 * U, 30 * U + 128), (10 * U, 72 * U, 30 * U + 128)]], W.FILL, 2)
    edit(ctx, model, grid, pal, lid)
    with pytest.raises(L.DustError) as e:
        scene.trace_rays(origin, direction)
    assert e.value.status == L.ERR_NOT_READY
    scene.commit()
    after = scene.trace_rays(origin, direction)[0]
    assert after["t"] < hit["t"] and tuple(int(c) for c in after["xyz"]) == (16, 64, 30)
    fill(ctx, model, grid, pal, octahedron, W.CARVE)
    with pytest.raises(L.DustError) as e:
        scene.trace_rays(origin, direction)
    assert e.value.status == L.ERR_NOT_READY
    scene.commit()
    assert scene.trace_rays(origin, direction)[0]["t"] == after["t"]
