"""What k_edit_upper_levels (dust_amd/csrc/edit.hip) writes -- the N16 root, the mid nodes, dense_mask, n_mid, the tight bounds -- and the
root copy a scene commit uses, read back through dust_hip_model_read_hierarchy after every call that ends in the device-side rebuild, and
held three ways, byte for byte: (a) the edited model, (b) a fresh model that dust_hip_model_create builds from the host flatten of the same
voxels, (c) tests/hierarchy_witness.py. The witness's descend(), the lookup the kernels do, must find every block of model.read() in the
device's arrays and none of a sample of empty bricks. No tolerance anywhere: integers and exactly representable floats."""
import functools

import numpy as np
import pytest

import distance_witness as DW
import flood_witness as FW
import hierarchy_witness as HW
import island_witness as IW
import shape_edit_witness as SW
import stamp_witness as TW
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

PAL = synth.make_palette(3)
MID_BITS = (0, 31, 32, 63)     # the ends of DevN4::mask_lo and mask_hi


@pytest.fixture(scope="module")
def ctx():
    return api.Context(device=0)


def empty_grid():
    return np.zeros((256, 256, 256), np.uint8)


def host_model(ctx, grid):
    """(b): the product's host flatten of the grid's voxels -> dust_hip_model_create"""
    return api.Model(ctx, *api.flatten_model(IW.to_xyzi(grid), (256, 256, 256), PAL), PAL)


def go_to(model, before, after):
    """one set_voxels call that takes the model from one grid to the other"""
    xyz, values = SW.edit_list(before, after)
    assert len(xyz)
    model.set_voxels(xyz, values)


def same(got, want, what):
    """every array of the contract, nothing left out: all 656 root bytes, host_root against the root's first 640, the n_mid mid nodes with
    their pad, n_mid * 64 dense masks, n_mid, the bounds as float32 bit patterns"""
    assert got["extent_log2"] == 8 and got["n_l2"] == 0 and len(got["l2"]) == 0 and len(got["l2_cells"]) == 0, what
    assert got["n_mid"] == want["n_mid"] == len(got["mid"]) and len(got["dense_mask"]) == want["n_mid"] * 64, (what, got["n_mid"], want["n_mid"])
    assert len(got["root"]) == HW.N16_BYTES and len(got["host_root"]) == HW.N16_ROOT_BYTES
    for name in ("root", "mid", "dense_mask"):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.tobytes() == w.tobytes(), f"{what}: {name} differs first at byte {int(np.flatnonzero(g.view(np.uint8) != w.view(np.uint8))[0])}"
    assert got["host_root"].tobytes() == got["root"][:HW.N16_ROOT_BYTES].tobytes() == want["root"][:HW.N16_ROOT_BYTES].tobytes(), f"{what}: host_root"
    for name in ("bmin", "bmax"):
        assert got[name].dtype == np.float32 and got[name].tobytes() == want[name].tobytes(), (what, name, got[name], want[name])


def three_ways(ctx, model, grid, what, rng=None):
    bricks = HW.bricks_of_grid(grid)
    want = HW.build(bricks, 8)
    fresh = host_model(ctx, grid)
    a, b = model.read_hierarchy(), fresh.read_hierarchy()
    same(a, want, what + ", edited against the witness")
    same(b, want, what + ", fresh against the witness")
    same(a, b, what + ", edited against fresh")
    blocks, materials = model.read()
    fresh_blocks, fresh_materials = fresh.read()
    assert blocks.tobytes() == fresh_blocks.tobytes() and materials.tobytes() == fresh_materials.tobytes(), what
    # the witness's block order is the device's; descend finds block i for every block i, and no empty brick
    assert np.array_equal(np.stack([blocks["x"], blocks["y"], blocks["z"]], axis=1), want["block_xyz"]) and np.array_equal(blocks["mask"], want["block_mask"]), what
    for i, (x, y, z) in enumerate(want["block_xyz"].tolist()):
        assert HW.descend(a, x >> 2, y >> 2, z >> 2) == i, (what, x, y, z)
    empty = HW.probes(bricks, 8, rng or np.random.default_rng(3))
    if len(empty) > 3000:
        empty = [empty[i] for i in np.random.default_rng(4).choice(len(empty), 3000, replace=False)] + [c for c in empty if all(v in (0, 63) for v in c)]
    for c in empty:
        assert HW.descend(a, *c) == -1, (what, c)
    return fresh, a


def leaf_codes(grid):
    """the non-empty bricks' codes in the rebuild's lattice order: root cell * 64 + mid bit"""
    b = np.array(list(HW.bricks_of_grid(grid)), np.int64)
    return ((((b[:, 0] >> 2) << 8) | ((b[:, 1] >> 2) << 4) | (b[:, 2] >> 2)) << 6) | ((b[:, 0] & 3) << 4) | ((b[:, 1] & 3) << 2) | (b[:, 2] & 3)


def brick_of(cell, bit):
    """the lowest voxel of the brick at mid bit `bit` of root cell (cx, cy, cz)"""
    return (cell[0] * 16 + (bit >> 4) * 4, cell[1] * 16 + ((bit >> 2) & 3) * 4, cell[2] * 16 + (bit & 3) * 4)


@functools.lru_cache(maxsize=None)
def state(k):
    """the grids of the set_voxels sequence, 1-based as the docstring of test_set_voxels_sequence numbers them"""
    g = empty_grid()
    rng = np.random.default_rng(100 + k)
    if k == 2:
        g[0, 0, 0] = 5
    elif k == 3:
        g[255, 255, 255] = 6
    elif k == 4:       # one voxel in each of the 4096 root cells, anywhere inside it
        cells = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 3)
        v = cells * 16 + rng.integers(0, 16, cells.shape)
        g[v[:, 0], v[:, 1], v[:, 2]] = rng.integers(1, 256, len(v))
    elif k == 5:       # root cells 0, 2047 and 4095
        g[3, 9, 14] = 1
        g[7 * 16 + 5, 15 * 16 + 1, 15 * 16 + 15] = 2
        g[255, 240, 250] = 3
    elif k == 7:       # one root cell fully solid; its face neighbours hold single bricks at the ends of the two mask words
        g[112:128, 112:128, 112:128] = rng.integers(1, 256, (16, 16, 16))
        for n, d in enumerate(((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1))):
            x, y, z = brick_of((7 + d[0], 7 + d[1], 7 + d[2]), MID_BITS[n % 4])
            g[x + n % 4, y + 1, z + 3] = 9
        for bit in MID_BITS:     # ... and the sixth all four
            x, y, z = brick_of((7, 7, 6), bit)
            g[x, y, z] = 10
    elif k == 8:       # a few thousand voxels over the whole tree and a slab of full bricks
        v = rng.integers(0, 256, (3000, 3))
        g[v[:, 0], v[:, 1], v[:, 2]] = rng.integers(1, 256, len(v))
        g[40:72, 100:104, 60:92] = 7
    else:
        assert k in (1, 6)
    g.setflags(write=False)
    return g


def test_set_voxels_sequence(ctx):
    """One model, never recreated, through set_voxels alone -- so going from large to small is part of it:
    1 empty (created empty, made editable by clearing an already empty voxel); 2 the single voxel (0, 0, 0); 3 the single voxel
    (255, 255, 255); 4 one voxel in each of the 4096 root cells (n_mid == the capacity of the mid buffer); 5 back down to three voxels, in
    root cells 0, 2047 and 4095; 6 empty again; 7 one root cell fully solid, single bricks at mid bits 0, 31, 32 and 63 around it; 8 a
    random model over the whole tree plus a slab of full bricks, its bricks straddling many 1024-code chunks of k_table_scan_local."""
    model = host_model(ctx, empty_grid())
    assert model.read_hierarchy()["n_mid"] == 0
    model.set_voxels(np.array([[17, 200, 3]], np.uint32), np.array([-1], np.int32))
    three_ways(ctx, model, state(1), "state 1")
    n_mid = {}
    for k in range(2, 9):
        go_to(model, state(k - 1), state(k))
        _, a = three_ways(ctx, model, state(k), f"state {k}")
        n_mid[k] = a["n_mid"]
    assert (n_mid[2], n_mid[3], n_mid[4], n_mid[5], n_mid[6], n_mid[7]) == (1, 1, 4096, 3, 0, 7)
    assert sorted(np.flatnonzero(np.unpackbits(model_root_mask(state(5)), bitorder="little")).tolist()) == [0, 2047, 4095]
    chunks = np.unique(leaf_codes(state(8)) >> 10)
    assert len(chunks) > 200 and chunks.min() < 8 and chunks.max() > 247, "state 8 must straddle the scan chunks of k_table_scan_local"
    assert 3000 < int(np.count_nonzero(state(8))) < 8000 and np.count_nonzero(np.array(list(HW.bricks_of_grid(state(8)).values()), np.uint64) == np.uint64((1 << 64) - 1)) == 64


def model_root_mask(grid):
    return HW.build(HW.bricks_of_grid(grid), 8)["root"][:512]


def start_grid(seed):
    """what the other entry points start from: a host-built model (its first edit is make_editable's switch and rebuild), sparse voxels in a
    64^3 corner region and two solid root cells"""
    rng = np.random.default_rng(seed)
    g = empty_grid()
    v = rng.integers(16, 80, (1500, 3))
    g[v[:, 0], v[:, 1], v[:, 2]] = rng.integers(1, 255, len(v))
    g[96:112, 32:48, 48:64] = 4
    g[32:48, 64:80, 16:32] = rng.integers(1, 255, (16, 16, 16))
    return g


def test_make_editable_alone(ctx):
    """the first-edit switch with nothing edited: an n == 0 batch moves the model into its full-capacity buffers and rebuilds it"""
    grid = start_grid(11)
    model = host_model(ctx, grid)
    before = model.read_hierarchy()
    model.set_voxels(np.zeros((0, 3), np.uint32), np.zeros(0, np.int32))
    _, after = three_ways(ctx, model, grid, "make_editable")
    same(after, before, "make_editable against the model before it")


def test_edit_shapes(ctx):
    """a carve that removes a whole root cell, a fill that creates one, and a sphere across cell boundaries"""
    grid = start_grid(12)
    model = host_model(ctx, grid)
    shapes = SW.shapes(SW.shape(SW.BOX, (96.0, 32.0, 48.0), (112.0, 48.0, 64.0), op=SW.CARVE),
                       SW.shape(SW.BOX, (208.0, 224.0, 240.0), (224.0, 240.0, 256.0), op=SW.FILL, palette=17),
                       SW.shape(SW.SPHERE, (48.5, 48.5, 48.5), radius=9.0, op=SW.PLACE, palette=30))
    want_changed = SW.apply_to_grid(grid, shapes)
    assert not grid[96:112, 32:48, 48:64].any() and (grid[208:224, 224:240, 240:256] == 18).all() and want_changed[0] == want_changed[1] == 4096
    assert model.edit_shapes(shapes).tolist() == want_changed.tolist()
    _, a = three_ways(ctx, model, grid, "edit_shapes")
    assert a["bmax"].tolist() == [224.0, 240.0, 256.0]


def test_stamp_from_another_model_and_onto_itself(ctx):
    grid = start_grid(13)
    src_grid = empty_grid()
    rng = np.random.default_rng(14)
    src_grid[200:230, 10:30, 100:124] = np.where(rng.random((30, 20, 24)) < 0.2, rng.integers(1, 255, (30, 20, 24)), 0)
    model, src = host_model(ctx, grid), host_model(ctx, src_grid)
    flip = TW.orient_word((2, 0, 1), (1, 0, 1))
    stamps = np.concatenate([TW.records((150, 180, 3), TW.IDENTITY, TW.PLACE, (200, 10, 100), (229, 29, 123)),
                             TW.records((-10, 240, 120), flip, TW.OVERWRITE, (200, 10, 100), (229, 29, 123))])
    want, want_changed = TW.stamp(grid, src_grid, stamps)
    assert model.stamp(src, stamps).tolist() == want_changed.tolist() and want_changed.min() > 0
    three_ways(ctx, model, want, "stamp from another model")
    before = src.read_hierarchy()
    same(before, HW.build(HW.bricks_of_grid(src_grid), 8), "the stamp's source is not touched")
    onto = np.concatenate([TW.records((100, 100, 100), flip, TW.REPLACE, (16, 16, 16), (79, 79, 79)),
                           TW.records((90, 30, 50), TW.IDENTITY, TW.CARVE, (96, 32, 48), (111, 47, 63))])
    want2, want_changed2 = TW.stamp(want, want, onto)
    assert model.stamp(model, onto).tolist() == want_changed2.tolist() and want_changed2.min() > 0
    three_ways(ctx, model, want2, "stamp onto itself")


def test_flood_apply(ctx):
    """water poured into the air around the sparse voxels of one region, and a solid root cell flooded away through its own material"""
    grid = start_grid(15)
    model = host_model(ctx, grid)
    region = ((10, 10, 10), (60, 40, 50))
    seed = np.array([[11, 11, 11]])
    assert grid[11, 11, 11] == 0
    field = FW.steps(grid, seed, FW.EMPTY, max_steps=20, region=region)
    want, n = FW.apply(grid, field, 21, 18)
    assert model.flood(seed, L.FLOOD_EMPTY, max_steps=20, region=region)["reached"] == np.count_nonzero(field != FW.UNREACHED)
    assert model.flood_apply(21, 18) == n > 1000
    three_ways(ctx, model, want, "flood_apply filling")
    seed = np.array([[100, 40, 50]])
    field = FW.steps(want, seed, FW.MATERIAL, palette=3)
    want2, n2 = FW.apply(want, field, -1)
    model.flood(seed, L.FLOOD_MATERIAL, palette=3)
    assert model.flood_apply(-1) == n2 == 4096
    three_ways(ctx, model, want2, "flood_apply clearing a root cell")


def test_distance_apply(ctx):
    """grow the solid by two voxels (new bricks and new root cells around it), then erode it by one"""
    grid = start_grid(16)
    model = host_model(ctx, grid)
    values = DW.field(grid, DW.TO_SOLID, DW.EUCLIDEAN, 2)
    want, n = DW.apply(grid, values, 40, 1, 4)
    model.distance(L.DISTANCE_TO_SOLID, L.DISTANCE_EUCLIDEAN, 2)
    assert model.distance_apply(40, 1, 4) == n > 4096
    three_ways(ctx, model, want, "distance_apply growing")
    values = DW.field(want, DW.TO_EMPTY, DW.CHEBYSHEV, 1)
    want2, n2 = DW.apply(want, values, -1, 1, 1)
    model.distance(L.DISTANCE_TO_EMPTY, L.DISTANCE_CHEBYSHEV, 1)
    assert model.distance_apply(-1, 1, 1) == n2 > 4096
    three_ways(ctx, model, want2, "distance_apply eroding")


def test_detach_islands(ctx):
    """the detached piece is born editable and never goes through make_editable's own rebuild; the carved source; and a KEEP_SOURCE copy
    that leaves the source's arrays as they were"""
    grid = empty_grid()
    rng = np.random.default_rng(17)
    grid[20:52, 20:30, 20:52] = np.where(rng.random((32, 10, 32)) < 0.35, rng.integers(1, 255, (32, 10, 32)), 0)
    grid[32:48, 48:64, 32:48] = 8          # a solid root cell above the rubble, touching nothing
    grid[60:64, 60:64, 60:64] = 9
    model = host_model(ctx, grid)
    labels = IW.label(grid, IW.FACES)
    recs = IW.records(labels)
    n, got = model.find_islands(L.ISLANDS_FACES)
    assert n == len(recs) > 20 and got["key"].tolist() == recs["key"].tolist()
    cell_key = 32 << 16 | 48 << 8 | 32
    keys = [int(k) for k in recs["key"][recs["voxels"] > 3]]
    assert cell_key in keys and 3 < len(keys) < len(recs)
    before = model.read_hierarchy()
    piece_grid, rest_grid = IW.detach(grid, labels, keys)
    copy = model.detach_islands(keys, keep_source=True)
    three_ways(ctx, copy, piece_grid, "a KEEP_SOURCE piece")
    same(model.read_hierarchy(), before, "the source of a KEEP_SOURCE detach")
    three_ways(ctx, model, grid, "the source of a KEEP_SOURCE detach")
    piece = model.detach_islands(keys)
    three_ways(ctx, piece, piece_grid, "the detached piece")
    three_ways(ctx, model, rest_grid, "the carved source")
    assert piece_grid.any() and rest_grid.any() and not rest_grid[32:48, 48:64, 32:48].any()


def test_a_deep_model_reads_back_as_the_witness(ctx):
    """a 4096^3 tree cannot be edited on the device; its read-back -- the l2 nodes and the per-cell table besides the rest -- is what
    dust_hip_model_create uploaded, which is the witness's"""
    blocks, materials = synth.procedural_deep_blocks(occupancy=1e-7, sample=True)
    model = api.Model(ctx, blocks, materials, PAL, tree_extent_log2=12)
    bricks = {(int(b["x"]) >> 2, int(b["y"]) >> 2, int(b["z"]) >> 2): int(b["mask"]) for b in blocks}
    want = HW.build(bricks, 12)
    got = model.read_hierarchy()
    assert (got["extent_log2"], got["n_mid"], got["n_l2"]) == (12, want["n_mid"], want["n_l2"]) and want["n_l2"] > 50
    for name in ("root", "host_root", "l2", "l2_cells", "mid", "dense_mask", "bmin", "bmax"):
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    for i, b in enumerate(model.read()[0]):
        assert HW.descend(got, int(b["x"]) >> 2, int(b["y"]) >> 2, int(b["z"]) >> 2) == i
    for c in HW.probes(bricks, 12, np.random.default_rng(9)):
        assert HW.descend(got, *c) == -1, c


def extreme_rays(grid):
    """a few hundred rays from outside the bounds along each axis: aimed at the voxels with the smallest and the largest coordinate on every
    axis, and up to two voxels past them on every side"""
    xyz = np.argwhere(grid != 0)
    picks = set()
    for axis in range(3):
        for side in (xyz[:, axis].min(), xyz[:, axis].max()):
            at = xyz[xyz[:, axis] == side]
            picks.add(tuple(int(v) for v in at[len(at) // 2]))
    origins, directions = [], []
    for v in sorted(picks):
        for axis in range(3):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            for du, dw in ((a, b) for a in range(-2, 3) for b in range(-2, 3)):
                for sign in (1.0, -1.0):
                    o = np.array(v, np.float64) + 0.5
                    o[u] += du
                    o[w] += dw
                    o[axis] = -20.0 if sign > 0 else 276.0
                    d = np.zeros(3)
                    d[axis] = sign
                    origins.append(o)
                    directions.append(d)
    return np.array(origins, np.float32), np.array(directions, np.float32)


@pytest.mark.parametrize("k", (2, 3, 4, 7))
def test_rays_at_the_extreme_voxels_answer_as_on_a_fresh_model(ctx, k):
    """the consequence: a scene on the edited model (which came down from the state before) and one on a fresh model answer the same rays
    with the same records"""
    model = host_model(ctx, state(k - 1))
    go_to(model, state(k - 1), state(k))
    fresh, _ = three_ways(ctx, model, state(k), f"state {k} from state {k - 1}")
    origins, directions = extreme_rays(state(k))
    assert 100 <= len(origins) <= 1000
    hits = []
    for m in (model, fresh):
        scene = api.Scene(ctx)
        scene.add_instance(m, np.eye(3, 4, dtype=np.float32).reshape(12))
        scene.commit()
        hits.append(scene.trace_rays(origins, directions))
    assert hits[0].tobytes() == hits[1].tobytes()
    found = hits[0]["instance"] != L.NO_HIT
    assert found.any() and not found.all()
    solid = state(k)[hits[0]["xyz"][found][:, 0], hits[0]["xyz"][found][:, 1], hits[0]["xyz"][found][:, 2]]
    assert (solid == hits[0]["palette"][found].astype(np.int64) + 1).all()
