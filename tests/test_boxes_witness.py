"""tests/boxes_witness.py held to the text of the contract (include/dust_hip.h, "Model boxes") by other means than its own: the boxes
paint the set exactly once; no run, rect or box can grow; a per-voxel reading of the rule on a 12^3 block; the mesh witness on a
one-slice slab; the three axes against each other on transposed grids."""
import itertools

import numpy as np
import pytest

import boxes_witness as W
import mesh_witness as M
import surface_witness as S


def random_block(seed, density, materials, shape=(40, 40, 40)):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, materials + 1, shape), 0).astype(np.uint8)


BLOCKS = [(0.5, 1), (0.9, 2), (0.97, 3)]
QUERIES = [dict(), dict(any_palette=True), dict(palette=0), dict(region=((3, 5, 7), (30, 22, 38))), dict(region=((3, 5, 7), (30, 22, 38)), palette=1, any_palette=True),
           dict(region=((17, 0, 0), (17, 39, 39))), dict(region=((9, 9, 9), (9, 9, 9)))]


@pytest.mark.parametrize("which", range(3))
def test_partition_and_result(which):
    grid = random_block(200 + which, *BLOCKS[which])
    deeper = 0
    for axis, query in itertools.product(range(3), QUERIES):
        result, boxes = W.boxes(grid, axis=axis, **query)
        want = W.the_set(grid, query.get("palette", -1), query.get("region"))
        count, bytes_ = W.paint(boxes, grid.shape, with_palette=True)
        assert np.array_equal(count, (want != 0).astype(np.uint16)), (axis, query)   # exactly 1 on S, 0 elsewhere
        if not query.get("any_palette"):
            assert np.array_equal(bytes_, want), (axis, query)                      # ... and of the voxels' own material
        solid = np.argwhere(want != 0)
        assert int(result["boxes"]) == len(boxes) <= int(result["rects"]) <= int(result["voxels"]) == len(solid)
        assert int(result["voxels"]) == int(S.surface(grid, palette=query.get("palette", -1), region=query.get("region"))[0]["solid"])
        if len(solid):
            assert result["lo"].tolist() == solid.min(axis=0).tolist() and result["hi"].tolist() == solid.max(axis=0).tolist()
        else:
            assert result.tobytes() == W.zero_result().tobytes()
        # the documented order, and the key voxel's palette
        lo, hi = W.bounds(boxes)
        n, v, u = W.AXES[axis]
        order = (lo[:, n] << 16) | (lo[:, v] << 8) | lo[:, u]
        assert np.all(np.diff(order) > 0)
        assert np.array_equal(boxes["palette"].astype(np.int64) + 1, grid[tuple(lo.T)])
        deeper += int(np.count_nonzero(hi[:, n] > lo[:, n]))
    assert deeper > 100                                                           # slices really stacked


def identical(a, name, s, v0, v1, u0, u1, nm):
    """slice s of a[s, v, u] holds the rect (v0..v1, u0..u1) of name nm as a RECT: every row holds the run, maximal along u, and the
    rows before and after do not hold the same run"""
    def row_holds_run(v):
        if not (0 <= v < a.shape[1]) or not np.all(name[s, v, u0:u1 + 1] == nm):
            return False
        return (u0 == 0 or name[s, v, u0 - 1] != nm) and (u1 == a.shape[2] - 1 or name[s, v, u1 + 1] != nm)
    if not (0 <= s < a.shape[0]):
        return False
    return all(row_holds_run(v) for v in range(v0, v1 + 1)) and not row_holds_run(v0 - 1) and not row_holds_run(v1 + 1)


@pytest.mark.parametrize("which", range(3))
def test_maximality(which):
    grid = random_block(210 + which, *BLOCKS[which], shape=(14, 15, 16))
    for axis, query in itertools.product(range(3), (dict(), dict(any_palette=True), dict(region=((2, 3, 1), (11, 9, 13))), dict(palette=0))):
        any_palette = bool(query.get("any_palette"))
        a = np.transpose(W.the_set(grid, query.get("palette", -1), query.get("region")), W.AXES[axis])
        name = (a != 0).astype(np.uint8) if any_palette else a
        runs, rects, boxes = W.decompose(grid, axis=axis, **query)
        assert len(boxes["s0"]) > 0
        for s, v, u0, u1, nm in zip(*(runs[k].tolist() for k in ("s", "v", "u0", "u1", "name"))):
            assert nm != 0 and np.all(name[s, v, u0:u1 + 1] == nm)
            assert (u0 == 0 or name[s, v, u0 - 1] != nm) and (u1 == a.shape[2] - 1 or name[s, v, u1 + 1] != nm)
        for s, v0, v1, u0, u1, nm in zip(*(rects[k].tolist() for k in ("s", "v0", "v1", "u0", "u1", "name"))):
            assert identical(a, name, s, v0, v1, u0, u1, nm)
        for s0, s1, v0, v1, u0, u1, nm in zip(*(boxes[k].tolist() for k in ("s0", "s1", "v0", "v1", "u0", "u1", "name"))):
            assert all(identical(a, name, s, v0, v1, u0, u1, nm) for s in range(s0, s1 + 1))
            assert not identical(a, name, s0 - 1, v0, v1, u0, u1, nm) and not identical(a, name, s1 + 1, v0, v1, u0, u1, nm)


def per_voxel_boxes(grid, axis, any_palette):
    """the rule read voxel by voxel: runs row by row, rects by looking each run up in the row before, boxes by looking each rect up in
    the slice before -- dictionaries and Python loops, nothing shared with the witness"""
    a = np.transpose(grid, W.AXES[axis]).tolist()
    ns, nv, nu = len(a), len(a[0]), len(a[0][0])
    name = (lambda b: 1) if any_palette else (lambda b: b)
    rects_of = []                                                                 # per slice: {(v0, v1, u0, u1, name): byte of the key voxel}
    for s in range(ns):
        open_, done = {}, {}                                                      # rects still growing: (u0, u1, name) -> (v0, byte)
        for v in range(nv + 1):
            row = {}
            if v < nv:
                u = 0
                while u < nu:
                    if a[s][v][u] == 0:
                        u += 1
                        continue
                    u0 = u
                    while u + 1 < nu and a[s][v][u + 1] != 0 and name(a[s][v][u + 1]) == name(a[s][v][u0]):
                        u += 1
                    row[(u0, u, name(a[s][v][u0]))] = a[s][v][u0]
                    u += 1
            for run, (v0, byte) in list(open_.items()):
                if run not in row:
                    done[(v0, v - 1) + run] = byte
                    del open_[run]
            for run, byte in row.items():
                open_.setdefault(run, (v, byte))
        rects_of.append(done)
    out = []
    for s in range(ns):
        for rect, byte in rects_of[s].items():
            if s > 0 and rect in rects_of[s - 1]:
                continue
            s1 = s
            while s1 + 1 < ns and rect in rects_of[s1 + 1]:
                s1 += 1
            out.append((s, rect[0], rect[2], s1, rect[1], rect[3], byte))        # s0, v0, u0, s1, v1, u1
    return sorted(out), sum(len(r) for r in rects_of)


@pytest.mark.parametrize("which", range(3))
def test_per_voxel_reading_on_a_small_block(which):
    grid = random_block(220 + which, *BLOCKS[which], shape=(12, 12, 12))
    for axis, any_palette in itertools.product(range(3), (False, True)):
        want, want_rects = per_voxel_boxes(grid, axis, any_palette)
        result, boxes = W.boxes(grid, axis=axis, any_palette=any_palette)
        lo, hi = W.bounds(boxes)
        n, v, u = W.AXES[axis]
        got = [tuple(r) for r in np.stack([lo[:, n], lo[:, v], lo[:, u], hi[:, n], hi[:, v], hi[:, u], boxes["palette"].astype(np.int64) + 1], axis=1).tolist()]
        assert got == want and int(result["rects"]) == want_rects


def test_hand_made_shapes():
    grid = np.zeros((16, 16, 16), np.uint8)
    grid[2:5, 3:7, 1:9] = 1                                                       # one box 3 x 4 x 8
    grid[6, 3:7, 1:9], grid[7, 3:7, 1:10], grid[8, 3:8, 1:10] = 1, 1, 1           # the same corner, a longer u1, then a taller v1: nothing stacks
    grid[10, 10:12, 10:12], grid[11, 10:12, 10:12] = 2, 3                         # identical rects of two materials
    grid[13:16, 0:3, 12:15] = 4
    grid[15, 1, 13] = 0                                                           # the third slice lacks its middle voxel
    result, boxes = W.boxes(grid)
    lo, hi = W.bounds(boxes)
    both = [tuple(a) + tuple(b) for a, b in zip(lo.tolist(), hi.tolist())]
    for box in ((2, 3, 1, 4, 6, 8), (6, 3, 1, 6, 6, 8), (7, 3, 1, 7, 6, 9), (8, 3, 1, 8, 7, 9), (10, 10, 10, 10, 11, 11), (11, 10, 10, 11, 11, 11), (13, 0, 12, 14, 2, 14),
                (15, 0, 12, 15, 0, 14), (15, 1, 12, 15, 1, 12), (15, 1, 14, 15, 1, 14), (15, 2, 12, 15, 2, 14)):
        assert box in both, box
    assert len(both) == 11 and int(result["rects"]) == 3 + 3 + 2 + 2 + 4         # the 3-deep box is three rects, the 2-deep one two
    merged, merged_boxes = W.boxes(grid, any_palette=True)
    assert len(merged_boxes) == 10 and (10, 10, 10, 11, 11, 11) in [tuple(a) + tuple(b) for a, b in zip(*(x.tolist() for x in W.bounds(merged_boxes)))]
    assert int(merged_boxes["palette"][merged_boxes["key"] == (10 << 16) | (10 << 8) | 10][0]) == 1      # the key voxel's
    # a region cuts the box on all three axes; one just behind a box's first slice starts it anew
    cut, cut_boxes = W.boxes(grid, region=((3, 4, 2), (3, 5, 6)))
    assert (int(cut["boxes"]), int(cut["voxels"])) == (1, 10) and cut_boxes[0].tolist() == ((3 << 16) | (4 << 8) | 2, 0, 0, 1, 4)
    late, late_boxes = W.boxes(grid, region=((3, 0, 0), (15, 15, 15)))
    assert late_boxes[0].tolist() == ((3 << 16) | (3 << 8) | 1, 0, 1, 3, 7)
    assert W.boxes(grid, region=((5, 0, 0), (4, 15, 15)))[0].tobytes() == W.zero_result().tobytes()


def test_one_slice_slab_against_the_mesh_witness():
    """on a one-slice slab seen from +x every voxel of S shows its face: the mesh's quads are the slab's rects, and with one slice
    the rects are the boxes"""
    for which, (density, materials) in enumerate(BLOCKS):
        slab = random_block(230 + which, density, materials, shape=(1, 64, 64))
        for any_palette in (False, True):
            result, boxes = W.boxes(slab, axis=0, any_palette=any_palette)
            _, quads = M.mesh(slab, faces=S.POS_X, any_palette=any_palette)
            assert int(result["boxes"]) == int(result["rects"]) == len(quads)
            assert boxes["key"].tolist() == quads["key"].tolist() and boxes["palette"].tolist() == quads["palette"].tolist()
            assert boxes["dz"].tolist() == quads["du"].tolist() and boxes["dy"].tolist() == quads["dv"].tolist() and not boxes["dx"].any()


def test_axes_agree_on_transposed_grids():
    """axis 1 and axis 2 are axis 0 of the grid with its axes permuted to (n, v, u)"""
    grid = random_block(240, 0.9, 2, shape=(20, 24, 28))
    for axis, any_palette in itertools.product((1, 2), (False, True)):
        order = W.AXES[axis]
        result, boxes = W.boxes(grid, axis=axis, any_palette=any_palette)
        turned, turned_boxes = W.boxes(np.ascontiguousarray(np.transpose(grid, order)), axis=0, any_palette=any_palette)
        assert [int(result[k]) for k in ("boxes", "rects", "voxels")] == [int(turned[k]) for k in ("boxes", "rects", "voxels")]
        lo, hi = W.bounds(boxes)
        tlo, thi = W.bounds(turned_boxes)
        assert np.array_equal(lo[:, order], tlo) and np.array_equal(hi[:, order], thi)      # the same boxes in the same order
        assert boxes["palette"].tolist() == turned_boxes["palette"].tolist()
        assert result["lo"][list(order)].tolist() == turned["lo"].tolist() and result["hi"][list(order)].tolist() == turned["hi"].tolist()


def test_refusals_and_zero_result():
    assert W.zero_result().tobytes() == bytes(12) + b"\xff\xff\xff\x00" + bytes(48) and W.RESULT_DTYPE.itemsize == 64 and W.BOX_DTYPE.itemsize == 8
    assert W.QUERY_DTYPE.itemsize == S.QUERY_DTYPE.itemsize == 48
    assert not W.refused(2, 1, 254, (0, 0, 0), (255, 255, 255)) and not W.refused(0, 0, -1, (9, 0, 0), (3, 0, 0))
    for bad in ((3, 0, -1, (0, 0, 0), (1, 1, 1)), (0, 2, -1, (0, 0, 0), (1, 1, 1)), (0, 1 << 31, -1, (0, 0, 0), (1, 1, 1)), (0, 0, -2, (0, 0, 0), (1, 1, 1)),
                (0, 0, 255, (0, 0, 0), (1, 1, 1)), (0, 0, -1, (0, 256, 0), (1, 1, 1)), (0, 0, -1, (0, 0, 0), (1, 1, 256))):
        assert W.refused(*bad), bad
    result, boxes = W.boxes(np.zeros((8, 8, 8), np.uint8))
    assert result.tobytes() == W.zero_result().tobytes() and len(boxes) == 0
    full, one = W.boxes(np.full((256, 256, 256), 7, np.uint8), axis=1)
    assert one.tolist() == [(0, 6, 255, 255, 255)] and (int(full["boxes"]), int(full["rects"]), int(full["voxels"])) == (1, 256, 1 << 24)
