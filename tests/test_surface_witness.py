"""The surface witness (tests/surface_witness.py) held to hand-counted cases and to a per-voxel Python loop that shares nothing with
it but the contract of include/dust_hip.h."""
import numpy as np

import surface_witness as W


def empty():
    return np.zeros((256,) * 3, np.uint8)


def test_one_voxel_has_six_faces():
    grid = empty()
    grid[100, 101, 102] = 7
    result, voxels, counts = W.surface(grid)
    assert (int(result["voxels"]), int(result["faces"]), int(result["solid"])) == (1, 6, 1) and result["by_face"].tolist() == [1] * 6
    assert result["lo"].tolist() == result["hi"].tolist() == [100, 101, 102]
    assert voxels.tolist() == [((100 << 16) | (101 << 8) | 102, 63, 6, 0)]
    assert counts[:, 7].tolist() == [1] * 6 and int(counts.sum()) == 6
    # one direction at a time, and a filter that lets nothing through
    for d in range(6):
        r, v, c = W.surface(grid, faces=1 << d)
        assert (int(r["voxels"]), int(r["faces"])) == (1, 1) and int(v["faces"][0]) == 1 << d and int(c[d, 7]) == 1 and int(c.sum()) == 1
    r, v, c = W.surface(grid, palette=5)
    assert r.tobytes() == W.zero_result().tobytes() and len(v) == 0 and not c.any()


def test_two_voxels_sharing_a_face_have_ten():
    for axis in range(3):
        grid = empty()
        a, b = [3, 7, 11], [3, 7, 11]
        b[axis] += 1                 # across a brick edge on x (3 | 4), inside a brick on z
        grid[tuple(a)], grid[tuple(b)] = 1, 2
        result, voxels, counts = W.surface(grid)
        assert (int(result["voxels"]), int(result["faces"])) == (2, 10)
        assert result["by_face"].tolist() == [1 if d // 2 == axis else 2 for d in range(6)]      # the shared face is hidden on both sides
        assert sorted(int(f) for f in voxels["faces"]) == sorted([63 & ~(2 << (2 * axis)), 63 & ~(1 << (2 * axis))])
        assert int(counts[:, 1].sum()) == 5 and int(counts[:, 2].sum()) == 5


def test_full_brick_shows_96_faces_on_56_voxels():
    grid = empty()
    grid[8:12, 12:16, 16:20] = 3
    result, voxels, counts = W.surface(grid)
    assert (int(result["voxels"]), int(result["faces"]), int(result["solid"])) == (56, 96, 64) and result["by_face"].tolist() == [16] * 6
    assert result["lo"].tolist() == [8, 12, 16] and result["hi"].tolist() == [11, 15, 19]
    # one brick: the list is in ascending voxel bit, the eight inner voxels missing
    bits = [((k >> 16) & 3) << 4 | ((k >> 8) & 3) << 2 | (k & 3) for k in voxels["key"].tolist()]
    inner = {(x << 4) | (y << 2) | z for x in (1, 2) for y in (1, 2) for z in (1, 2)}
    assert bits == [b for b in range(64) if b not in inner]


def test_full_tree_and_walls():
    grid = np.full((256,) * 3, 9, np.uint8)
    result, voxels, counts = W.surface(grid)
    assert int(result["voxels"]) == 256 ** 3 - 254 ** 3 == 390152 and int(result["faces"]) == 393216 and result["by_face"].tolist() == [65536] * 6
    assert int(result["solid"]) == 1 << 24 and int(counts[:, 9].sum()) == 393216
    result, voxels, counts = W.surface(grid, walls=True)
    assert (int(result["voxels"]), int(result["faces"]), int(result["solid"])) == (0, 0, 1 << 24) and len(voxels) == 0 and not counts.any()
    assert result["lo"].tolist() == [255] * 3 and result["hi"].tolist() == [0] * 3


def test_block_order_is_cells_then_bricks_then_voxels():
    assert W.block_order(0, 0, 0) == 0 and W.block_order(0, 0, 1) == 1 and W.block_order(0, 1, 0) == 4 and W.block_order(1, 0, 0) == 16
    assert W.block_order(0, 0, 4) == 64 and W.block_order(0, 4, 0) == 4 * 64 and W.block_order(4, 0, 0) == 16 * 64
    assert W.block_order(0, 0, 16) == 4096 and W.block_order(0, 16, 0) == 16 * 4096 and W.block_order(16, 0, 0) == 256 * 4096
    assert W.block_order(255, 255, 255) == (1 << 24) - 1


def loop_surface(grid, faces, palette, lo, hi, walls):
    """voxel by voxel: -> {(x, y, z): faces byte} of the listed voxels, and the solid count"""
    n = grid.shape[0]
    listed, solid = {}, 0
    for x in range(max(lo[0], 0), min(hi[0], n - 1) + 1):
        for y in range(max(lo[1], 0), min(hi[1], n - 1) + 1):
            for z in range(max(lo[2], 0), min(hi[2], n - 1) + 1):
                g = int(grid[x, y, z])
                if g == 0 or (palette >= 0 and g != palette + 1):
                    continue
                solid += 1
                byte = 0
                for d, (sx, sy, sz) in enumerate(W.STEPS):
                    p = (x + sx, y + sy, z + sz)
                    if all(0 <= c < n for c in p):
                        across = grid[p] != 0
                    else:
                        across = walls
                    if not across and (faces >> d) & 1:
                        byte |= 1 << d
                if byte:
                    listed[(x, y, z)] = byte
    return listed, solid


def test_random_block_against_a_per_voxel_loop():
    rng = np.random.default_rng(91)
    grid = np.where(rng.random((12,) * 3) < 0.6, rng.integers(1, 4, (12,) * 3), 0).astype(np.uint8)
    cases = [(63, -1, (0, 0, 0), (11, 11, 11), False), (63, -1, (0, 0, 0), (11, 11, 11), True), (8, -1, (0, 0, 0), (11, 11, 11), False),
             (63, 1, (0, 0, 0), (11, 11, 11), False), (21, 2, (2, 3, 1), (9, 5, 10), True), (42, -1, (5, 5, 5), (6, 300, 6), False),
             (1, -1, (0, 0, 0), (0, 11, 11), True), (63, -1, (7, 0, 0), (6, 11, 11), False)]
    for faces, palette, lo, hi, walls in cases:
        want, want_solid = loop_surface(grid, faces, palette, lo, hi, walls)
        result, voxels, counts = W.surface(grid, faces, palette, (lo, hi), walls)
        got = {(int(k) >> 16, (int(k) >> 8) & 255, int(k) & 255): int(f) for k, f in zip(voxels["key"], voxels["faces"])}
        assert got == want and int(result["solid"]) == want_solid and int(result["voxels"]) == len(want)
        assert int(result["faces"]) == sum(bin(f).count("1") for f in want.values()) == int(counts.sum())
        assert all(int(p) + 1 == int(grid[c]) for c, p in zip(got, voxels["palette"]))
        order = [int(W.block_order(*c)) for c in got]
        assert order == sorted(order)
        for d in range(6):
            for p in range(3):
                assert int(counts[d, 1 + p]) == sum(1 for c, f in want.items() if (f >> d) & 1 and int(grid[c]) == p + 1)
        if want:
            assert result["lo"].tolist() == [min(c[r] for c in want) for r in range(3)] and result["hi"].tolist() == [max(c[r] for c in want) for r in range(3)]
        else:
            assert result["lo"].tolist() == [255] * 3 and result["hi"].tolist() == [0] * 3
    # erosion: None on everything listed takes exactly the voxels with an open face
    after, changed = W.apply(grid, -1)
    want, _ = loop_surface(grid, 63, -1, (0, 0, 0), (11, 11, 11), False)
    assert changed == len(want) and np.count_nonzero(after) == np.count_nonzero(grid) - len(want) and all(after[c] == 0 for c in want)
    same, changed = W.apply(grid, 0, palette=0)
    assert changed == 0 and np.array_equal(same, grid)
