"""The mesh witness (tests/mesh_witness.py) held to a brute-force reading of the rule of include/dust_hip.h -- per slice every row's
set of runs as Python tuples, a quad where the row above lacks the identical one -- that shares with it only the exposure and the
region of the surface witness, and to hand-counted cases. Also dust_amd.api.mesh_corners on hand-made quads of every face."""
import numpy as np
import pytest

import mesh_witness as W
import surface_witness as S
from dust_amd import api


def brute_force(grid, faces, palette, region, walls, any_palette):
    """the quads as tuples (d, slice, v0, u0, u1, v1, palette of the key voxel), in the documented order"""
    box = S.clip(grid, region)
    exposed = S.exposure(grid, walls)
    quads = []
    for d in range(6):
        if box is None or not (faces >> d) & 1:
            continue
        n_axis, v_axis, u_axis = W.AXES[d >> 1]

        def voxel(s, v, u):
            at = [0, 0, 0]
            at[n_axis], at[v_axis], at[u_axis] = s, v, u
            return tuple(at)

        def in_f(s, v, u):
            x = voxel(s, v, u)
            if any(not cut.start <= c < cut.stop for c, cut in zip(x, box)):
                return False
            byte = int(grid[x])
            return byte != 0 and (palette < 0 or byte == palette + 1) and bool((int(exposed[x]) >> d) & 1)

        for s in range(grid.shape[n_axis]):
            rows = []
            for v in range(grid.shape[v_axis]):
                runs, u = set(), 0
                while u < grid.shape[u_axis]:
                    if not in_f(s, v, u):
                        u += 1
                        continue
                    name = 0 if any_palette else int(grid[voxel(s, v, u)])
                    u1 = u
                    while u1 + 1 < grid.shape[u_axis] and in_f(s, v, u1 + 1) and (any_palette or int(grid[voxel(s, v, u1 + 1)]) == name):
                        u1 += 1
                    runs.add((u, u1, name))
                    u = u1 + 1
                rows.append(runs)
            for v0, runs in enumerate(rows):
                for run in sorted(runs):
                    if v0 > 0 and run in rows[v0 - 1]:
                        continue
                    v1 = v0
                    while v1 + 1 < len(rows) and run in rows[v1 + 1]:
                        v1 += 1
                    quads.append((d, s, v0, run[0], run[1], v1, int(grid[voxel(s, v0, run[0])]) - 1))
    return quads


def as_tuples(quads):
    out = []
    for q in quads:
        key, d = int(q["key"]), int(q["face"])
        xyz = (key >> 16, (key >> 8) & 255, key & 255)
        n_axis, v_axis, u_axis = W.AXES[d >> 1]
        out.append((d, xyz[n_axis], xyz[v_axis], xyz[u_axis], xyz[u_axis] + int(q["du"]), xyz[v_axis] + int(q["dv"]), int(q["palette"])))
    return out


def check(grid, **query):
    result, quads = W.mesh(grid, **query)
    full = dict(faces=63, palette=-1, region=None, walls=False, any_palette=False)
    full.update(query)
    want = brute_force(grid, **full)
    got = as_tuples(quads)
    assert got == want, (query, got[:3], want[:3])
    assert got == sorted(got, key=lambda q: q[:4])                                # face, slice, v0, u0
    surface_query = {k: v for k, v in query.items() if k != "any_palette"}
    surface = S.surface(grid, **surface_query)[0]
    area = (quads["du"].astype(np.int64) + 1) * (quads["dv"].astype(np.int64) + 1)
    assert int(area.sum()) == int(result["faces"]) == int(surface["faces"]) and result["faces_by_face"].tolist() == surface["by_face"].tolist()
    assert int(result["quads"]) == len(quads) == int(result["quads_by_face"].sum()) and int(result["largest"]) == (int(area.max()) if len(area) else 0)
    assert result["quads_by_face"].tolist() == np.bincount(quads["face"], minlength=6).tolist() and int(result["reserved"]) == 0
    covered, twice = W.rasterise(quads, grid.shape)
    box = S.clip(grid, full["region"])
    want_cover = np.zeros(grid.shape, np.uint8)
    if box is not None:
        looked_at = grid[box] != 0 if full["palette"] < 0 else grid[box] == full["palette"] + 1
        want_cover[box] = np.where(looked_at, S.exposure(grid, full["walls"])[box] & np.uint8(full["faces"]), 0)
    assert not twice and np.array_equal(covered, want_cover), query
    return result, quads


@pytest.mark.parametrize("density", [0.3, 0.6, 0.9, 0.97])
def test_random_blocks_against_a_brute_force_reading(density):
    rng = np.random.default_rng(int(density * 100))
    merged = 0
    for materials in (1, 2, 6):
        grid = np.where(rng.random((14, 13, 12)) < density, rng.integers(1, materials + 1, (14, 13, 12)), 0).astype(np.uint8)
        result, quads = check(grid)
        merged += int(result["faces"]) - int(result["quads"])
        check(grid, walls=True)
        anyp, _ = check(grid, any_palette=True)
        assert int(anyp["quads"]) <= int(result["quads"]) and int(anyp["faces"]) == int(result["faces"])
        check(grid, palette=0)
        check(grid, palette=materials - 1, any_palette=True, walls=True)
        check(grid, faces=S.POS_Y | S.NEG_X)
        check(grid, faces=S.NEG_Z, walls=True)
        check(grid, region=((3, 2, 4), (9, 11, 8)))                               # cuts through the block
        check(grid, region=((0, 5, 0), (13, 5, 11)), any_palette=True)            # one slice of y
        check(grid, region=((5, 5, 5), (4, 9, 9)))                                # lo > hi: nothing
    assert merged > 0


def test_hand_counted_cases():
    grid = np.zeros((34, 28, 34), np.uint8)
    grid[5, 6, 7] = 3
    result, quads = check(grid)
    assert (int(result["quads"]), int(result["faces"]), int(result["largest"])) == (6, 6, 1)
    assert quads.tolist() == [((5 << 16) | (6 << 8) | 7, d, 2, 0, 0) for d in range(6)]
    # a 30 x 3 x 30 plate of one material: six quads; with a stripe of another material across it the big faces split in three
    grid[:] = 0
    grid[2:32, 10:13, 2:32] = 8
    result, quads = check(grid)
    assert (int(result["quads"]), int(result["faces"]), int(result["largest"])) == (6, 2 * 900 + 4 * 90, 900)
    top = quads[quads["face"] == 3][0]
    assert (int(top["key"]), int(top["du"]), int(top["dv"])) == ((2 << 16) | (12 << 8) | 2, 29, 29)      # +y: u = z, v = x
    side = quads[quads["face"] == 1][0]
    assert (int(side["key"]), int(side["du"]), int(side["dv"])) == ((31 << 16) | (10 << 8) | 2, 29, 2)   # +x: u = z, v = y
    grid[2:32, 10:13, 15:17] = 9                                                  # the stripe runs along x: it cuts every run along z
    result, _ = check(grid)
    assert result["quads_by_face"].tolist() == [3, 3, 3, 3, 1, 1] and int(result["largest"]) == 30 * 15
    assert int(check(grid, any_palette=True)[0]["quads"]) == 6
    # rows that share u0 but not u1, and u1 but not u0, do not merge; a run under a longer run does not merge
    grid[:] = 0
    for k in range(4):
        grid[3 + k, 20, 5:10 + k] = 1
        grid[3 + k, 25, 5 + k:12] = 1
    result, _ = check(grid, faces=S.POS_Y)
    assert (int(result["quads"]), int(result["faces"])) == (8, sum(5 + k for k in range(4)) + sum(7 - k for k in range(4)))
    # two identical runs of different materials, stacked: one quad only under any_palette
    grid[:] = 0
    grid[3, 20, 5:10], grid[4, 20, 5:10] = 1, 2
    assert int(check(grid, faces=S.POS_Y)[0]["quads"]) == 2 and int(check(grid, faces=S.POS_Y, any_palette=True)[0]["quads"]) == 1
    # the full box: one quad per direction; nothing under walls
    grid[:] = 5
    result, quads = check(grid)
    assert int(result["quads"]) == 6 and quads["du"].tolist() == [33, 33, 33, 33, 27, 27] and quads["dv"].tolist() == [27, 27, 33, 33, 33, 33]
    assert int(result["largest"]) == 34 * 34
    assert W.mesh(grid, walls=True)[0].tobytes() == W.zero_result().tobytes()
    # a 3-D checkerboard: every quad is one face
    grid[:] = 0
    grid[8:24, 8:24, 8:24] = (np.indices((16,) * 3).sum(axis=0) & 1).astype(np.uint8) * 4
    result, _ = check(grid)
    assert int(result["quads"]) == int(result["faces"]) == 6 * 16 ** 3 // 2 and int(result["largest"]) == 1


def test_refusals_are_the_surface_calls_plus_the_flag_bits():
    for flags in (0, 1, 2, 3):
        assert not W.refused(63, flags, -1, (0, 0, 0), (255, 255, 255))
    assert W.refused(63, 4, -1, (0, 0, 0), (255, 255, 255)) and W.refused(63, 1 << 31, -1, (0, 0, 0), (255, 255, 255))
    assert W.refused(0, 0, -1, (0, 0, 0), (0, 0, 0)) and W.refused(64, 0, -1, (0, 0, 0), (0, 0, 0)) and W.refused(1, 0, -2, (0, 0, 0), (0, 0, 0))
    assert W.refused(1, 0, 255, (0, 0, 0), (0, 0, 0)) and W.refused(1, 2, 0, (0, 256, 0), (0, 0, 0)) and not W.refused(1, 2, 0, (9, 0, 0), (3, 0, 0))


def hand_made_quads():
    quads = np.zeros(12, api.MESH_QUAD_DTYPE)
    for d in range(6):
        quads[d] = ((10 << 16) | (20 << 8) | 30, d, 1, 0, 0)                       # one voxel face each
        quads[6 + d] = ((1 << 16) | (2 << 8) | 3, d, 1, 4, 6)                      # 5 along u, 7 along v
    return quads


def test_mesh_corners_positions_normals_and_winding():
    quads = hand_made_quads()
    corners, normals = api.mesh_corners(quads)
    assert corners.dtype == np.int32 and corners.shape == (12, 4, 3) and normals.dtype == np.int8 and normals.shape == (12, 3)
    steps = np.array(S.STEPS)
    assert np.array_equal(normals[:6], steps) and np.array_equal(normals[6:], steps)
    for q, c, n in zip(quads, corners.astype(np.int64), normals.astype(np.int64)):
        d = int(q["face"])
        n_axis, v_axis, u_axis = W.AXES[d >> 1]
        key = int(q["key"])
        voxel = np.array([key >> 16, (key >> 8) & 255, key & 255])
        area = (int(q["du"]) + 1) * (int(q["dv"]) + 1)
        assert np.array_equal(np.cross(c[1] - c[0], c[3] - c[0]), n * area)       # counter-clockwise seen from outside
        assert np.array_equal(c[2] - c[0], (c[1] - c[0]) + (c[3] - c[0]))         # a rectangle
        assert np.all(c[:, n_axis] == voxel[n_axis] + (d & 1))                    # a + face lies on the plane coordinate + 1
        assert c[:, u_axis].min() == voxel[u_axis] and c[:, u_axis].max() == voxel[u_axis] + int(q["du"]) + 1
        assert c[:, v_axis].min() == voxel[v_axis] and c[:, v_axis].max() == voxel[v_axis] + int(q["dv"]) + 1
        assert np.array_equal(c[0], voxel + (d & 1) * np.abs(n))
    assert api.mesh_corners(np.zeros(0, api.MESH_QUAD_DTYPE))[0].shape == (0, 4, 3)
    # the far corner of the tree: positions reach 256
    far = np.array([((255 << 16) | (255 << 8) | 255, 1, 0, 0, 0)], api.MESH_QUAD_DTYPE)
    assert api.mesh_corners(far)[0].max() == 256


def test_rasterising_the_corners_agrees_with_rasterising_the_records():
    rng = np.random.default_rng(7)
    grid = np.where(rng.random((14, 13, 12)) < 0.9, rng.integers(1, 3, (14, 13, 12)), 0).astype(np.uint8)
    for quads in (W.mesh(grid)[1], hand_made_quads()):
        corners, normals = api.mesh_corners(quads)
        covered = np.zeros((40, 40, 40), np.uint8)
        for c, n in zip(corners.astype(np.int64), normals.astype(np.int64)):
            d = int(np.flatnonzero(n)[0]) * 2 + int(n.sum() > 0)
            lo, hi = c.min(axis=0), c.max(axis=0)
            lo[d >> 1] -= d & 1                                                   # the voxels behind the rectangle
            hi[d >> 1] = lo[d >> 1] + 1
            covered[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= np.uint8(1 << d)
        assert np.array_equal(covered, W.rasterise(quads, covered.shape)[0]) and covered.any()
