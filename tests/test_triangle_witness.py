"""The witness of model voxelisation (tests/triangle_witness.py) held to definitions that share nothing with it: the surface rule to
exact clipping of the triangle against the cube in fractions.Fraction (the closed sets share a point iff the clipped polygon is not
empty), the solid rule to half-space membership of convex solids -- on every centre that is not on the solid's boundary; on the rest the
witness must still be deterministic -- and to the round trip voxels -> exposed faces -> triangles -> voxels under shuffled order,
random winding and random diagonals."""
import itertools
from fractions import Fraction

import numpy as np

import triangle_witness as W

U = W.UNIT


def clip(polygon, axis, bound, keep_above):
    """Sutherland-Hodgman against one closed half-space, exact: the polygon may shrink to a segment or a point"""
    out = []
    for k, p in enumerate(polygon):
        q = polygon[(k + 1) % len(polygon)]
        p_in = p[axis] >= bound if keep_above else p[axis] <= bound
        q_in = q[axis] >= bound if keep_above else q[axis] <= bound
        if p_in:
            out.append(p)
        if p_in != q_in:
            t = Fraction(bound - p[axis]) / (q[axis] - p[axis])
            out.append(tuple(a + t * (b - a) for a, b in zip(p, q)))
    return out


def shares_a_point(v, x, y, z):
    polygon = [tuple(Fraction(c) for c in p) for p in v]
    for axis, at in enumerate((x, y, z)):
        polygon = clip(polygon, axis, U * at, True)
        polygon = polygon and clip(polygon, axis, U * (at + 1), False)
        if not polygon:
            return False
    return True


def test_surface_rule_is_exact_clipping():
    rng = np.random.default_rng(11)
    checked = touching = covered = 0
    for step, span in ((256, 5), (128, 4), (64, 3), (1, 3)):
        for _ in range(45):
            v = [tuple(int(c) for c in p) for p in rng.integers(-span * U // step, span * U // step + 1, (3, 3)) * step]
            if W.normal(v) == (0, 0, 0):
                continue
            lo = [(min(p[r] for p in v) - 1) // U - 1 for r in range(3)]
            hi = [max(p[r] for p in v) // U + 1 for r in range(3)]
            got = W.covered_voxels(v, lo, hi)
            for x, y, z in itertools.product(*(range(l, h + 1) for l, h in zip(lo, hi))):
                want = shares_a_point(v, x, y, z)
                assert ((x, y, z) in got) == want, (v, x, y, z)
                checked += 1
                covered += want
                # touching: covered, but not by the cube shrunk by one unit on every side (two half-unit steps)
                if want and step >= 64:
                    shrunk = [tuple(2 * c for c in p) for p in v]
                    polygon = [tuple(Fraction(c) for c in p) for p in shrunk]
                    for axis, at in enumerate((x, y, z)):
                        polygon = polygon and clip(polygon, axis, 2 * U * at + 1, True)
                        polygon = polygon and clip(polygon, axis, 2 * U * (at + 1) - 1, False)
                    touching += not polygon
    assert checked > 15000 and covered > 3000 and touching > 300


def signed_volume(a, b, c, d):
    m = [[q - p for p, q in zip(a, x)] for x in (b, c, d)]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def convex_faces(points):
    """the triangles of the convex hull of a few points in general position (brute force: a face has every other point on one side)"""
    faces = []
    for a, b, c in itertools.combinations(points, 3):
        sides = [signed_volume(a, b, c, p) for p in points if p not in (a, b, c)]
        if all(s > 0 for s in sides) or all(s < 0 for s in sides):
            faces.append((a, b, c, 1 if sides[0] > 0 else -1))
    return faces


def check_solid(points, rng, lo, hi):
    """the witness on the hull's triangles against half-space membership; returns (strictly inside, on the boundary)"""
    faces = convex_faces(points)
    tri = np.array([[a, b, c] for a, b, c, _ in faces], np.int64)
    got = W.inside(W.triangles(tri), lo, hi)
    flipped = tri[rng.permutation(len(tri))]
    turn = rng.random(len(flipped)) < 0.5
    flipped[turn] = flipped[turn][:, ::-1]
    again = W.inside(W.triangles(flipped), lo, hi)
    assert np.array_equal(got, again)                                        # order and winding do not matter, boundary centres included
    inside = boundary = 0
    for x, y, z in itertools.product(*(range(l, h + 1) for l, h in zip(lo, hi))):
        c = (U * x + 128, U * y + 128, U * z + 128)
        sides = [side * signed_volume(a, b, q, c) for a, b, q, side in faces]
        if any(s == 0 for s in sides):
            boundary += 1
            continue
        want = all(s > 0 for s in sides)
        assert bool(got[x - lo[0], y - lo[1], z - lo[2]]) == want, (points, x, y, z)
        inside += want
    return inside, boundary


def test_solid_rule_is_half_space_membership_of_convex_solids():
    rng = np.random.default_rng(12)
    inside = boundary = 0
    c = 5 * U + 128                                                           # an octahedron with its vertices on voxel centres
    octahedron = [(c - 4 * U, c, c), (c + 4 * U, c, c), (c, c - 4 * U, c), (c, c + 4 * U, c), (c, c, c - 4 * U), (c, c, c + 4 * U)]
    faces = [(octahedron[i], octahedron[2 + j], octahedron[4 + k]) for i in range(2) for j in range(2) for k in range(2)]
    got = W.inside(W.triangles(np.array(faces, np.int64)), (0, 0, 0), (11, 11, 11))
    for x, y, z in itertools.product(range(12), repeat=3):
        d = abs(x - 5) + abs(y - 5) + abs(z - 5)
        if d != 4:                                                            # (d == 4: the centre is on the surface)
            assert bool(got[x, y, z]) == (d < 4)
            inside += d < 4
    done = 0
    while done < 40:                                                          # tetrahedra on the lattice of centres and voxel corners
        points = [tuple(int(v) for v in p) for p in rng.integers(0, 15, (4, 3)) * 128]
        if signed_volume(*points) == 0:
            continue
        i, b = check_solid(points, rng, (-1, -1, -1), (8, 8, 8))
        inside += i
        boundary += b
        done += 1
    assert inside > 200 and boundary > 50


def test_round_trip_voxels_faces_triangles_voxels():
    rng = np.random.default_rng(13)
    solid = rng.random((8, 8, 8)) < 0.45
    want = np.zeros((12, 12, 12), bool)
    want[2:10, 2:10, 2:10] = solid
    for _ in range(3):
        tri = W.face_triangles(solid, (13, 61, 2), rng)                       # (the box 13..20 x 61..68 x 2..9: across 15 | 16 and 63 | 64)
        assert np.array_equal(W.inside(W.triangles(tri), (11, 59, 0), (22, 70, 11)), want)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[14, 62, 3] = 9
    result = W.fill_mesh(grid, W.triangles(tri), W.PLACE, 4)
    assert int(result["covered"]) == int(solid.sum()) and int(result["changed"]) == int(solid.sum()) - int(solid[1, 1, 1])
    assert int(result["live"]) == len(tri) and 0 < int(result["crossing"]) < len(tri)
    assert np.array_equal(grid[13:21, 61:69, 2:10] != 0, solid | (np.indices((8, 8, 8)) == 1).all(axis=0)) and grid[14, 62, 3] == 9
    at = np.argwhere(solid)
    assert result["lo"].tolist() == (at.min(axis=0) + (13, 61, 2)).tolist() and result["hi"].tolist() == (at.max(axis=0) + (13, 61, 2)).tolist()
    # a region that cuts the mesh, the empty region, an open mesh (its parity, whatever that is, twice the same)
    cut = W.fill_mesh(np.zeros((256,) * 3, np.uint8), W.triangles(tri), W.FILL, 1, (15, 0, 0), (17, 255, 5))
    assert int(cut["covered"]) == int(solid[2:5, :, :4].sum())
    assert W.fill_mesh(grid, W.triangles(tri), W.FILL, 1, (5, 5, 5), (4, 9, 9)).tobytes() == W.zero_result().tobytes()
    open_mesh = W.triangles(tri[: len(tri) // 2])
    assert np.array_equal(W.inside(open_mesh, (11, 59, 0), (22, 70, 11)), W.inside(open_mesh[::-1], (11, 59, 0), (22, 70, 11)))


def test_edit_order_operations_and_counts():
    grid = np.zeros((256,) * 3, np.uint8)
    a = [(2 * U + 10, 2 * U + 10, 2 * U + 10), (4 * U + 10, 2 * U + 10, 2 * U + 10), (2 * U + 10, 4 * U + 10, 2 * U + 10)]
    tris = W.triangles([a, a, a, a, a], [W.FILL, W.PAINT, W.PLACE, W.CARVE, W.PAINT], [3, 4, 5, 0, 6])
    n = len(W.covered_voxels(a))
    assert W.edit_triangles(grid, tris).tolist() == [n, n, 0, n, 0] and not grid.any() and n >= 4
    dead = W.triangles([[(0, 0, 0), (U, U, U), (2 * U, 2 * U, 2 * U)], [(W.MAX_COORD + 1, 0, 0), (0, U, 0), (0, 0, U)]], W.FILL, 1)
    assert W.edit_triangles(grid, dead).tolist() == [0, 0] and not grid.any()
    assert W.refused(W.triangles([a], 4, 0)) and W.refused(W.triangles([a], W.FILL, 255)) and not W.refused(W.triangles([a], W.CARVE, 255))
    assert W.query_refused(4, 0) and W.query_refused(W.FILL, -1) and W.query_refused(W.FILL, 0, 1) and W.query_refused(W.FILL, 0, 0, (0, 1))
    assert not W.query_refused(W.CARVE, -7)
