"""The witness of model voxelisation (dust_hip_model_edit_triangles, dust_hip_model_fill_mesh; the contract is in include/dust_hip.h).
A helper module, not a test: tests/test_triangle_witness.py holds it to independent definitions (exact polygon clipping, half-space
membership, the voxels -> faces -> triangles -> voxels round trip), tests/test_triangle_rule.py holds the C++ rule to it and
tests/test_gpu_triangles.py the device.

Written from the header text, literally: the surface rule takes the minimum and the maximum of dot(a, corner) over the cube's eight
corners for each of the 13 axes; the solid rule evaluates the three edge functions and the height test per voxel centre. Per-triangle
quantities are Python ints; the per-voxel arithmetic is numpy int64, which every intermediate fits (below 2^60). The only shortcut is
the set of voxels looked at: those the vertices' extent touches. The grid holds palette index + 1 per voxel, 0 = None, indexed
[x, y, z]."""
import itertools

import numpy as np

EXTENT = 256
UNIT = 256
MAX_COORD = 262144
MAX_EDIT_TRIANGLES = 65536
MAX_MESH_TRIANGLES = 1 << 20
CARVE, FILL, PAINT, PLACE = 0, 1, 2, 3

TRIANGLE_DTYPE = np.dtype([("v", "<i4", (3, 3)), ("op", "<u4"), ("palette", "<i4"), ("reserved", "<u4")])
QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("op", "<u4"), ("palette", "<i4"), ("flags", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3), ("reserved", "<u4", 2)])
RESULT_DTYPE = np.dtype([("covered", "<u4"), ("changed", "<u4"), ("live", "<u4"), ("crossing", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3), ("reserved", "<u4", 2)])
CORNERS = list(itertools.product((0, 1), repeat=3))


def triangles(vertices, op=FILL, palette=0):
    """integer vertices (n, 3, 3) in 1/256 voxel -> TRIANGLE_DTYPE records"""
    v = np.asarray(vertices, np.int64).reshape(-1, 3, 3)
    out = np.zeros(len(v), TRIANGLE_DTYPE)
    out["v"] = v
    out["op"] = np.broadcast_to(np.asarray(op, np.uint32), (len(v),))
    out["palette"] = np.broadcast_to(np.asarray(palette, np.int32), (len(v),))
    return out


def verts(t):
    """a record's (or a (3, 3) array's) vertices as three tuples of Python ints"""
    v = t["v"] if isinstance(t, np.void) or (hasattr(t, "dtype") and t.dtype.names) else t
    return [tuple(int(c) for c in p) for p in np.asarray(v).reshape(3, 3)]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def sub(a, b):
    return tuple(p - q for p, q in zip(a, b))


def normal(v):
    return cross(sub(v[1], v[0]), sub(v[2], v[0]))


def in_range(v):
    return all(abs(c) <= MAX_COORD for p in v for c in p)


def live(v):
    """in range and not degenerate: the triangles that cover anything at all"""
    return in_range(v) and normal(v) != (0, 0, 0)


def refused(tris, limit=MAX_EDIT_TRIANGLES):
    """what edit_triangles refuses with DUST_ERR_INVALID_ARGUMENT before anything changes (beyond null pointers)"""
    t = np.asarray(tris, TRIANGLE_DTYPE).reshape(-1)
    if len(t) > limit:
        return True
    uses = t["op"] != CARVE
    return bool(np.any(t["op"] > PLACE) or np.any(uses & ((t["palette"] < 0) | (t["palette"] > 254))))


def query_refused(op, palette, flags=0, reserved=(0, 0)):
    """what fill_mesh refuses of its query's fields (beyond struct_size)"""
    return op > PLACE or (op != CARVE and not 0 <= palette <= 254) or flags != 0 or any(r != 0 for r in reserved)


def voxel_bounds(v, lo=0, hi=EXTENT - 1):
    """inclusive bounds (lo[3], hi[3]) of the voxels the vertices' extent touches -- a coordinate at exactly 256 k touches voxels k - 1
    and k -- clipped to lo..hi (each a number or one per axis); None when nothing is left"""
    lo, hi = np.broadcast_to(lo, 3).tolist(), np.broadcast_to(hi, 3).tolist()
    out_lo, out_hi = [], []
    for r in range(3):
        cs = [p[r] for p in v]
        l, h = max((min(cs) - 1) // UNIT, lo[r]), min(max(cs) // UNIT, hi[r])     # (// floors, whatever the sign)
        if l > h:
            return None
        out_lo.append(l)
        out_hi.append(h)
    return out_lo, out_hi


def axes(v):
    """the 13 axes of the surface rule"""
    edges = [sub(v[1], v[0]), sub(v[2], v[1]), sub(v[0], v[2])]
    units = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    return units + [normal(v)] + [cross(e, u) for e in edges for u in units]


def covers(v, x, y, z):
    """one voxel, in Python ints throughout: the closed triangle and the closed cube share a point"""
    if not live(v):
        return False
    corners = [(UNIT * (x + i), UNIT * (y + j), UNIT * (z + k)) for i, j, k in CORNERS]
    for a in axes(v):
        tri = [sum(p * q for p, q in zip(a, p_k)) for p_k in v]
        box = [sum(p * q for p, q in zip(a, c)) for c in corners]
        if max(tri) < min(box) or min(tri) > max(box):
            return False
    return True


def coverage(v, lo=0, hi=EXTENT - 1):
    """(bounds lo, bool array over the bounds): the voxels of lo..hi the triangle covers; (None, None) when it covers nothing"""
    if not live(v):
        return None, None
    bounds = voxel_bounds(v, lo, hi)
    if bounds is None:
        return None, None
    b_lo, b_hi = bounds
    ax = [np.arange(b_lo[r], b_hi[r] + 1, dtype=np.int64) * UNIT for r in range(3)]
    base = [ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]]
    apart = np.zeros(tuple(len(a) for a in ax), bool)
    for a in axes(v):
        tri = [sum(p * q for p, q in zip(a, p_k)) for p_k in v]
        at = a[0] * base[0] + a[1] * base[1] + a[2] * base[2]                # dot(a, the cube's lowest corner)
        steps = [UNIT * sum(p * q for p, q in zip(a, c)) for c in CORNERS]    # ... and what each corner adds to it
        apart |= (max(tri) < at + min(steps)) | (min(tri) > at + max(steps))
    return b_lo, ~apart


def covered_voxels(v, lo=0, hi=EXTENT - 1):
    b_lo, m = coverage(v, lo, hi)
    if m is None:
        return set()
    return {(int(x) + b_lo[0], int(y) + b_lo[1], int(z) + b_lo[2]) for x, y, z in np.argwhere(m)}


def apply_op(grid, m, op, palette):
    """the operation on the voxels of mask m (the grid's shape), in place; returns how many changed"""
    byte = np.uint8((int(palette) + 1) & 255)
    if op == CARVE:
        m = m & (grid != 0)
        new = np.uint8(0)
    elif op == FILL:
        m = m & (grid != byte)
        new = byte
    elif op == PAINT:
        m = m & (grid != 0) & (grid != byte)
        new = byte
    else:
        m = m & (grid == 0)
        new = byte
    grid[m] = new
    return int(m.sum())


def edit_triangles(grid, tris):
    """the triangles in array order, in place; returns changed (uint32 per triangle)"""
    t = np.asarray(tris, TRIANGLE_DTYPE).reshape(-1)
    assert not refused(t)
    changed = np.zeros(len(t), np.uint32)
    for i, one in enumerate(t):
        b_lo, m = coverage(verts(one))
        if m is None:
            continue
        view = grid[tuple(slice(b_lo[r], b_lo[r] + m.shape[r]) for r in range(3))]
        changed[i] = apply_op(view, m, int(one["op"]), int(one["palette"]))
    return changed


# ---- the solid rule
def column_crossed(v, px, py):
    """one column, Python ints: the column test of the header"""
    s = (normal(v)[2] > 0) - (normal(v)[2] < 0)
    if s == 0:
        return False
    for a, b in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
        dx, dy = s * (b[0] - a[0]), s * (b[1] - a[1])
        e = dx * (py - a[1]) - dy * (px - a[0])
        if not (e > 0 or (e == 0 and (dy > 0 or (dy == 0 and dx < 0)))):
            return False
    return True


def crossed_above(v, c):
    """is the triangle crossed above the point c (units)?"""
    n = normal(v)
    s = (n[2] > 0) - (n[2] < 0)
    return live(v) and column_crossed(v, c[0], c[1]) and s * sum(p * (q - r) for p, q, r in zip(n, c, v[0])) < 0


def crossing_count(v, px, py):
    """how many of the column's 256 voxel centres the triangle is crossed above (needs n.z != 0; the column test is not applied)"""
    n = normal(v)
    s = (n[2] > 0) - (n[2] < 0)
    cz = np.arange(EXTENT, dtype=np.int64) * UNIT + UNIT // 2
    return int(np.count_nonzero(s * (n[0] * (px - v[0][0]) + n[1] * (py - v[0][1]) + n[2] * (cz - v[0][2])) < 0))


def inside(tris, lo=(0, 0, 0), hi=(255, 255, 255)):
    """bool array over the inclusive region lo..hi: the voxels whose centre has an odd number of triangles crossed above it"""
    lo, hi = [int(c) for c in lo], [int(c) for c in hi]
    shape = tuple(h - l + 1 for l, h in zip(lo, hi))
    odd = np.zeros(shape, bool)
    cz = (np.arange(lo[2], hi[2] + 1, dtype=np.int64) * UNIT + UNIT // 2)[None, None, :]
    for one in np.asarray(tris, TRIANGLE_DTYPE).reshape(-1):
        v = verts(one)
        if not live(v):
            continue
        n = normal(v)
        s = (n[2] > 0) - (n[2] < 0)
        if s == 0:
            continue
        # the columns whose centre lies in the vertices' extent (the only shortcut: every other column fails an edge function)
        x0 = max(-((-(min(p[0] for p in v) - UNIT // 2)) // UNIT), lo[0])
        x1 = min((max(p[0] for p in v) - UNIT // 2) // UNIT, hi[0])
        y0 = max(-((-(min(p[1] for p in v) - UNIT // 2)) // UNIT), lo[1])
        y1 = min((max(p[1] for p in v) - UNIT // 2) // UNIT, hi[1])
        if x0 > x1 or y0 > y1:
            continue
        px = (np.arange(x0, x1 + 1, dtype=np.int64) * UNIT + UNIT // 2)[:, None]
        py = (np.arange(y0, y1 + 1, dtype=np.int64) * UNIT + UNIT // 2)[None, :]
        column = np.ones((x1 - x0 + 1, y1 - y0 + 1), bool)
        for a, b in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
            dx, dy = s * (b[0] - a[0]), s * (b[1] - a[1])
            e = dx * (py - a[1]) - dy * (px - a[0])
            column &= (e > 0) | ((e == 0) & bool(dy > 0 or (dy == 0 and dx < 0)))
        height = s * ((n[0] * (px - v[0][0]) + n[1] * (py - v[0][1]))[:, :, None] + n[2] * (cz - v[0][2])) < 0
        odd[x0 - lo[0]:x1 - lo[0] + 1, y0 - lo[1]:y1 - lo[1] + 1, :] ^= column[:, :, None] & height
    return odd


def zero_result():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["lo"] = 255
    return r


def fill_mesh(grid, tris, op=FILL, palette=0, lo=(0, 0, 0), hi=(255, 255, 255)):
    """the call on a grid, in place -> its DustHipFillMeshResult (RESULT_DTYPE)"""
    t = np.asarray(tris, TRIANGLE_DTYPE).reshape(-1)
    assert len(t) <= MAX_MESH_TRIANGLES and not query_refused(op, palette)
    r = zero_result()
    hi = [min(int(c), EXTENT - 1) for c in hi]
    lo = [int(c) for c in lo]
    if len(t) == 0 or any(l > h for l, h in zip(lo, hi)):
        return r
    alive = [verts(one) for one in t if live(verts(one))]
    r["live"] = len(alive)
    r["crossing"] = sum(1 for v in alive if normal(v)[2] != 0)
    m = inside(t, lo, hi)
    r["covered"] = int(m.sum())
    view = grid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    r["changed"] = apply_op(view, m, op, palette)
    if m.any():
        at = np.argwhere(m)
        r["lo"] = at.min(axis=0) + lo
        r["hi"] = at.max(axis=0) + lo
    return r


# ---- voxels -> faces -> triangles (the round trip's first half)
def face_triangles(solid, offset=(0, 0, 0), rng=None):
    """The exposed unit faces of a bool array (a face between a solid voxel and an empty or outside one), two triangles each, on integer
    voxel corners shifted by `offset` voxels -> (n, 3, 3) int64 in units. rng: shuffle the order, flip random windings and cut each
    face along a random diagonal."""
    solid = np.asarray(solid, bool)
    padded = np.pad(solid, 1)
    out = []
    for axis in range(3):
        u, w = [r for r in range(3) if r != axis]
        for side in (0, 1):
            across = np.roll(padded, -1 if side else 1, axis=axis)[1:-1, 1:-1, 1:-1]
            for p in np.argwhere(solid & ~across):
                base = np.array(p, np.int64) + offset
                base[axis] += side
                du, dw = np.zeros(3, np.int64), np.zeros(3, np.int64)
                du[u], dw[w] = 1, 1
                c = [base, base + du, base + du + dw, base + dw]
                if rng is not None and rng.random() < 0.5:
                    c = c[1:] + c[:1]                                          # the other diagonal
                out += [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
    tri = np.array(out, np.int64).reshape(-1, 3, 3) * UNIT
    if rng is not None and len(tri):
        flip = rng.random(len(tri)) < 0.5
        tri[flip] = tri[flip][:, ::-1]
        tri = tri[rng.permutation(len(tri))]
    return tri
