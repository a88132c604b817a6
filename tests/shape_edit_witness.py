"""The numpy witness of the shape edits (dust_hip_model_edit_shapes; the contract is in include/dust_hip.h). A helper module, not a
test: tests/test_shape_edit_witness.py checks it on hand-built cases, tests/test_gpu_shape_edit.py holds the device to it.

Written from the header text: a shape covers voxel (x, y, z) when it contains the centre c = (x + 0.5, y + 0.5, z + 0.5); the
membership formulas are evaluated in numpy float32, operation by operation (every float32 +, -, *, / of numpy rounds to nearest
and nothing is fused). The only shortcut is the region the formulas are evaluated over: the shape's extent in float64, grown by
PAD = 4 voxels on every side and clipped to the tree -- far more than float32 rounding can move a boundary (below a tenth of a
voxel for coordinates up to 65 536), and more than any bound the device may cull by. The grid holds palette index + 1 per voxel,
0 = None, indexed [x, y, z]."""
import numpy as np

F = np.float32
EXTENT = 256
BOX, SPHERE, CAPSULE = 0, 1, 2
CARVE, FILL, PAINT, PLACE = 0, 1, 2, 3
MAX_SHAPES = 65536
PAD = 4
LIMIT = F(65536.0)   # spheres and capsules: no |coordinate| or radius above this

SHAPE_DTYPE = np.dtype([("a", "<f4", 3), ("kind", "<u4"), ("b", "<f4", 3), ("radius", "<f4"), ("op", "<u4"), ("palette", "<i4"),
                        ("reserved", "<u4", 2)])


def shape(kind, a, b=None, radius=0.0, op=CARVE, palette=0):
    s = np.zeros(1, SHAPE_DTYPE)[0]
    s["kind"], s["a"], s["b"], s["radius"], s["op"], s["palette"] = kind, a, (a if b is None else b), radius, op, palette
    return s


def shapes(*records):
    return np.array(list(records), SHAPE_DTYPE)


def refused(shape_array):
    """what the call refuses with DUST_ERR_INVALID_ARGUMENT before anything changes (beyond null pointers)"""
    s = np.asarray(shape_array, SHAPE_DTYPE).reshape(-1)
    if len(s) > MAX_SHAPES:
        return True
    uses_palette = s["op"] != CARVE
    return bool(np.any(s["kind"] > CAPSULE) or np.any(s["op"] > PLACE) or np.any(uses_palette & ((s["palette"] < 0) | (s["palette"] > 254))))


def covers_nothing(s):
    a, b, r, kind = s["a"], s["b"], s["radius"], int(s["kind"])
    if kind == BOX:
        return not (np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(a <= b))
    used = [a, np.array([r])] + ([b] if kind == CAPSULE else [])
    if not all(np.all(np.isfinite(u)) for u in used):
        return True
    if r < 0:
        return True
    return bool(any(np.any(np.abs(u) > LIMIT) for u in used))


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def region(s):
    """three slices: the voxels whose centres lie within PAD voxels of the shape's extent (float64), clipped to the tree"""
    a, b = np.asarray(s["a"], np.float64), np.asarray(s["b"], np.float64)
    if int(s["kind"]) == BOX:
        lo, hi = a, b
    else:
        if int(s["kind"]) == SPHERE:
            b = a
        lo, hi = np.minimum(a, b) - float(s["radius"]), np.maximum(a, b) + float(s["radius"])
    lo = np.clip(np.floor(lo) - PAD, 0, EXTENT)
    hi = np.clip(np.ceil(hi) + PAD, 0, EXTENT)
    return tuple(slice(int(l), int(max(l, h))) for l, h in zip(lo, hi))


def coverage(s):
    """(region, bool array over it): the voxels whose centre the shape contains; shapes are clipped to the tree"""
    if covers_nothing(s):
        return (slice(0, 0),) * 3, np.zeros((0, 0, 0), bool)
    reg = region(s)
    shp = tuple(r.stop - r.start for r in reg)
    ax = [(np.arange(r.start, r.stop, dtype=F) + F(0.5)).astype(F) for r in reg]
    c = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
    a = [F(t) for t in s["a"]]
    b = [F(t) for t in s["b"]]
    kind = int(s["kind"])
    if kind == BOX:
        per_axis = [(a[r] <= c[r]) & (c[r] <= b[r]) for r in range(3)]
        return reg, np.broadcast_to(per_axis[0] & per_axis[1] & per_axis[2], shp).copy()
    rr = F(s["radius"]) * F(s["radius"])
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        ap = [np.broadcast_to((c[r] - a[r]).astype(F), shp) for r in range(3)]
        if kind == SPHERE:
            return reg, _dot(ap, ap) <= rr
        ab = [F(b[r] - a[r]) for r in range(3)]
        l = F(_dot(ab, ab))
        if l == 0:
            h = np.zeros(shp, F)
        else:
            h = np.minimum(np.maximum((_dot(ap, ab) / l).astype(F), F(0)), F(1)).astype(F)
        q = [(ap[r] - (ab[r] * h).astype(F)).astype(F) for r in range(3)]
        return reg, _dot(q, q) <= rr


def covered_voxels(s):
    """the covered voxels as a set of (x, y, z)"""
    reg, m = coverage(s)
    return {(int(x) + reg[0].start, int(y) + reg[1].start, int(z) + reg[2].start) for x, y, z in np.argwhere(m)}


def to_grid(vox):
    g = np.zeros((EXTENT,) * 3, np.uint8)
    if vox:
        k = np.array(list(vox.keys()), np.int64)
        g[k[:, 0], k[:, 1], k[:, 2]] = np.array(list(vox.values()), np.int64) + 1
    return g


def to_dict(grid):
    idx = np.argwhere(grid != 0)
    vals = grid[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.int64) - 1
    return {(int(x), int(y), int(z)): int(v) for (x, y, z), v in zip(idx, vals)}


def apply_to_grid(grid, shape_array):
    """the shapes in array order, in place; returns changed (uint32 per shape)"""
    s = np.asarray(shape_array, SHAPE_DTYPE).reshape(-1)
    assert not refused(s)
    changed = np.zeros(len(s), np.uint32)
    for i, one in enumerate(s):
        if covers_nothing(one):
            continue
        reg, m = coverage(one)
        full, grid = grid, grid[reg]   # (a view: the writes below land in the caller's grid)
        op, byte = int(one["op"]), np.uint8((int(one["palette"]) + 1) & 255)
        if op == CARVE:
            m &= grid != 0
            new = np.uint8(0)
        elif op == FILL:
            m &= grid != byte
            new = byte
        elif op == PAINT:
            m &= (grid != 0) & (grid != byte)
            new = byte
        else:
            m &= grid == 0
            new = byte
        changed[i] = int(m.sum())
        grid[m] = new
        grid = full
    return changed


def apply(vox, shape_array):
    """voxel dict {(x, y, z): palette index} and a shape array -> (the new dict, changed)"""
    grid = to_grid(vox)
    changed = apply_to_grid(grid, shape_array)
    return to_dict(grid), changed


def edit_list(before_grid, after_grid):
    """the (xyz, values) a set_voxels call needs to take one grid to the other (values: palette index, or -1 to clear)"""
    idx = np.argwhere(before_grid != after_grid)
    vals = after_grid[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.int32) - 1
    return idx.astype(np.uint32), vals
