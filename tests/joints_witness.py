"""The numpy witness of the model joints (dust_hip_model_joints; the contract is in include/dust_hip.h). A helper module, not a test:
tests/test_joints_witness.py checks it against a per-face loop, identities and hand-made cases, tests/test_gpu_joints.py holds the
device to it.

Written from the header text, whole-array: a voxel EXISTS when it is solid and lies inside the inclusive region clipped to the tree; its
group is its palette index (MATERIALS) or its cell of the standing fracture, REST where it answers NO_CELL (CELLS). Per axis one shifted
compare finds the faces -- both voxels exist, the groups differ --, np.unique over the packed pair keys names the records and reduceat
sums them. The grid holds palette index + 1 per voxel, 0 = None, indexed [x, y, z]; labels are an array of the grid's shape with cell
indices and NO_CELL (tests/fracture_witness.py `labels`)."""
import numpy as np

MATERIALS, CELLS = 0, 1
REST = 0xFFFF
NO_CELL = 0xFFFF
EXTENT = 256
QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("group", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                        ("reserved", "<u4", 2)])
JOINT_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("faces", "<u4"), ("reserved0", "<u4"), ("by_face", "<u4", 6), ("lo2", "<u2", 3), ("hi2", "<u2", 3),
                        ("reserved1", "<u4"), ("sum2", "<u8", 3)])


def refused(group=MATERIALS, flags=0, palette=-1, reserved=(0, 0)):
    """what the call refuses with DUST_ERR_INVALID_ARGUMENT beyond null pointers and struct_size (any region is legal: it is clipped)"""
    return bool(group > CELLS or flags != 0 or any(reserved) or palette != -1)


def clip(region):
    """(lo, hi) clipped to the tree as dust_hip_model_columns clips it, or None for the empty region"""
    lo, hi = ((0, 0, 0), (EXTENT - 1,) * 3) if region is None else region
    lo, hi = [int(v) for v in lo], [min(int(v), EXTENT - 1) for v in hi]
    return None if any(a > b for a, b in zip(lo, hi)) else (lo, hi)


def pair_key(a, b):
    """the records' order: ascending (a, b), REST (the largest 16-bit value) last"""
    return a * 65536 + b


def faces(grid, group, labels=None, region=None):
    """every face of a call, one row each: (key, direction 0..5, centre x, y, z in half voxels), in no order"""
    grid = np.asarray(grid)
    box = clip(region)
    rows = np.zeros((0, 5), np.int64)
    if box is None:
        return rows
    exists = np.zeros(grid.shape, bool)
    (x0, y0, z0), (x1, y1, z1) = box
    exists[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = grid[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] != 0
    if not exists.any():
        return rows
    # the bounding box of what exists: nothing outside it takes part
    spans = [np.flatnonzero(exists.any(axis=tuple(a for a in range(3) if a != r))) for r in range(3)]
    sub = tuple(slice(int(s[0]), int(s[-1]) + 1) for s in spans)
    origin = np.array([s.start for s in sub], np.int64)
    exists = exists[sub]
    of = (grid[sub].astype(np.int64) - 1) if group == MATERIALS else np.asarray(labels)[sub].astype(np.int64)   # (NO_CELL is REST)
    out = [rows]
    for r in range(3):
        lower = tuple(slice(0, -1) if k == r else slice(None) for k in range(3))
        upper = tuple(slice(1, None) if k == r else slice(None) for k in range(3))
        g, n = of[lower], of[upper]
        p = np.argwhere(exists[lower] & exists[upper] & (g != n))
        if len(p) == 0:
            continue
        at = (p[:, 0], p[:, 1], p[:, 2])
        g, n = g[at], n[at]
        centre = 2 * (p + origin) + 1
        centre[:, r] += 1
        direction = 2 * r + (g < n)                       # the lower voxel is a: from a to b is +r
        out.append(np.column_stack([pair_key(np.minimum(g, n), np.maximum(g, n)), direction, centre]))
    return np.concatenate(out)


def records_of(rows):
    """the JOINT_DTYPE records of a list of faces, in key order"""
    if len(rows) == 0:
        return np.zeros(0, JOINT_DTYPE)
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    keys, starts, counts = np.unique(rows[:, 0], return_index=True, return_counts=True)
    out = np.zeros(len(keys), JOINT_DTYPE)
    out["a"], out["b"], out["faces"] = keys >> 16, keys & 0xFFFF, counts
    which = np.repeat(np.arange(len(keys)), counts)
    out["by_face"] = np.bincount(which * 6 + rows[:, 1], minlength=6 * len(keys)).reshape(-1, 6)
    for k in range(3):
        c = rows[:, 2 + k]
        out["lo2"][:, k] = np.minimum.reduceat(c, starts)
        out["hi2"][:, k] = np.maximum.reduceat(c, starts)
        out["sum2"][:, k] = np.add.reduceat(c, starts)
    return out


def joints(grid, group, labels=None, region=None):
    """the records of a call, all of them"""
    assert not refused(group)
    return records_of(faces(grid, group, labels, region))


def slab_case(axis, at=15, first=3, n=40):
    """a slab two voxels thick, index 2 in the layer at `at` and index 1 in the layer above it, `first`..`first + n - 1` on the other two
    axes: the grid and the one record it has, in closed form"""
    grid = np.zeros((256,) * 3, np.uint8)
    low = [slice(first, first + n)] * 3
    high = list(low)
    low[axis], high[axis] = at, at + 1
    grid[tuple(low)], grid[tuple(high)] = 3, 2
    rec = np.zeros(1, JOINT_DTYPE)[0]
    rec["a"], rec["b"], rec["faces"] = 1, 2, n * n
    rec["by_face"][2 * axis] = n * n                                         # the a voxel is the upper one: toward b is -axis
    for k in range(3):
        if k == axis:
            rec["lo2"][k] = rec["hi2"][k] = 2 * at + 2
            rec["sum2"][k] = n * n * (2 * at + 2)
        else:
            rec["lo2"][k], rec["hi2"][k] = 2 * first + 1, 2 * (first + n - 1) + 1
            rec["sum2"][k] = n * sum(2 * v + 1 for v in range(first, first + n))
    return grid, rec
