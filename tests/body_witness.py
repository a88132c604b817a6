"""The numpy witness of the model bodies (dust_hip_model_bodies; the contract is in include/dust_hip.h). A helper module, not a test:
tests/test_body_witness.py checks it against a per-voxel loop and identities, tests/test_gpu_bodies.py holds the device to it.

Written from the header text, whole-array: a voxel COUNTS when it is solid, lies inside the inclusive region, passes the palette filter
and belongs to a group of the chosen kind; per group the counted voxels, their bounds, and with w = weights[palette index] the sums of
w, of w x, w y, w z and of w xx, w yy, w zz, w xy, w yz, w zx over the integer coordinates, in np.uint64. The grid holds palette index
+ 1 per voxel, 0 = None, indexed [x, y, z]; it may be smaller than the tree. Labels are an array of the grid's shape: island keys with
NO_ISLAND where there is none (tests/island_witness.py `label`), or cell indices with NO_CELL (tests/fracture_witness.py `labels`)."""
import numpy as np

ALL, MATERIALS, ISLANDS, CELLS = 0, 1, 2, 3
WEIGHTS = 255
NO_ISLAND = 0xFFFFFFFF
NO_CELL = 0xFFFF
QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("group", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                        ("reserved", "<u4", 2)])
BODY_DTYPE = np.dtype([("key", "<u4"), ("voxels", "<u4"), ("lo", "u1", 3), ("reserved0", "u1"), ("hi", "u1", 3), ("reserved1", "u1"), ("mass", "<u8"),
                       ("m1", "<u8", 3), ("m2", "<u8", 6)])
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0))   # m2's order: xx, yy, zz, xy, yz, zx


def refused(group=ALL, flags=0, palette=-1, region=None, reserved=(0, 0)):
    """what the call refuses with DUST_ERR_INVALID_ARGUMENT beyond null pointers and struct_size"""
    lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
    return bool(group > CELLS or flags != 0 or any(reserved) or palette < -1 or palette > 254 or any(v >= 256 for v in (*lo, *hi)))


def zero_record(key=0):
    r = np.zeros(1, BODY_DTYPE)[0]
    r["key"] = key
    r["lo"] = 255
    return r


def voxel_list(grid, labels=None):
    """(xyz, byte, label) of a grid's solid voxels: everything a call looks at. A test that asks many questions of one grid makes
    the list once and passes it to `bodies` in the grid's place."""
    grid = np.asarray(grid)
    xyz = np.argwhere(grid != 0)
    at = (xyz[:, 0], xyz[:, 1], xyz[:, 2])
    return xyz, grid[at], (None if labels is None else np.asarray(labels)[at])


def counted(xyz, byte, palette=-1, region=None):
    """which of the solid voxels lie inside the region and pass the filter"""
    m = np.ones(len(xyz), bool)
    if palette >= 0:
        m &= byte == palette + 1
    if region is not None:
        lo, hi = (np.asarray(v, np.int64) for v in region)
        m &= np.all((xyz >= lo) & (xyz <= hi), axis=1)                            # (lo > hi on an axis: nothing)
    return m


def record_of(key, xyz, w):
    """one group: xyz (n, 3) integer coordinates of its counted voxels, w (n,) their weights"""
    r = zero_record(key)
    if len(xyz) == 0:
        return r
    xyz, w = xyz.astype(np.uint64), w.astype(np.uint64)
    r["voxels"] = len(xyz)
    r["lo"], r["hi"] = xyz.min(axis=0), xyz.max(axis=0)
    r["mass"] = w.sum(dtype=np.uint64)
    r["m1"] = (w[:, None] * xyz).sum(axis=0, dtype=np.uint64)
    r["m2"] = [(w * xyz[:, a] * xyz[:, b]).sum(dtype=np.uint64) for a, b in PAIRS]
    return r


def bodies(grid, group=ALL, weights=None, palette=-1, region=None, labels=None, keys=None):
    """The records of a call. `grid` a grid, or the voxel_list of one (then `labels` is the list's). ISLANDS: `labels` the island keys
    per voxel, `keys` the standing islands' keys in ascending order (None: the keys that occur in `labels`). CELLS: `labels` the cell
    index per voxel, `keys` the number of seeds."""
    assert not refused(group, 0, palette, region)
    xyz, byte, word = grid if isinstance(grid, tuple) else voxel_list(grid, labels)
    m = counted(xyz, byte, palette, region)
    table = np.ones(256, np.uint64) if weights is None else np.concatenate([[0], np.asarray(weights, np.uint64).reshape(WEIGHTS)])
    if group == ALL:
        names, of = [0], np.zeros(len(xyz), np.int64)
    elif group == MATERIALS:
        names, of = list(range(WEIGHTS)), byte.astype(np.int64) - 1
    elif group == ISLANDS:
        names = sorted(int(k) for k in np.unique(word[word != NO_ISLAND])) if keys is None else [int(k) for k in keys]
        of = word.astype(np.int64)
        m = m & (word != NO_ISLAND)
    else:
        names, of = list(range(int(keys))), word.astype(np.int64)
        m = m & (word != NO_CELL)
    xyz, of, w = xyz[m], of[m], table[byte[m]]
    order = np.argsort(of, kind="stable")
    xyz, of, w = xyz[order], of[order], w[order]
    out = np.zeros(len(names), BODY_DTYPE)
    for i, key in enumerate(names):
        a, b = np.searchsorted(of, key, "left"), np.searchsorted(of, key, "right")
        out[i] = record_of(key, xyz[a:b], w[a:b])
    return out


def translate(records, by):
    """the records of the same pieces moved by the integer vector `by`: the parallel-axis formulas on the raw sums"""
    out = np.array(records, BODY_DTYPE).reshape(-1).copy()
    t = [int(v) for v in by]
    for r in out:
        if r["voxels"] == 0:
            continue
        m, m1, m2 = int(r["mass"]), [int(v) for v in r["m1"]], [int(v) for v in r["m2"]]
        r["lo"], r["hi"] = r["lo"] + np.array(t), r["hi"] + np.array(t)
        r["m1"] = [m1[a] + t[a] * m for a in range(3)]
        r["m2"] = [m2[k] + t[a] * m1[b] + t[b] * m1[a] + t[a] * t[b] * m for k, (a, b) in enumerate(PAIRS)]
    return out
