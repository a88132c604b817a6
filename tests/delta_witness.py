"""The numpy witness of the model deltas (dust_hip_model_delta, dust_hip_model_delta_apply; the contract is in include/dust_hip.h). A
helper module, not a test: tests/test_delta_witness.py holds it to a plain per-voxel loop, tests/test_delta_rule.py holds the brick-word
rule and the host records to it, tests/test_gpu_delta.py the device.

Written from the header text on whole arrays: a voxel differs where the two grids' bytes differ (one comparison of the two grids;
the rest works on the list of those voxels); its kind follows from which of the two is None; a voxel is listed when it lies inside the clipped region, differs, its kind is asked for and its value before or after is the
filter's; the list is sorted by the voxel's place in the model's block order (surface_witness.block_order, written out there from its
definition). A grid holds palette index + 1 per voxel, 0 = None, indexed [x, y, z]; it may be any box (the tree is 256^3)."""
import numpy as np

from surface_witness import block_order, clip

ADDED, REMOVED, REPAINTED = 1, 2, 4
ALL = 7
NONE = 255
BACKWARD = 1
BINS = 256
MAX_RECORDS = 1 << 24

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("kinds", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                        ("reserved", "<u4", 2)])
RESULT_DTYPE = np.dtype([("voxels", "<u4"), ("added", "<u4"), ("removed", "<u4"), ("repainted", "<u4"), ("solid_before", "<u4"), ("solid_after", "<u4"),
                         ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 8)])
VOXEL_DTYPE = np.dtype([("key", "<u4"), ("kind", "u1"), ("before", "u1"), ("after", "u1"), ("reserved", "u1")])


def refused(kinds, flags, palette, lo, hi):
    """what dust_hip_model_delta refuses with DUST_ERR_INVALID_ARGUMENT (beyond null pointers, contexts and struct_size)"""
    return bool(kinds == 0 or kinds > ALL or flags != 0 or palette < -1 or palette > 254 or max(*lo, *hi) >= 256)


def zero_result():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["lo"] = 255
    return r


def delta(before, after, kinds=ALL, palette=-1, region=None):
    """(result, voxels, counts) of a call with room for every voxel"""
    assert before.shape == after.shape and not refused(kinds, 0, palette, (0, 0, 0), (0, 0, 0))
    result, counts = zero_result(), np.zeros((2, BINS), np.uint32)
    box = clip(before, region)
    if box is None:
        return result, np.zeros(0, VOXEL_DTYPE), counts
    a, b = before[box], after[box]
    xyz = np.argwhere(a != b) + np.array([s.start for s in box])              # the voxels that differ, then those of them that are listed
    was, now = before[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int64), after[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int64)
    kind = np.where(was == 0, ADDED, np.where(now == 0, REMOVED, REPAINTED))
    listed = (kind & kinds) != 0
    if palette >= 0:
        listed &= (was == palette + 1) | (now == palette + 1)
    xyz, was, now, kind = xyz[listed], was[listed], now[listed], kind[listed]
    order = np.argsort(block_order(xyz[:, 0], xyz[:, 1], xyz[:, 2]), kind="stable")
    xyz, was, now, kind = xyz[order], was[order], now[order], kind[order]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    voxels = np.zeros(len(xyz), VOXEL_DTYPE)
    voxels["key"] = (x << 16) | (y << 8) | z
    voxels["kind"] = kind
    voxels["before"], voxels["after"] = (was - 1) & 255, (now - 1) & 255     # None (0) becomes NONE (255)
    result["voxels"] = len(xyz)
    for name, bit in (("added", ADDED), ("removed", REMOVED), ("repainted", REPAINTED)):
        result[name] = np.count_nonzero(voxels["kind"] == bit)
    result["solid_before"], result["solid_after"] = np.count_nonzero(a), np.count_nonzero(b)
    counts[0], counts[1] = np.bincount(was, minlength=BINS), np.bincount(now, minlength=BINS)
    if len(xyz):
        result["lo"], result["hi"] = xyz.min(axis=0), xyz.max(axis=0)
    return result, voxels, counts


def survivors(records):
    """the records a delta_apply call keeps: of a key named more than once the last one"""
    keys = records["key"].astype(np.int64)
    _, first_from_the_back = np.unique(keys[::-1], return_index=True)
    return records[np.sort(len(records) - 1 - first_from_the_back)]


def apply(grid, records, backward=False):
    """(the grid after delta_apply, changed, conflicts): every surviving record's voxel takes `after` and is expected to hold `before`
    (backward: the other way round), judged on the grid as it is"""
    kept = survivors(np.asarray(records, VOXEL_DTYPE))
    assert np.all(kept["key"] < 1 << 24)
    key = kept["key"].astype(np.int64)
    x, y, z = key >> 16, (key >> 8) & 255, key & 255
    expected, to = ("after", "before") if backward else ("before", "after")
    out = grid.copy()
    conflicts = int(np.count_nonzero(grid[x, y, z] != ((kept[expected].astype(np.int64) + 1) & 255)))
    out[x, y, z] = (kept[to].astype(np.int64) + 1) & 255                       # NONE (255) becomes None (0)
    return out, int(np.count_nonzero(out != grid)), conflicts
