"""The numpy witness of the model settling (dust_hip_model_settle, dust_hip_model_settle_apply; the contract is in include/dust_hip.h).
A helper module, not a test: tests/test_settle_witness.py checks it against a plain per-voxel loop, the conservation of every material
and the descent identity; tests/test_gpu_settle.py holds the device to it.

Written from the header text on whole arrays. A fall turns the region into [v][u][position, the toward end first]: a loose voxel's
floor is a running maximum over the fixed voxels below it, its rank a difference of two cumulative sums of the loose voxels, and every
loose byte is scattered to floor + rank at once. A slide is array shifts inside the region: what lies off the region is blocked for a
destination and empty for the voxel above. The grid holds palette index + 1 per voxel, 0 = None, indexed [x, y, z]; it may be any box
(the tree is 256^3)."""
import numpy as np

from column_witness import FACES, NEG_X, NEG_Y, NEG_Z, POS_X, POS_Y, POS_Z, U_AXIS, V_AXIS, clip, side, turned  # noqa: F401

MAX_GENERATIONS = 256
QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("toward", "<u4"), ("flags", "<u4"), ("reserved", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3), ("loose", "<u4", 8)])
RESULT_DTYPE = np.dtype([("columns", "<u4"), ("loose", "<u4"), ("fixed", "<u4"), ("moved", "<u4"), ("changed", "<u4"), ("fall_max", "<u4"), ("fall_sum", "<u8"),
                         ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("changed_columns", "<u4"), ("reserved", "<u4", 5)])
APPLIED_DTYPE = np.dtype([("generations", "<u4"), ("first_moved", "<u4"), ("loose", "<u4"), ("reserved0", "<u4"), ("slid", "<u8"), ("fell", "<u8"),
                          ("fall_sum", "<u8"), ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 4)])


def loose_mask(indices=None):
    """the eight words of query.loose: the palette indices named (ints or inclusive (first, last) pairs); None: all 255"""
    bits = (1 << 255) - 1 if indices is None else 0
    for item in () if indices is None else indices:
        first, last = item if isinstance(item, tuple) else (item, item)
        for p in range(first, last + 1):
            bits |= 1 << p
    return tuple((bits >> (32 * w)) & 0xFFFFFFFF for w in range(8))


ALL_LOOSE = loose_mask()


def refused(toward, flags, reserved, lo, hi, loose, generations=0):
    """what the calls refuse with DUST_ERR_INVALID_ARGUMENT (beyond null pointers and struct_size)"""
    return bool(toward not in FACES or flags != 0 or reserved != 0 or any(c >= 256 for c in tuple(lo) + tuple(hi)) or (loose[7] >> 31) or generations > MAX_GENERATIONS)


def zero_result():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["lo"] = 255
    return r


def zero_applied():
    r = np.zeros(1, APPLIED_DTYPE)[0]
    r["lo"] = 255
    return r


def is_loose(grid, loose):
    """per voxel: solid, and its palette index has its bit in the mask"""
    lut = np.zeros(256, bool)
    for p in range(255):
        lut[p + 1] = (loose[p >> 5] >> (p & 31)) & 1
    return lut[grid]


def step(toward):
    """g: the unit step toward the side"""
    axis, high = side(toward)
    g = [0, 0, 0]
    g[axis] = 1 if high else -1
    return tuple(g)


def lateral(toward, k):
    """the slide direction of generation k: +u, -u, +v, -v"""
    axis, _ = side(toward)
    d = [0, 0, 0]
    d[(U_AXIS, V_AXIS)[(k >> 1) & 1][axis]] = -1 if k & 1 else 1
    return tuple(d)


def shifted(array, offset, fill):
    """out[p] = array[p + offset], `fill` where p + offset lies outside the array"""
    out = np.full_like(array, fill)
    src, dst = [], []
    for n, o in zip(array.shape, offset):
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n + min(-o, 0)))
    if all(s.stop > s.start for s in src):
        out[tuple(dst)] = array[tuple(src)]
    return out


WHOLE = (slice(None),) * 3


def height_sum(grid, toward, loose, box):
    """the sum over the region's loose voxels of their position counted from the toward end"""
    at = np.nonzero(turned(is_loose(grid[box], loose), WHOLE, toward))[2]
    return int(at.sum())


def fall_region(region, toward, loose):
    """(the region after one fall, its record as a dict): the columns that hold a loose voxel are gathered and walked together"""
    out = region.copy()
    free_all = turned(is_loose(region, loose), WHOLE, toward)
    vs, us = np.nonzero(free_all.any(axis=2))
    before = turned(region, WHOLE, toward)[vs, us]                                   # (n, length) copies
    free = free_all[vs, us]
    fixed = (before != 0) & ~free
    n = before.shape[1]
    position = np.arange(n, dtype=np.int32)[None, :]
    floor = np.maximum.accumulate(np.where(fixed, position + 1, 0), axis=1)          # one past the highest fixed position at or below: a loose voxel is not fixed
    below = np.cumsum(free, axis=1, dtype=np.int32) - free                           # loose voxels below each position
    padded = np.concatenate([below, np.zeros((len(vs), 1), np.int32)], axis=1)
    to = floor + below - np.take_along_axis(padded, floor, axis=1)                   # the floor + the loose voxels between the floor and it
    rows, at = np.nonzero(free)
    after = np.where(free, 0, before)
    after[rows, to[rows, at]] = before[rows, at]
    turned(out, WHOLE, toward)[vs, us] = after                                       # a view: writing it writes `out`
    falls = at - to[rows, at]
    record = {"loose": int(free.sum()), "fixed": int(np.count_nonzero(region)) - int(free.sum()), "moved": int(np.count_nonzero(falls)),
              "changed": int(np.count_nonzero((before != 0) != (after != 0))), "fall_max": int(falls.max()) if len(falls) else 0, "fall_sum": int(falls.sum()),
              "changed_columns": len(np.unique(rows[falls > 0])), "turned": (region != 0) != (out != 0)}
    return out, record


def slide_region(region, toward, d, loose):
    """(the region after one slide in direction d, the voxels slid, the voxels that turned solid or empty)"""
    g = step(toward)
    dg = tuple(a + b for a, b in zip(d, g))
    solid = region != 0
    leave = is_loose(region, loose) & ~shifted(solid, tuple(-c for c in g), False) & ~shifted(solid, d, True) & ~shifted(solid, dg, True)
    back = tuple(-c for c in dg)
    arrive = shifted(leave, back, False)
    new = np.where(leave, 0, region)
    new = np.where(arrive, shifted(region, back, 0), new)
    return new, int(leave.sum()), leave | arrive


def fall(grid, toward, loose, box):
    """(the grid after one fall of the region `box`, the fall's record; its "turned" has the region's shape)"""
    out = grid.copy()
    out[box], record = fall_region(grid[box], toward, loose)
    return out, record


def slide(grid, toward, d, loose, box):
    """(the grid after one slide of the region `box` in direction d, the voxels slid, the region's voxels that turned solid or empty)"""
    out = grid.copy()
    out[box], slid, turned_over = slide_region(grid[box], toward, d, loose)
    return out, slid, turned_over


def bounds_of(mask, box):
    """the inclusive bounds, in the grid's coordinates, of the set voxels of a mask over the region `box`"""
    if not mask.any():
        return (255, 255, 255), (0, 0, 0)
    where = np.nonzero(mask)
    return tuple(int(c.min()) + b.start for c, b in zip(where, box)), tuple(int(c.max()) + b.start for c, b in zip(where, box))


def settle(grid, toward, loose=ALL_LOOSE, region=None):
    """the result of dust_hip_model_settle: what ONE fall would do"""
    result = zero_result()
    box = clip(grid, region)
    if box is None:
        return result
    _, record = fall_region(grid[box], toward, loose)
    axis, _ = side(toward)
    shape = grid[box].shape
    result["columns"] = shape[U_AXIS[axis]] * shape[V_AXIS[axis]]
    for name in ("loose", "fixed", "moved", "changed", "fall_max", "fall_sum", "changed_columns"):
        result[name] = record[name]
    result["lo"], result["hi"] = bounds_of(record["turned"], box)
    return result


def apply(grid, toward, loose=ALL_LOOSE, generations=0, region=None, rest_within=None):
    """(the grid after dust_hip_model_settle_apply, the applied record, the per-generation rows (generations, 2)). Once four generations
    in a row moved nothing the rest is not computed: they move nothing either. rest_within: assert that this happens within so many
    generations."""
    assert 0 <= generations <= MAX_GENERATIONS
    applied, rows = zero_applied(), np.zeros((generations, 2), np.uint32)
    box = clip(grid, region)
    if box is None:
        return grid.copy(), applied, rows
    at, first = fall_region(grid[box], toward, loose)
    touched = first["turned"].copy()
    fall_sum, slid_sum, fell_sum, last, still, rest = first["fall_sum"], 0, 0, 0, 0, None
    for k in range(generations):
        at, slid, turned_by_slide = slide_region(at, toward, lateral(toward, k), loose)
        at, record = fall_region(at, toward, loose)
        rows[k] = slid, record["moved"]
        if slid + record["moved"]:
            last, still = k + 1, 0
            touched |= turned_by_slide | record["turned"]
            fall_sum, slid_sum, fell_sum = fall_sum + record["fall_sum"], slid_sum + slid, fell_sum + record["moved"]
        else:
            still += 1
            if still == 4:
                rest = k + 1 - 4
                break
    if rest_within is not None:
        assert rest is not None and rest <= rest_within, (rest, rest_within)
    applied["generations"], applied["first_moved"], applied["loose"] = last, first["moved"], first["loose"]
    applied["slid"], applied["fell"], applied["fall_sum"] = slid_sum, fell_sum, fall_sum
    applied["lo"], applied["hi"] = bounds_of(touched, box)
    out = grid.copy()
    out[box] = at
    return out, applied, rows
