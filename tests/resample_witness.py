"""The numpy witness of the model resample (dust_hip_model_resample; the contract is in include/dust_hip.h). A helper module, not a test
file: written from the header text alone, it shares no code with the device path.

Grids are uint8 [x, y, z] arrays of 256 per axis holding palette index + 1 (0 = empty), the convention of tests/island_witness.py.
The formulation is whole-array int64: the three separable terms of Q are 1-D arrays broadcast into the clipped destination box, the
floor is np.floor_divide by 131072, the image is the boolean array of the voxels whose s lies inside the sub-box, and the ops are
np.where over it. loop_one() is the same contract once more as a pure-Python loop over single voxels with Python integers
(tests/test_resample_witness.py holds the two against each other)."""
import numpy as np

PLACE, OVERWRITE, REPLACE, CARVE, PAINT = 0, 1, 2, 3, 4
ONE = 65536
MAX_M = 8 * 65536
MAX_T = 1 << 28
DRY_RUN = 1
MAX_RESAMPLES = 65536
EXTENT = 256

RESAMPLE_DTYPE = np.dtype([("m", "<i4", (3, 3)), ("t", "<i4", 3), ("dst_lo", "<i4", 3), ("dst_hi", "<i4", 3), ("src_lo", "u1", 3), ("pad0", "u1"),
                           ("src_hi", "u1", 3), ("pad1", "u1"), ("op", "<u4"), ("reserved", "<u4", 3)])
COUNT_DTYPE = np.dtype([("changed", "<u4"), ("covered", "<u4"), ("solid", "<u4"), ("blocked", "<u4")])


def records(m, t, dst_lo, dst_hi, op=PLACE, src_lo=(0, 0, 0), src_hi=(255, 255, 255)):
    """records from integer matrices (n, 3, 3) and translations (n, 3) in units of 1 / 65536"""
    m = np.asarray(m, np.int64).reshape(-1, 3, 3)
    n = len(m)
    out = np.zeros(n, RESAMPLE_DTYPE)
    out["m"] = m
    out["t"] = np.broadcast_to(np.asarray(t, np.int64), (n, 3))
    out["dst_lo"] = np.broadcast_to(np.asarray(dst_lo, np.int64), (n, 3))
    out["dst_hi"] = np.broadcast_to(np.asarray(dst_hi, np.int64), (n, 3))
    out["op"] = np.broadcast_to(np.asarray(op, np.uint32), (n,))
    out["src_lo"] = np.broadcast_to(np.asarray(src_lo, np.uint8), (n, 3))
    out["src_hi"] = np.broadcast_to(np.asarray(src_hi, np.uint8), (n, 3))
    return out


def refused(record=None, flags=0, n=1, palette_map=None):
    """whether the call refuses with INVALID_ARGUMENT for a reason the record, the flags, n or the palette map give"""
    if n > MAX_RESAMPLES or flags & ~DRY_RUN:
        return True
    if palette_map is not None and max(int(v) for v in palette_map) > 254:
        return True
    if record is None:
        return False
    if int(record["op"]) > PAINT:
        return True
    return bool(max(abs(int(v)) for v in record["m"].reshape(-1)) > MAX_M or max(abs(int(v)) for v in record["t"]) > MAX_T)


def clipped_box(record):
    """the destination box clipped to the tree as ([lo], [hi]), or None when the record covers nothing"""
    lo = [max(int(v), 0) for v in record["dst_lo"]]
    hi = [min(int(v), EXTENT - 1) for v in record["dst_hi"]]
    if any(l > h for l, h in zip(lo, hi)) or any(int(l) > int(h) for l, h in zip(record["src_lo"], record["src_hi"])):
        return None
    return lo, hi


def source_of(record, lo, hi):
    """s[k] of every voxel of the inclusive destination box lo..hi: three int64 arrays of the box's shape"""
    m = record["m"].astype(np.int64)
    t = record["t"].astype(np.int64)
    axes = [2 * np.arange(lo[r], hi[r] + 1, dtype=np.int64) + 1 for r in range(3)]
    out = []
    for k in range(3):
        q = (m[k, 0] * axes[0])[:, None, None] + (m[k, 1] * axes[1])[None, :, None] + (m[k, 2] * axes[2])[None, None, :] + 2 * t[k]
        assert np.abs(q).max() < 1 << 31            # the header's bound
        out.append(np.floor_divide(q, 131072))
    return out


def image_of(record, lo, hi):
    """(inside, s): which voxels of the box belong to the image, and their source coordinates"""
    s = source_of(record, lo, hi)
    inside = np.ones(s[0].shape, bool)
    for k in range(3):
        inside &= (s[k] >= int(record["src_lo"][k])) & (s[k] <= int(record["src_hi"][k]))
    return inside, s


def mapped(values, palette_map):
    if palette_map is None:
        return values
    table = np.concatenate([[0], np.asarray(palette_map, np.int64).reshape(255) + 1]).astype(np.uint8)
    return table[values]


def combine(op, v, w):
    if op == PLACE:
        return np.where((v != 0) & (w == 0), v, w)
    if op == OVERWRITE:
        return np.where(v != 0, v, w)
    if op == REPLACE:
        return v.copy()
    if op == CARVE:
        return np.where(v != 0, 0, w).astype(np.uint8)
    assert op == PAINT
    return np.where((v != 0) & (w != 0), v, w)


def resample_one(dst, src, record, palette_map=None, write=True):
    """one record applied to `dst` in place (write) or only held against it, reading `src` (which must not alias dst when writing);
    returns (changed, covered, solid, blocked)"""
    box = clipped_box(record)
    if box is None:
        return 0, 0, 0, 0
    lo, hi = box
    inside, s = image_of(record, lo, hi)
    if not inside.any():
        return 0, 0, 0, 0
    region = tuple(slice(l, h + 1) for l, h in zip(lo, hi))
    w_all = dst[region]
    v = mapped(src[s[0][inside], s[1][inside], s[2][inside]], palette_map)
    w = w_all[inside]
    out = combine(int(record["op"]), v, w)
    counts = (int(np.count_nonzero(out != w)), int(inside.sum()), int(np.count_nonzero(v)), int(np.count_nonzero((v != 0) & (w != 0))))
    if write:
        w_all[inside] = out          # (a view of dst)
    return counts


def resample(dst, src, recs, palette_map=None, dry_run=False):
    """(grid, counts) after a call: the records in array order, every one reading the source as it stood when the call began (src may be
    dst). dry_run: the grid comes back unchanged and every record is counted against it alone"""
    recs = np.asarray(recs, RESAMPLE_DTYPE).reshape(-1)
    assert len(recs) <= MAX_RESAMPLES
    snapshot = np.array(src, np.uint8, copy=True)
    out = np.array(dst, np.uint8, copy=True)
    counts = np.zeros(len(recs), COUNT_DTYPE)
    for i, r in enumerate(recs):
        assert not refused(r)
        counts[i] = resample_one(out, snapshot, r, palette_map, write=not dry_run)
    return out, counts


def loop_one(dst, src, record, palette_map=None):
    """resample_one(write=True) as a loop over single voxels with Python integers: `dst` changed in place, the four counts returned"""
    m = [[int(v) for v in row] for row in record["m"]]
    t = [int(v) for v in record["t"]]
    src_lo = [int(v) for v in record["src_lo"]]
    src_hi = [int(v) for v in record["src_hi"]]
    op = int(record["op"])
    changed = covered = solid = blocked = 0
    if any(l > h for l, h in zip(src_lo, src_hi)):
        return 0, 0, 0, 0
    for x in range(max(int(record["dst_lo"][0]), 0), min(int(record["dst_hi"][0]), 255) + 1):
        for y in range(max(int(record["dst_lo"][1]), 0), min(int(record["dst_hi"][1]), 255) + 1):
            for z in range(max(int(record["dst_lo"][2]), 0), min(int(record["dst_hi"][2]), 255) + 1):
                s = []
                for k in range(3):
                    q = m[k][0] * (2 * x + 1) + m[k][1] * (2 * y + 1) + m[k][2] * (2 * z + 1) + 2 * t[k]
                    s.append(q // 131072)         # Python's // rounds toward minus infinity
                if not all(src_lo[k] <= s[k] <= src_hi[k] for k in range(3)):
                    continue
                v = int(src[s[0], s[1], s[2]])
                if v and palette_map is not None:
                    v = int(palette_map[v - 1]) + 1
                w = int(dst[x, y, z])
                if op == PLACE:
                    to = v if v and not w else w
                elif op == OVERWRITE:
                    to = v if v else w
                elif op == REPLACE:
                    to = v
                elif op == CARVE:
                    to = 0 if v else w
                else:
                    to = v if v and w else w
                covered += 1
                solid += v != 0
                blocked += v != 0 and w != 0
                changed += to != w
                dst[x, y, z] = to
    return changed, covered, solid, blocked


def box_range(record, lo, hi):
    """the exact (min, max) of Q[k] over the inclusive destination box lo..hi, k = 0, 1, 2: Q is affine and separable, so each axis'
    term is extreme at an end of its interval and the sums of the per-axis extremes are attained"""
    out = []
    for k in range(3):
        least = most = 2 * int(record["t"][k])
        for r in range(3):
            ends = [int(record["m"][k][r]) * (2 * c + 1) for c in (lo[r], hi[r])]
            least += min(ends)
            most += max(ends)
        out.append((least, most))
    return out


def box_can_hold(record, lo, hi):
    """the interval test: False -> no voxel of the destination box reads a source voxel inside the sub-box"""
    return all(most // 131072 >= int(record["src_lo"][k]) and least // 131072 <= int(record["src_hi"][k])
               for k, (least, most) in enumerate(box_range(record, lo, hi)))


def cells_listed(record):
    """the root cells (x << 8 | y << 4 | z) the interval test cannot rule out for the record, ascending; all reached cells counted too"""
    box = clipped_box(record)
    if box is None or not box_can_hold(record, *box):
        return [], 0
    lo, hi = box
    listed, reached = [], 0
    for cx in range(lo[0] >> 4, (hi[0] >> 4) + 1):
        for cy in range(lo[1] >> 4, (hi[1] >> 4) + 1):
            for cz in range(lo[2] >> 4, (hi[2] >> 4) + 1):
                c = (cx, cy, cz)
                reached += 1
                if box_can_hold(record, [max(16 * c[r], lo[r]) for r in range(3)], [min(16 * c[r] + 15, hi[r]) for r in range(3)]):
                    listed.append(cx << 8 | cy << 4 | cz)
    return listed, reached
