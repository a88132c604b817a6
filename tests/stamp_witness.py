"""The numpy witness of the model stamps (dust_hip_model_stamp; the contract is in include/dust_hip.h). A helper module, not a test file:
written from the header text alone, it shares no code with the device path.

Grids are uint8 [x, y, z] arrays of 256 per axis holding palette index + 1 (0 = empty), the convention of tests/island_witness.py.
The formulation is forward and whole-array -- the opposite direction from a per-voxel gather: the source sub-box is sliced out,
np.transpose puts source axis p[r] on destination axis r, np.flip reverses the axes with g[r] set, the image is clipped to the tree
and combined with the destination slice it lands on, per op. All index arithmetic is on Python integers: no offset overflows."""
import itertools

import numpy as np

PLACE, OVERWRITE, REPLACE, CARVE, PAINT = 0, 1, 2, 3, 4
MAX_STAMPS = 65536
EXTENT = 256
IDENTITY = 0x24

STAMP_DTYPE = np.dtype([("offset", "<i4", 3), ("orient", "<u4"), ("op", "<u4"), ("src_lo", "u1", 3), ("pad0", "u1"), ("src_hi", "u1", 3), ("pad1", "u1"),
                        ("reserved", "<u4")])


def orient_word(perm, flips):
    return perm[0] | perm[1] << 2 | perm[2] << 4 | sum(1 << (6 + r) for r in range(3) if flips[r])


def orient_fields(orient):
    """(p, g) of an orient word; None when it is not one of the 48"""
    orient = int(orient)
    p = [(orient >> (2 * r)) & 3 for r in range(3)]
    g = [(orient >> (6 + r)) & 1 for r in range(3)]
    if orient >> 9 or sorted(p) != [0, 1, 2]:
        return None
    return p, g


def all_orientations():
    """the 48 orient words: every permutation with every combination of flips"""
    return [orient_word(p, g) for p in itertools.permutations(range(3)) for g in itertools.product((0, 1), repeat=3)]


def inverse(orient):
    """the orientation that maps an image back onto its source: q[p[r]] = r, flipped where r was"""
    p, g = orient_fields(orient)
    q, h = [0, 0, 0], [0, 0, 0]
    for r in range(3):
        q[p[r]], h[p[r]] = r, g[r]
    return orient_word(q, h)


def mapped(values, palette_map):
    """source grid bytes as they arrive: None stays None, index i becomes palette_map[i]"""
    if palette_map is None:
        return values
    table = np.concatenate([[0], np.asarray(palette_map, np.int64).reshape(255) + 1]).astype(np.uint8)
    return table[values]


def stamp_one(dst, src, stamp, palette_map=None):
    """one stamp applied to `dst` in place, reading `src` (which must not alias dst); returns the number of voxels changed"""
    p, g = orient_fields(stamp["orient"])
    lo = [int(v) for v in stamp["src_lo"]]
    hi = [int(v) for v in stamp["src_hi"]]
    if any(l > h for l, h in zip(lo, hi)):
        return 0
    image = mapped(src[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1], palette_map)
    image = np.transpose(image, p)
    image = np.flip(image, [r for r in range(3) if g[r]])
    at = [int(v) for v in stamp["offset"]]
    take, put = [], []
    for r in range(3):
        first, last = max(at[r], 0), min(at[r] + image.shape[r] - 1, EXTENT - 1)
        if first > last:
            return 0
        put.append(slice(first, last + 1))
        take.append(slice(first - at[r], last - at[r] + 1))
    v = image[tuple(take)]
    w = dst[tuple(put)]
    op = int(stamp["op"])
    if op == PLACE:
        out = np.where((v != 0) & (w == 0), v, w)
    elif op == OVERWRITE:
        out = np.where(v != 0, v, w)
    elif op == REPLACE:
        out = v.copy()
    elif op == CARVE:
        out = np.where(v != 0, 0, w)
    else:
        assert op == PAINT
        out = np.where((v != 0) & (w != 0), v, w)
    changed = int(np.count_nonzero(out != w))
    dst[tuple(put)] = out
    return changed


def stamp(dst, src, stamps, palette_map=None):
    """(grid, changed) after a call: the stamps in array order, every one reading the source as it stood when the call began (src may be dst)"""
    stamps = np.asarray(stamps, STAMP_DTYPE).reshape(-1)
    assert len(stamps) <= MAX_STAMPS
    snapshot = np.array(src, np.uint8, copy=True)
    out = np.array(dst, np.uint8, copy=True)
    changed = np.array([stamp_one(out, snapshot, s, palette_map) for s in stamps], np.uint32).reshape(-1)
    return out, changed


def records(offset, orient=IDENTITY, op=PLACE, src_lo=(0, 0, 0), src_hi=(255, 255, 255)):
    offset = np.asarray(offset, np.int64).reshape(-1, 3)
    out = np.zeros(len(offset), STAMP_DTYPE)
    out["offset"] = offset
    out["orient"] = np.broadcast_to(np.asarray(orient, np.uint32), (len(offset),))
    out["op"] = np.broadcast_to(np.asarray(op, np.uint32), (len(offset),))
    out["src_lo"] = np.broadcast_to(np.asarray(src_lo, np.uint8), (len(offset), 3))
    out["src_hi"] = np.broadcast_to(np.asarray(src_hi, np.uint8), (len(offset), 3))
    return out
