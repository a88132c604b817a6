"""The numpy witness of the model casts (dust_hip_model_cast; the contract is in include/dust_hip.h). A helper module, not a test file:
written from the header text alone, it shares no code with the device path.

Grids are [x, y, z] arrays, cubes of one extent (256 for a model; the CPU tests also use small ones), nonzero = solid: the uint8 grids
of tests/stamp_witness.py work as they are. The formulation is whole-array and per placement -- the opposite direction from a per-voxel
walk: the source sub-box is sliced out, oriented with np.transpose / np.flip (stamp_witness's helpers name p and g), and for a
placement k the whole image is shifted to offset + k * step as one boolean array, clipped to the tree and ANDed with the destination
slice it lands on; under WALLS the part of the image the clip cut off is blocked as it stands. Placements are examined upward, but only
those at which the tight box of the piece's voxels can meet the tree (plus, under WALLS, the first one at which it sticks out): the
count does not grow with the offset or with max_steps. All index arithmetic is on Python integers: no offset overflows; `contact` alone is
reduced to int32, as the header says."""
import numpy as np

from stamp_witness import IDENTITY, orient_fields

WALLS = 1
HIT, OVERLAP, HIT_WALL = 1, 2, 4
MAX_STEPS = 65535
MAX_CASTS = 65536
NO_KEY = 0xFFFFFFFF

CAST_DTYPE = np.dtype([("offset", "<i4", 3), ("orient", "<u4"), ("step", "<i4", 3), ("max_steps", "<u4"), ("flags", "<u4"), ("src_lo", "u1", 3),
                       ("pad0", "u1"), ("src_hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("steps", "<u4"), ("flags", "<u4"), ("contacts", "<u4"), ("voxels", "<u4"), ("contact", "<i4", 3), ("src_key", "<u4")])


def records(offset, step, max_steps, orient=IDENTITY, flags=0, src_lo=(0, 0, 0), src_hi=(255, 255, 255)):
    offset = np.asarray(offset, np.int64).reshape(-1, 3)
    out = np.zeros(len(offset), CAST_DTYPE)
    out["offset"] = offset
    out["orient"] = np.broadcast_to(np.asarray(orient, np.uint32), (len(offset),))
    out["step"] = np.broadcast_to(np.asarray(step, np.int32), (len(offset), 3))
    out["max_steps"] = np.broadcast_to(np.asarray(max_steps, np.uint32), (len(offset),))
    out["flags"] = np.broadcast_to(np.asarray(flags, np.uint32), (len(offset),))
    out["src_lo"] = np.broadcast_to(np.asarray(src_lo, np.uint8), (len(offset), 3))
    out["src_hi"] = np.broadcast_to(np.asarray(src_hi, np.uint8), (len(offset), 3))
    return out


def oriented(src, cast):
    """the image of the cast's sub-box as a boolean array indexed by u (None: src_lo > src_hi), and a function u -> source voxel"""
    p, g = orient_fields(cast["orient"])
    lo = [int(v) for v in cast["src_lo"]]
    hi = [int(v) for v in cast["src_hi"]]
    if any(l > h for l, h in zip(lo, hi)):
        return None, None
    image = np.asarray(src)[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] != 0
    image = np.flip(np.transpose(image, p), [r for r in range(3) if g[r]])

    def source_of(u):
        s = [0, 0, 0]
        for r in range(3):
            s[p[r]] = hi[p[r]] - int(u[r]) if g[r] else lo[p[r]] + int(u[r])
        return s
    return image, source_of


def blocked_at(dst, image, at, walls):
    """(blocked, outside): boolean arrays of the image's shape -- the piece voxels blocked with the image's lowest corner at `at`, and those
    among them that stand outside the tree"""
    extent = dst.shape[0]
    take, put = [], []
    for r in range(3):
        first, last = max(at[r], 0), min(at[r] + image.shape[r] - 1, extent - 1)
        if first > last:
            take = None
            break
        put.append(slice(first, last + 1))
        take.append(slice(first - at[r], last - at[r] + 1))
    blocked = np.zeros(image.shape, bool)
    outside = image.copy() if walls else np.zeros(image.shape, bool)
    if take is not None:
        blocked[tuple(take)] = image[tuple(take)] & (dst[tuple(put)] != 0)
        outside[tuple(take)] = False
    return blocked | outside, outside


def cast_one(dst, src, cast):
    """one DustHipCastHit as a tuple (steps, flags, contacts, voxels, contact, src_key)"""
    extent = dst.shape[0]
    max_steps = int(cast["max_steps"])
    miss = (max_steps, 0, 0, 0, (0, 0, 0), NO_KEY)
    image, source_of = oriented(src, cast)
    if image is None or not image.any():
        return miss
    voxels = int(np.count_nonzero(image))
    miss = miss[:3] + (voxels,) + miss[4:]
    off = [int(v) for v in cast["offset"]]
    step = [int(v) for v in cast["step"]]
    walls = bool(int(cast["flags"]) & WALLS)
    last_k = 0 if step == [0, 0, 0] else max_steps
    # the tight box of the piece in image coordinates, and the placement intervals in which it is wholly inside / meets the tree
    solid = np.argwhere(image)
    bb_lo, bb_hi = solid.min(axis=0), solid.max(axis=0)
    big = 1 << 40
    in_lo, in_hi, meet_lo, meet_hi = -big, big, -big, big
    for r in range(3):
        a, b = off[r] + int(bb_lo[r]), off[r] + int(bb_hi[r])
        if step[r] == 0:
            if not (a >= 0 and b <= extent - 1):
                in_lo, in_hi = 1, 0
            if not (b >= 0 and a <= extent - 1):
                meet_lo, meet_hi = 1, 0
            continue
        # position = a + k * step: inside needs a + k s >= 0 and b + k s <= extent - 1
        if step[r] > 0:
            il, ih, ml, mh = -a, extent - 1 - b, -b, extent - 1 - a
        else:
            il, ih, ml, mh = b - (extent - 1), a, a - (extent - 1), b
        in_lo, in_hi = max(in_lo, il), min(in_hi, ih)
        meet_lo, meet_hi = max(meet_lo, ml), min(meet_hi, mh)
    if walls:
        if in_lo <= 0 <= in_hi:
            placements = range(0, min(last_k, in_hi + 1) + 1)   # inside the tree up to in_hi, then it sticks out
        else:
            placements = range(0, 1)                            # it sticks out at once
    else:
        placements = range(max(meet_lo, 0), min(meet_hi, last_k) + 1)
    for k in placements:
        at = [off[r] + k * step[r] for r in range(3)]
        blocked, outside = blocked_at(dst, image, at, walls)
        if not blocked.any():
            continue
        us = np.argwhere(blocked)
        keys = [(s[0] << 16 | s[1] << 8 | s[2], tuple(int(v) for v in u)) for u in us for s in [source_of(u)]]
        key, u = min(keys)
        contact = tuple(((at[r] + u[r] + (1 << 31)) % (1 << 32)) - (1 << 31) for r in range(3))
        flags = HIT | (OVERLAP if k == 0 else 0) | (HIT_WALL if outside.any() else 0)
        return (k - 1 if k else 0, flags, len(us), voxels, contact, key)
    return miss


def cast(dst, src, casts):
    """the hits of a call (HIT_DTYPE): every cast on its own, both grids only read"""
    casts = np.asarray(casts, CAST_DTYPE).reshape(-1)
    assert len(casts) <= MAX_CASTS
    dst, src = np.asarray(dst), np.asarray(src)
    out = np.zeros(len(casts), HIT_DTYPE)
    for i, c in enumerate(casts):
        steps, flags, contacts, voxels, contact, key = cast_one(dst, src, c)
        out[i] = (steps, flags, contacts, voxels, contact, key)
    return out
