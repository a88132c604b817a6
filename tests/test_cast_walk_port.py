"""The cast kernels' arithmetic without a device: a line-by-line Python port of the host's record (model_records.hpp device_cast;
tests/test_model_records.py holds the native function to this port), of k_cast_walk and of k_cast_count (cast.hip) -- lanes as numpy
arrays of 64, the wave-uniform values as Python integers, int32 sums checked for overflow -- run against tests/cast_witness.py on 256^3 grids. The work items run one after the other in a shuffled order against one
shared `best`, so the relaxed read that prunes a walk sees anything from nothing to every other wave's result; every brick-mask index
the port forms is checked against the lattice."""
import numpy as np
import pytest

import cast_witness as W
from stamp_witness import all_orientations

LATTICE = 1 << 18
NO_HIT = (1 << 64) - 1
OFFSET_LIMIT = 1 << 20
MAX_WALK = 256 + 255 + 2
WALLS_BIT = 1 << 16
LANE = np.arange(64)


def leaf_code(bx, by, bz):
    return ((((bx >> 2) << 8) | ((by >> 2) << 4) | (bz >> 2)) << 6) | ((bx & 3) << 4) | ((by & 3) << 2) | (bz & 3)


def brick_masks(grid):
    """EditArgs::brick_mask of a grid, as Python integers"""
    masks = [0] * LATTICE
    for x, y, z in np.argwhere(grid != 0).tolist():
        masks[leaf_code(x >> 2, y >> 2, z >> 2)] |= 1 << (((x & 3) << 4) | ((y & 3) << 2) | (z & 3))
    return masks


def int32(v):
    assert -2 ** 31 <= v < 2 ** 31, v
    return v


def device_cast(c):
    lo, hi = [int(v) for v in c["src_lo"]], [int(v) for v in c["src_hi"]]
    if any(l > h for l, h in zip(lo, hi)):
        return None
    orient, walls = int(c["orient"]), int(c["flags"]) & 1
    step = [int(v) for v in c["step"]]
    max_steps = 0 if step == [0, 0, 0] else int(c["max_steps"])
    never = 1 << 40
    first, last, off = -never, never, []
    for r in range(3):
        p = (orient >> (2 * r)) & 3
        o, ext = int(c["offset"][r]), hi[p] - lo[p]
        if step[r] == 0:
            meets = o + ext >= 0 and o <= 255
            f, l = (-never, never) if meets else (1, 0)
        elif step[r] > 0:
            f, l = -(o + ext), 255 - o
        else:
            f, l = o - 255, o + ext
        first, last = max(first, f), min(last, l)
        off.append(min(max(o, -OFFSET_LIMIT), OFFSET_LIMIT))
    if walls:
        k_lo, k_hi = 0, (min(max_steps, last + 1) if first <= 0 <= last else 0)
    else:
        k_lo, k_hi = max(first, 0), min(last, max_steps)
    if k_lo > k_hi:
        k_lo, k_hi = 1, 0
    assert 0 <= k_lo < 2 ** 32 and 0 <= k_hi < 2 ** 32
    return dict(off=off, orient=orient | (WALLS_BIT if walls else 0), step=step, max_steps=max_steps, k_lo=k_lo, k_hi=k_hi, lo=lo, hi=hi)


class View:
    def __init__(self, d):
        self.d = d
        self.p = [(d["orient"] >> (2 * r)) & 3 for r in range(3)]
        self.g = [(d["orient"] >> (6 + r)) & 1 for r in range(3)]
        self.walls = bool(d["orient"] & WALLS_BIT)

    def clipped(self, src_mask, cell):
        """per lane: the mask of the cell's brick `lane`, clipped to the sub-box"""
        out = []
        for lane in range(64):
            origin = ((((cell >> 8) << 2) | (lane >> 4)) * 4, ((((cell >> 4) & 15) << 2) | ((lane >> 2) & 3)) * 4, (((cell & 15) << 2) | (lane & 3)) * 4)
            keep = [0, 0, 0]
            for i in range(4):
                for axis, unit, shift in ((0, 0xFFFF, 16 * i), (1, 0x000F000F000F000F, 4 * i), (2, 0x1111111111111111, i)):
                    if self.d["lo"][axis] <= origin[axis] + i <= self.d["hi"][axis]:
                        keep[axis] |= (unit << shift) & NO_HIT
            index = cell * 64 + lane
            assert 0 <= index < LATTICE
            out.append(src_mask[index] & keep[0] & keep[1] & keep[2])
        return out

    def brick(self, cell, b, bm):
        s0 = [((((cell >> 8) << 2) | (b >> 4)) * 4), (((((cell >> 4) & 15) << 2) | ((b >> 2) & 3)) * 4), ((((cell & 15) << 2) | (b & 3)) * 4)]
        s = [s0[0] + (LANE >> 4), s0[1] + ((LANE >> 2) & 3), s0[2] + (LANE & 3)]
        solid = np.array([(bm >> int(l)) & 1 for l in LANE], bool)
        key = (s[0] << 16) | (s[1] << 8) | s[2]
        d0 = []
        for r in range(3):
            sp, lp, hp = s[self.p[r]], self.d["lo"][self.p[r]], self.d["hi"][self.p[r]]
            d0.append(self.d["off"][r] + (hp - sp if self.g[r] else sp - lp))
        return s0, solid, key, d0

    def blocked(self, solid, d0, k, dst_mask):
        d = [d0[r] + k * self.d["step"][r] for r in range(3)]
        for r in range(3):
            assert np.abs(d[r][solid]).max(initial=0) < 2 ** 31
        inside = ((d[0] | d[1] | d[2]) & 0xFFFFFFFF) < 256
        out = np.zeros(64, bool)
        for l in np.nonzero(solid)[0]:
            if not inside[l]:
                out[l] = self.walls
                continue
            x, y, z = int(d[0][l]), int(d[1][l]), int(d[2][l])
            code = leaf_code(x >> 2, y >> 2, z >> 2)
            assert 0 <= code < LATTICE and 0 <= min(x, y, z) and max(x, y, z) < 256
            out[l] = (dst_mask[code] >> (((x & 3) << 4) | ((y & 3) << 2) | (z & 3))) & 1
        return out, ~inside


def walk_wave(view, cell, wave, src_mask, dst_mask, best, slot, prune):
    d = view.d
    if d["k_lo"] > d["k_hi"]:
        return
    m = view.clipped(src_mask, cell)
    todo = [b for b in range(16 * wave, 16 * wave + 16) if m[b]]
    mine, bound = NO_HIT, d["k_hi"]
    for b in todo:
        s0, solid, key, d0 = view.brick(cell, b, m[b])
        first, last = -2 ** 31, 2 ** 31 - 1
        for r in range(3):
            p = view.p[r]
            smin, smax = max(s0[p], d["lo"][p]), min(s0[p] + 3, d["hi"][p])
            dmin = int32(d["off"][r] + (d["hi"][p] - smax if view.g[r] else smin - d["lo"][p]))
            dmax = int32(d["off"][r] + (d["hi"][p] - smin if view.g[r] else smax - d["lo"][p]))
            if d["step"][r] == 0:
                f, l = (-2 ** 31, 2 ** 31 - 1) if dmax >= 0 and dmin <= 255 else (1, 0)
            elif d["step"][r] > 0:
                f, l = -dmax, 255 - dmin
            else:
                f, l = dmin - 255, dmax
            first, last = max(first, f), min(last, l)
        if view.walls:
            ka, kb = 0, (last + 1 if first <= 0 <= last else 0)
        else:
            ka, kb = max(first, 0), last
        ka, kb = max(ka, d["k_lo"]), min(kb, bound)
        assert kb <= ka + MAX_WALK or ka > kb     # the defensive clamp never binds
        if ka > kb:
            continue
        k, end, found = ka, kb, None
        rounds = 0
        while k <= end and found is None:
            rounds += 1
            assert rounds <= MAX_WALK // 4 + 2
            seen = (best[slot] >> 24) if prune else NO_HIT
            end = min(end, seen)
            hits = [view.blocked(solid, d0, k + j, dst_mask)[0] & (k + j <= end) for j in range(4)]
            for j in range(4):
                if found is None and hits[j].any():
                    found = k + j
                    mine = min(mine, min(((found << 24) | int(kk)) for kk in key[hits[j]]))
            k += 4
        if found is not None and found < bound:
            bound = found
    if mine != NO_HIT:
        best[slot] = min(best[slot], mine)


def count_wave(view, cell, wave, src_mask, dst_mask, best, slot, acc):
    m = view.clipped(src_mask, cell)
    for b in range(16 * wave, 16 * wave + 16):
        if not m[b]:
            continue
        acc[slot][1] += bin(m[b]).count("1")
        if best[slot] == NO_HIT:
            continue
        _, solid, _, d0 = view.brick(cell, b, m[b])
        blk, outside = view.blocked(solid, d0, best[slot] >> 24, dst_mask)
        acc[slot][0] += int(np.count_nonzero(blk))
        acc[slot][2] |= int((blk & outside).any())


def port_call(dst_mask, src_mask, casts, rng, prune=True):
    """dust_hip_model_cast as the host and the two kernels compute it"""
    hits = np.zeros(len(casts), W.HIT_DTYPE)
    hits["steps"], hits["src_key"] = casts["max_steps"], W.NO_KEY
    dev = [(i, device_cast(c)) for i, c in enumerate(casts)]
    dev = [(i, d) for i, d in dev if d is not None]
    best, acc = [NO_HIT] * len(dev), [[0, 0, 0] for _ in dev]
    items = [(slot, (x << 8) | (y << 4) | z, wave) for slot, (_, d) in enumerate(dev)
             for x in range(d["lo"][0] >> 4, (d["hi"][0] >> 4) + 1) for y in range(d["lo"][1] >> 4, (d["hi"][1] >> 4) + 1)
             for z in range(d["lo"][2] >> 4, (d["hi"][2] >> 4) + 1) for wave in range(4)]
    views = [View(d) for _, d in dev]
    for j in rng.permutation(len(items)):
        slot, cell, wave = items[j]
        walk_wave(views[slot], cell, wave, src_mask, dst_mask, best, slot, prune)
    for slot, cell, wave in items:
        count_wave(views[slot], cell, wave, src_mask, dst_mask, best, slot, acc)
    for slot, (i, d) in enumerate(dev):
        c, h = casts[i], hits[i]
        h["voxels"] = acc[slot][1]
        if best[slot] == NO_HIT:
            continue
        k, key = best[slot] >> 24, best[slot] & 0xFFFFFF
        sv = [key >> 16, (key >> 8) & 255, key & 255]
        h["flags"] = W.HIT | (W.OVERLAP if k == 0 else 0) | (W.HIT_WALL if acc[slot][2] else 0)
        h["steps"] = k - 1 if k else 0
        h["contacts"], h["src_key"] = acc[slot][0], key
        for r in range(3):
            p, g = (int(c["orient"]) >> (2 * r)) & 3, (int(c["orient"]) >> (6 + r)) & 1
            u = int(c["src_hi"][p]) - sv[p] if g else sv[p] - int(c["src_lo"][p])
            h["contact"][r] = ((int(c["offset"][r]) + k * int(c["step"][r]) + u + 2 ** 31) % 2 ** 32) - 2 ** 31
    return hits


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(11)
    src = np.zeros((256,) * 3, np.uint8)
    src[10:23, 12:21, 14:20] = rng.random((13, 9, 6)) < 0.4          # over two root cells in x and y, bricks cut by the sub-box
    dst = np.zeros((256,) * 3, np.uint8)
    dst[0:64, 0:64, 0:64] = rng.random((64, 64, 64)) < 0.03
    dst[200:256, 200:256, 200:256] = rng.random((56, 56, 56)) < 0.03
    return src, dst, brick_masks(src), brick_masks(dst)


def test_the_port_matches_the_witness(world):
    src, dst, src_mask, dst_mask = world
    rng = np.random.default_rng(12)
    words = all_orientations()
    steps = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
    n = 240
    base = rng.integers(-20, 70, (n, 3))
    base[n // 2:] += 190
    lim = 2 ** 31
    base[:6] = [(lim - 1, 5, 5), (-lim, 5, 5), (5, lim - 1, -lim), (-300, 20, 20), (20, 20, 400), (250, 250, 250)]
    lo = rng.integers(9, 14, (n, 3))
    casts = W.records(base, [steps[i % 27] for i in range(n)], rng.choice([0, 3, 60, 400, W.MAX_STEPS], n), [words[i % 48] for i in range(n)],
                      rng.integers(0, 2, n), lo, lo + rng.integers(-1, 11, (n, 3)))
    want = W.cast(dst, src, casts)
    assert np.count_nonzero(want["flags"] == 0) > 20 and np.count_nonzero(want["flags"] & W.OVERLAP) > 20
    assert np.count_nonzero(want["flags"] & (W.HIT | W.OVERLAP) == W.HIT) > 20 and np.count_nonzero(want["contacts"] > 1) > 10
    for prune in (True, False):
        got = port_call(dst_mask, src_mask, casts, rng, prune)
        for i in range(n):
            assert got[i].tobytes() == want[i].tobytes(), (i, casts[i], got[i], want[i])
