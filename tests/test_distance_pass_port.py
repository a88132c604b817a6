"""The passes of dust_amd/csrc/distance.hip (k_distance_bits, k_distance_scan) ported to numpy line by line and run against the witness
on the random fixture: the brick-major addressing of the field and of the brick columns, the padded LDS lines, pass x's bit scan on
64-bit words, the outward scan with its stopping rule evaluated over groups of 64 lanes (a wave), the all-FAR line vote, the limit
after every pass and the WALLS fold of the last pass's store. Every address formed must lie inside the 32 MiB field and every LDS
index inside the column's array. It checks the algorithm without a device; tests/test_gpu_distance.py checks the kernels."""
import functools

import numpy as np
import pytest

import distance_witness as W

FAR = W.FAR
PAD = 256
STRIDE = 256 + 2 * PAD + 4          # kStride
NO_BIT = 1024
LATTICE = 64 ** 3
LANE = np.arange(64, dtype=np.int64)


def leaf_code(bx, by, bz):
    return ((((bx >> 2) << 8) | ((by >> 2) << 4) | (bz >> 2)) << 6) | ((bx & 3) << 4) | ((by & 3) << 2) | (bz & 3)


def voxel_index(x, y, z):
    return leaf_code(x >> 2, y >> 2, z >> 2) * 64 + (((x & 3) << 4) | ((y & 3) << 2) | (z & 3))


def bit_along(axis, bit):
    return (bit >> (4 - 2 * axis)) & 3


def bit_line(axis, bit):
    s = 4 - 2 * axis
    return ((bit >> (s + 2)) << s) | (bit & ((1 << s) - 1))


@functools.lru_cache(maxsize=None)
def column_addresses(axis):
    """per column (u, v), brick b and lane: the field element the lane loads or stores, and its LDS index (store_column)"""
    u, v, b = np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing="ij")
    code = leaf_code(b, u, v) if axis == 0 else leaf_code(u, b, v) if axis == 1 else leaf_code(u, v, b)
    address = (code[..., None] * 64 + LANE).reshape(4096, 4096)
    lds = (bit_line(axis, LANE) * STRIDE + PAD + bit_along(axis, LANE) + b[..., None] * 4).reshape(4096, 4096)
    assert address.min() >= 0 and address.max() * 2 + 1 < 32 << 20 and len(np.unique(address)) == LATTICE * 64
    assert lds.min() >= 0 and lds.max() < 16 * STRIDE
    return address, lds


def clz64(x):
    """count of leading zeros of non-zero uint64 values"""
    x = x.copy()
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        top = (x >> np.uint64(64 - s)) == 0
        n += np.where(top, s, 0)
        x = np.where(top, x << np.uint64(s), x)
    return n


def ctz64(x):
    low = x & (~x + np.uint64(1))
    return 63 - clz64(low)


def pass_bits(grid_flat, mask, q):
    """k_distance_bits: the field after pass x, from the brick masks (or the grid bytes' ballots under TO_MATERIAL)"""
    field = np.full(LATTICE * 64, 0xABCD, np.uint16)
    address, lds = column_addresses(0)
    column = np.arange(4096)
    u, v = column >> 6, column & 63
    codes = leaf_code(np.arange(64)[None, :], u[:, None], v[:, None])                    # [column, brick]
    if q["target"] == W.TO_MATERIAL:
        hit = grid_flat.reshape(LATTICE, 64)[codes] == q["byte"]                         # the ballot: lane = bit
        m = (hit.astype(np.uint64) << LANE.astype(np.uint64)).sum(axis=-1, dtype=np.uint64)
    else:
        m = mask[codes]
        m = ~m if q["target"] == W.TO_EMPTY else m
    col = np.zeros((4096, 16 * STRIDE), np.uint16)
    for line in range(16):
        w = []
        for p in range(4):
            i = p * 64 + LANE
            t = (m[:, i >> 2] >> (((i & 3) << 4) | line).astype(np.uint64)) & np.uint64(1)
            w.append((t << LANE.astype(np.uint64)).sum(axis=-1, dtype=np.uint64))       # [column]
        for p in range(4):
            d_lo = np.full((4096, 64), NO_BIT, np.int64)
            d_hi = np.full((4096, 64), NO_BIT, np.int64)
            for pp in range(p):
                has = w[pp] != 0
                d = LANE[None, :] + (p - pp) * 64 - 63 + clz64(np.where(has, w[pp], np.uint64(1)))[:, None]
                d_lo = np.where(has[:, None], d, d_lo)
            for pp in range(3, p, -1):
                has = w[pp] != 0
                d = (pp - p) * 64 + ctz64(np.where(has, w[pp], np.uint64(1)))[:, None] - LANE[None, :]
                d_hi = np.where(has[:, None], d, d_hi)
            below = w[p][:, None] & (np.uint64(0xFFFFFFFFFFFFFFFF) >> (63 - LANE).astype(np.uint64))[None, :]
            above = w[p][:, None] >> LANE.astype(np.uint64)[None, :]
            d_lo = np.where(below != 0, LANE[None, :] - 63 + clz64(np.where(below != 0, below, np.uint64(1))), d_lo)
            d_hi = np.where(above != 0, ctz64(np.where(above != 0, above, np.uint64(1))), d_hi)
            d = np.minimum(d_lo, d_hi)
            assert d.min() >= 0
            value = np.where(d > q["radius"], FAR, d * d if q["metric"] == W.EUCLIDEAN else d)
            col[:, line * STRIDE + PAD + p * 64:line * STRIDE + PAD + p * 64 + 64] = value
    field[address] = np.take_along_axis(col, lds, axis=1)
    return field


def pass_scan(field, axis, last, q):
    """k_distance_scan, in place on the field; returns the longest scan (in steps of k) any wave made"""
    address, lds = column_addresses(axis)
    col = np.full((4096, 16 * STRIDE), 0x1234, np.uint16)
    lines = col.reshape(4096, 16, STRIDE)
    lines[:, :, :PAD] = FAR
    lines[:, :, PAD + 256:PAD + 256 + PAD] = FAR
    np.put_along_axis(col, lds, field[address], axis=1)
    radius, limit, euclid = q["radius"], q["limit"], q["metric"] == W.EUCLIDEAN
    out = lines[:, :, PAD:PAD + 256].astype(np.int64).reshape(4096, 16, 4, 64)
    voted = (out != FAR).any(axis=(2, 3))                                    # the wave vote over a whole line
    c, l, p = np.nonzero(np.broadcast_to(voted[:, :, None], (4096, 16, 4)))  # the waves' scans: one group of 64 lanes each
    best = out[c, l, p]
    at = PAD + p[:, None] * 64 + LANE[None, :]
    done = np.zeros(len(c), bool)
    longest = 0
    for k in range(1, radius + 1):
        kk = k * k if euclid else k
        done |= ~(kk < best).any(axis=1)                                     # (a wave that broke out stays out)
        go = np.flatnonzero(~done)
        if len(go) == 0:
            break
        longest = k
        assert at[go].min() - k >= 0 and at[go].max() + k < STRIDE
        g = np.minimum(lines[c[go, None], l[go, None], at[go] - k], lines[c[go, None], l[go, None], at[go] + k]).astype(np.int64)
        best[go] = np.minimum(best[go], g + kk if euclid else np.maximum(g, kk))
    out[c, l, p] = np.where(best > limit, FAR, best)
    if last and q["walls"]:
        column = np.arange(4096)
        u, v = column >> 6, column & 63
        line = np.arange(16)
        c1 = (u[:, None] * 4 + (line >> 2)[None, :])[:, :, None, None]
        c2 = (v[:, None] * 4 + (line & 3)[None, :])[:, :, None, None]
        i = (np.arange(4)[:, None] * 64 + LANE[None, :])[None, None, :, :]
        w = np.minimum(np.minimum(np.minimum(c1 + 1, 256 - c1), np.minimum(c2 + 1, 256 - c2)), np.minimum(i + 1, 256 - i))
        out = np.minimum(out, np.where(w > radius, FAR, w * w if euclid else w))
    lines[:, :, PAD:PAD + 256] = out.reshape(4096, 16, 256)
    field[address] = np.take_along_axis(col, lds, axis=1)
    return longest


@pytest.fixture(scope="module")
def fixture():
    """the random fill brick-major, its brick masks, and where each voxel (x, y, z) lives in the field"""
    grid, _ = W.random_fill()
    x, y, z = np.indices((256, 256, 256))
    index = voxel_index(x, y, z)
    flat = np.zeros(LATTICE * 64, np.uint8)
    flat[index] = grid
    mask = ((flat.reshape(LATTICE, 64) != 0).astype(np.uint64) << LANE.astype(np.uint64)).sum(axis=-1, dtype=np.uint64)
    return grid, flat, mask, index


CASES = ((W.TO_SOLID, W.EUCLIDEAN, 20, False), (W.TO_SOLID, W.CHEBYSHEV, 3, True), (W.TO_EMPTY, W.EUCLIDEAN, 3, False),
         (W.TO_MATERIAL, W.CHEBYSHEV, 20, False), (W.TO_MATERIAL, W.EUCLIDEAN, 3, True), (W.TO_EMPTY, W.CHEBYSHEV, 1, True))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_port_gives_the_witness_field(fixture, case):
    grid, flat, mask, index = fixture
    target, metric, radius, walls = case
    q = dict(target=target, metric=metric, radius=radius, limit=W.limit_of(metric, radius), walls=walls, byte=W.RANDOM_PALETTE + 1)   # device_distance
    field = pass_bits(flat, mask, q)
    assert not (field == 0xABCD).any()                                       # every element of the field was written
    steps = [pass_scan(field, 1, False, q), pass_scan(field, 2, True, q)]
    want = W.field(grid, target, metric, radius, walls, W.RANDOM_PALETTE)
    assert np.array_equal(field[index], want)
    assert max(steps) <= radius
    r = W.result(want)
    assert int(r["targets"]) > 0 and int(r["near"]) > 0
