"""A witness for the upper levels of a model: from the set of occupied bricks to every array the traversal descends through, written
from the format alone -- the layout comments of dust_amd/csrc/dust_dev.h (N16 node: 512 bytes of child mask, 128 of rank prefixes,
4 of child_base, 12 of padding; DevN4; DevL2Cell) and the reader in dust_amd/csrc/traverse.hpp (n16_child, find_brick, resolve_block)
-- and on whole arrays: a sort, np.unique and cumulative sums, no pass through sorted blocks creating nodes on first touch.

    build(bricks, extent_log2) -> dict      bricks: {(bx, by, bz): 64-bit mask}, brick coordinates (voxel >> 2)
    descend(arrays, bx, by, bz) -> block index or -1, the lookup the kernels do, on any such dict (the witness's or a device's)
    bricks_of_grid(grid)                    (256, 256, 256) uint8 grid in tree coordinates [x, y, z] -> the brick dict
"""
import numpy as np

N16_BYTES, N16_ROOT_BYTES = 656, 640
MID_DTYPE = np.dtype([("mask_lo", "<u4"), ("mask_hi", "<u4"), ("first_block", "<u4"), ("pad", "<u4")])
L2_CELL_DTYPE = np.dtype([("mid", "<u4"), ("bounds", "<u4"), ("child_mask", "<u8")])
EMPTY_CELL = 0xFFFFFFFF


def _cell16(x, y, z):
    """index of a child among a node's 16^3: x slowest"""
    return (x << 8) | (y << 4) | z


def _n16(children, child_base):
    """one N16 node from the sorted indices (0..4095) of its children"""
    bits = np.zeros(4096, np.uint8)
    bits[children] = 1
    node = np.zeros(N16_BYTES, np.uint8)
    node[:512] = np.packbits(bits, bitorder="little")                      # bit i of the mask = bit (i & 63) of little-endian word i >> 6
    per_word = bits.reshape(64, 64).sum(axis=1)
    node[512:640] = (np.cumsum(per_word) - per_word).astype("<u2").view(np.uint8)   # children in the words before this one
    node[640:644] = np.array([child_base], "<u4").view(np.uint8)
    return node


def build(bricks, extent_log2):
    assert extent_log2 in (8, 12)
    deep = extent_log2 == 12
    n = len(bricks)
    b = np.array(list(bricks.keys()), np.int64).reshape(n, 3)
    masks = np.array(list(bricks.values()), np.uint64).reshape(n)
    assert n == 0 or (b.min() >= 0 and b.max() < (1 << (extent_log2 - 2)) and masks.min() > 0)
    bit = ((b[:, 0] & 3) << 4) | ((b[:, 1] & 3) << 2) | (b[:, 2] & 3)                       # the brick among its 16-cell's 4^3
    c16 = _cell16((b[:, 0] >> 2) & 15, (b[:, 1] >> 2) & 15, (b[:, 2] >> 2) & 15)          # the 16-cell among its parent's 16^3
    top = _cell16(b[:, 0] >> 6, b[:, 1] >> 6, b[:, 2] >> 6) if deep else np.zeros(n, np.int64)   # the 256-cell among the root's 16^3
    # Tree::iter_leaf: depth first, per level x slowest -- the lexicographic order of (top, c16, bit)
    order = np.argsort((top * 4096 + c16) * 64 + bit, kind="stable")
    b, masks, bit, c16, top = b[order], masks[order], bit[order], c16[order], top[order]
    out = dict(extent_log2=extent_log2, block_xyz=(b * 4).astype(np.uint16), block_mask=masks)
    # mid nodes: one per occupied 16-cell, in the same order; a block's mid node is its rank among them
    mid_key, first_block, mid_of = np.unique(top * 4096 + c16, return_index=True, return_inverse=True)
    n_mid = len(mid_key)
    child_mask = np.zeros(n_mid, np.uint64)
    np.add.at(child_mask, mid_of, np.uint64(1) << bit.astype(np.uint64))    # (distinct bits: the sum is the union)
    mid = np.zeros(n_mid, MID_DTYPE)
    mid["mask_lo"], mid["mask_hi"] = child_mask & np.uint64(0xFFFFFFFF), child_mask >> np.uint64(32)
    mid["first_block"] = first_block
    dense = np.zeros(n_mid * 64, np.uint64)
    dense[mid_of * 64 + bit] = masks
    out.update(n_mid=n_mid, mid=mid, dense_mask=dense)
    if not deep:
        out.update(root=_n16(mid_key, 0), n_l2=0, l2=np.zeros(0, np.uint8), l2_cells=np.zeros(0, L2_CELL_DTYPE))
    else:
        tops, mids_before = np.unique(mid_key >> 12, return_index=True)    # l2 nodes: one per occupied 256-cell; its first mid node
        n_l2 = len(tops)
        ends = np.append(mids_before, n_mid)
        l2 = [_n16(mid_key[ends[i]:ends[i + 1]] & 4095, int(mids_before[i])) for i in range(n_l2)]
        cells = np.zeros(n_l2 * 4096, L2_CELL_DTYPE)
        cells["mid"] = EMPTY_CELL
        at = np.searchsorted(tops, mid_key >> 12) * 4096 + (mid_key & 4095)
        cells["mid"][at] = np.arange(n_mid)
        cells["child_mask"][at] = child_mask
        lo, hi = np.full((n_mid, 3), 3, np.int64), np.zeros((n_mid, 3), np.int64)
        for k, v in enumerate((bit >> 4, (bit >> 2) & 3, bit & 3)):
            np.minimum.at(lo[:, k], mid_of, v)
            np.maximum.at(hi[:, k], mid_of, v)
        cells["bounds"][at] = lo[:, 0] | lo[:, 1] << 2 | lo[:, 2] << 4 | hi[:, 0] << 6 | hi[:, 1] << 8 | hi[:, 2] << 10
        out.update(root=_n16(tops, 0), n_l2=n_l2, l2=np.concatenate(l2) if n_l2 else np.zeros(0, np.uint8), l2_cells=cells)
    out["host_root"] = out["root"][:N16_ROOT_BYTES].copy()
    if n:
        out.update(bmin=(b.min(axis=0) * 4).astype(np.float32), bmax=(b.max(axis=0) * 4 + 4).astype(np.float32))
    else:
        out.update(bmin=np.zeros(3, np.float32), bmax=np.zeros(3, np.float32))
    return out


def _popcount_below(word, bit):
    return bin(word & ((1 << bit) - 1)).count("1")


def n16_child(node, idx):
    """traverse.hpp n16_child on the 656 bytes of one node: bit test, then child_base + prefix + rank inside the word; -1 = no child"""
    w, bit = idx >> 6, idx & 63
    word = int(np.frombuffer(node[w * 8:w * 8 + 8].tobytes(), "<u8")[0])
    if not (word >> bit) & 1:
        return -1
    pre = int(np.frombuffer(node[512 + 2 * w:514 + 2 * w].tobytes(), "<u2")[0])
    base = int(np.frombuffer(node[640:644].tobytes(), "<u4")[0])
    return base + pre + _popcount_below(word, bit)


def descend(arrays, bx, by, bz):
    """The block index the kernels arrive at for brick (bx, by, bz), or -1: root (through l2 and its child_base for a 4096^3 tree) ->
    mid index; dense_mask[mid * 64 + bit] -> is there a brick; first_block + rank of the bit in the mid mask -> block"""
    root = np.asarray(arrays["root"], np.uint8)
    if arrays["extent_log2"] == 12:
        l2 = n16_child(root, _cell16(bx >> 6, by >> 6, bz >> 6))
        if l2 < 0 or l2 >= arrays["n_l2"]:
            return -1
        node = np.asarray(arrays["l2"], np.uint8)[l2 * N16_BYTES:(l2 + 1) * N16_BYTES]
    else:
        node = root
    mid = n16_child(node, _cell16((bx >> 2) & 15, (by >> 2) & 15, (bz >> 2) & 15))
    if mid < 0:
        return -1
    assert mid < arrays["n_mid"], "a set bit leads past the mid nodes in use"
    bit = ((bx & 3) << 4) | ((by & 3) << 2) | (bz & 3)
    if int(arrays["dense_mask"][mid * 64 + bit]) == 0:
        return -1
    m = arrays["mid"][mid]
    return int(m["first_block"]) + _popcount_below(int(m["mask_hi"]) << 32 | int(m["mask_lo"]), bit)


def bricks_of_grid(grid):
    """(256, 256, 256) uint8 grid [x, y, z] in tree coordinates, nonzero = solid -> {(bx, by, bz): mask}, voxel bit x << 4 | y << 2 | z"""
    g = (np.asarray(grid).reshape(64, 4, 64, 4, 64, 4) != 0).transpose(0, 2, 4, 1, 3, 5).reshape(64, 64, 64, 64)
    masks = np.packbits(g, axis=3, bitorder="little").view("<u8")[..., 0]
    return {(int(x), int(y), int(z)): int(masks[x, y, z]) for x, y, z in zip(*np.nonzero(masks))}


def bricks_of_voxels(vox):
    """{(x, y, z): anything} or an iterable of (x, y, z), tree coordinates of any extent -> the brick dict"""
    v = np.array(list(vox), np.int64).reshape(-1, 3)
    out = {}
    for (x, y, z) in v.tolist():
        k = (x >> 2, y >> 2, z >> 2)
        out[k] = out.get(k, 0) | 1 << (((x & 3) << 4) | ((y & 3) << 2) | (z & 3))
    return out


def probes(bricks, extent_log2, rng=None, n_random=64):
    """empty bricks worth asking for: the six neighbours of every occupied one, the eight far corners, and a few random ones"""
    side = 1 << (extent_log2 - 2)
    cand = set()
    for (x, y, z) in bricks:
        for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            c = (x + d[0], y + d[1], z + d[2])
            if min(c) >= 0 and max(c) < side:
                cand.add(c)
    cand.update((x, y, z) for x in (0, side - 1) for y in (0, side - 1) for z in (0, side - 1))
    if rng is not None:
        cand.update(tuple(int(v) for v in c) for c in rng.integers(0, side, (n_random, 3)))
    return sorted(c for c in cand if c not in bricks)
