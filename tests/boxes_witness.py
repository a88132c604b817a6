"""The numpy witness of the model boxes (dust_hip_model_boxes; the contract is in include/dust_hip.h). A helper module, not a test:
tests/test_boxes_witness.py holds it to a brute-force reading of the rule, tests/test_boxes_rule.py the row functions of
dust_amd/csrc/boxes_rule.hpp to it, tests/test_gpu_boxes.py the device.

Written from the header text on whole arrays, with no bit planes. The region and the palette filter first leave the set S in an
otherwise empty array: nothing outside the region exists for the call. Runs come from shifted compares over the whole array (a run
starts where a voxel of S does not follow one of the same name, and ends where none follows it); rects from sorting the runs by
(s, u0, u1, name, v) and cutting where v is not consecutive; boxes from sorting the rects by (v0, v1, u0, u1, name, s) and cutting
where s is not consecutive. The name is the voxel's byte, or 1 for every voxel of S under ANY_PALETTE. The grid holds palette index
+ 1 per voxel, 0 = None, indexed [x, y, z]; it may be any box (the tree is 256^3)."""
import numpy as np

import surface_witness as S

ANY_PALETTE = 1
# per stacking axis n: the grid's axes in the order (n, v, u) -- u the higher-numbered remaining axis, v the other one (the mesh's)
AXES = ((0, 1, 2), (1, 0, 2), (2, 0, 1))

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("axis", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                        ("reserved", "<u4", 2)])
RESULT_DTYPE = np.dtype([("boxes", "<u4"), ("rects", "<u4"), ("voxels", "<u4"), ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"),
                         ("reserved", "<u4", 11)])
BOX_DTYPE = np.dtype([("key", "<u4"), ("palette", "u1"), ("dx", "u1"), ("dy", "u1"), ("dz", "u1")])


def refused(axis, flags, palette, lo, hi):
    """what the call refuses with DUST_ERR_INVALID_ARGUMENT (beyond null pointers and struct_size)"""
    return bool(axis > 2 or (flags & ~ANY_PALETTE) or palette < -1 or palette > 254 or max(*lo, *hi) >= 256)


def zero_result():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["lo"] = 255
    return r


def the_set(grid, palette=-1, region=None):
    """the grid with everything that is not in S emptied: outside the region, or of another palette index under a filter"""
    out = np.zeros_like(grid)
    box = S.clip(grid, region)
    if box is not None:
        out[box] = grid[box]
        if palette >= 0:
            out[out != palette + 1] = 0
    return out


def crop(grid, palette=-1, region=None):
    """(the part of the_set that holds all of S, its origin): the region, then the bounds of what is solid in it -- the rule looks at
    nothing else, and a small region costs little"""
    box = S.clip(grid, region)
    if box is None:
        return np.zeros((0, 0, 0), grid.dtype), (0, 0, 0)
    part = grid[box]
    if palette >= 0:
        part = np.where(part == palette + 1, part, 0).astype(grid.dtype)
    cuts = []
    for axis in range(3):
        held = np.flatnonzero(part.any(axis=tuple(k for k in range(3) if k != axis)))
        cuts.append(slice(int(held[0]), int(held[-1]) + 1) if len(held) else slice(0, 0))
    return part[tuple(cuts)], tuple(b.start + c.start for b, c in zip(box, cuts))


def decompose(grid, axis=0, palette=-1, region=None, any_palette=False):
    """(runs, rects, boxes) of the set, each a dict of equally long int64 columns in slice coordinates: runs s, v, u0, u1, name, byte;
    rects s, v0, v1, u0, u1, name, byte; boxes s0, s1, v0, v1, u0, u1, name, byte. `byte` is that of the lowest corner voxel. The
    boxes come in the documented order, ascending (s0, v0, u0)."""
    part, origin = crop(grid, palette, region)
    a = np.transpose(part, AXES[axis])                                            # [s, v, u]
    base = [origin[k] for k in AXES[axis]]
    solid = a != 0
    name = solid.astype(np.uint8) if any_palette else a
    start, end = solid.copy(), solid.copy()
    start[:, :, 1:] &= name[:, :, 1:] != name[:, :, :-1]                          # (an empty voxel's name is 0: no voxel of S has it)
    end[:, :, :-1] &= name[:, :, :-1] != name[:, :, 1:]
    first, last = np.argwhere(start), np.argwhere(end)                            # both row by row, along u: the k-th start and the k-th end are one run's
    assert len(first) == len(last) and np.array_equal(first[:, :2], last[:, :2]) and np.all(first[:, 2] <= last[:, 2])
    runs = dict(s=first[:, 0] + base[0], v=first[:, 1] + base[1], u0=first[:, 2] + base[2], u1=last[:, 2] + base[2], name=name[start].astype(np.int64),
                byte=a[start].astype(np.int64))

    def cut(table, keys, along):
        """sort by keys + (along,); groups of equal keys and consecutive `along`: (sorted table, index of each group's first, last)"""
        order = np.lexsort([table[along]] + [table[k] for k in reversed(keys)])
        t = {k: c[order] for k, c in table.items()}
        same = np.zeros(len(order), bool)
        if len(order):
            same[1:] = t[along][1:] == t[along][:-1] + 1
            for k in keys:
                same[1:] &= t[k][1:] == t[k][:-1]
        head = np.flatnonzero(~same)
        return t, head, (np.append(head[1:], len(order)) - 1)[:len(head)]            # (nothing sorted: no group)

    t, head, tail = cut(runs, ("s", "u0", "u1", "name"), "v")
    rects = dict(s=t["s"][head], v0=t["v"][head], v1=t["v"][tail], u0=t["u0"][head], u1=t["u1"][head], name=t["name"][head], byte=t["byte"][head])
    t, head, tail = cut(rects, ("v0", "v1", "u0", "u1", "name"), "s")
    boxes = dict(s0=t["s"][head], s1=t["s"][tail], v0=t["v0"][head], v1=t["v1"][head], u0=t["u0"][head], u1=t["u1"][head], name=t["name"][head],
                 byte=t["byte"][head])
    order = np.lexsort((boxes["u0"], boxes["v0"], boxes["s0"]))
    return runs, rects, {k: c[order] for k, c in boxes.items()}


def boxes(grid, axis=0, palette=-1, region=None, any_palette=False):
    """(result, boxes) of a call with room for every box"""
    assert not refused(axis, 0, palette, (0, 0, 0), (0, 0, 0))
    result = zero_result()
    _, rects, b = decompose(grid, axis, palette, region, any_palette)
    out = np.zeros(len(b["s0"]), BOX_DTYPE)
    if len(out) == 0:
        return result, out
    n_axis, v_axis, u_axis = AXES[axis]
    lo, hi = np.zeros((len(out), 3), np.int64), np.zeros((len(out), 3), np.int64)
    lo[:, n_axis], lo[:, v_axis], lo[:, u_axis] = b["s0"], b["v0"], b["u0"]
    hi[:, n_axis], hi[:, v_axis], hi[:, u_axis] = b["s1"], b["v1"], b["u1"]
    out["key"] = (lo[:, 0] << 16) | (lo[:, 1] << 8) | lo[:, 2]
    out["palette"] = b["byte"] - 1                                                # (under any_palette: that of the key voxel)
    out["dx"], out["dy"], out["dz"] = (hi - lo).T
    result["boxes"], result["rects"] = len(out), len(rects["s"])
    result["voxels"] = (hi - lo + 1).prod(axis=1).sum()
    result["lo"], result["hi"] = lo.min(axis=0), hi.max(axis=0)
    return result, out


def bounds(records):
    """(lo, hi) int64 (N, 3), inclusive, of BOX_DTYPE records"""
    key = records["key"].astype(np.int64)
    lo = np.stack([key >> 16, (key >> 8) & 255, key & 255], axis=1)
    return lo, lo + np.stack([records["dx"], records["dy"], records["dz"]], axis=1).astype(np.int64)


def paint(records, shape, with_palette=False):
    """how many boxes cover each voxel (uint16); with_palette: also the grid the records describe, palette index + 1 per voxel"""
    count, bytes_ = np.zeros(shape, np.uint16), np.zeros(shape, np.uint8)
    lo, hi = bounds(records)
    assert len(records) == 0 or np.all(hi.max(axis=0) < np.array(shape)), "a box reaches past the grid"
    for (x0, y0, z0), (x1, y1, z1), p in zip(lo.tolist(), hi.tolist(), records["palette"].tolist()):
        count[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] += 1
        bytes_[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = p + 1
    return (count, bytes_) if with_palette else count
