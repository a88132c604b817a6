"""Model fracture as include/dust_hip.h defines it, on whole numpy arrays -- the witness the device (tests/test_gpu_fracture.py) and
the rule header (tests/test_fracture_rule.py) are held to. A grid is a (256, 256, 256) uint8 array, 0 = None, otherwise palette index +
1. Labels are found by brute force: for every counted voxel the (d2, index) argmin over ALL seeds, in chunks of seeds, with no pruning
of any kind; records, cut faces and seams by shifted compares; detach and apply as array operations. tests/test_fracture_witness.py
holds this file to independent statements."""
import numpy as np

EXTENT = 256
MAX_SEEDS = 4096
SEED_MIN, SEED_MAX = -1024, 1279
MAX_SCALE = 16
NO_LIMIT = 0xFFFFFFFF
NO_CELL = 0xFFFF
SEAMS, LABELLED = 0, 1

SEED_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("reserved", "<u4")])
QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("max_distance2", "<u4"), ("scale", "u1", 3), ("reserved0", "u1"),
                        ("lo", "<u4", 3), ("hi", "<u4", 3), ("reserved", "<u4")])
RESULT_DTYPE = np.dtype([("solid", "<u4"), ("labelled", "<u4"), ("cells", "<u4"), ("largest_cell", "<u4"), ("largest_voxels", "<u4"), ("cut_faces", "<u4"),
                         ("max_d2", "<u4"), ("lo", "u1", 3), ("reserved0", "u1"), ("hi", "u1", 3), ("reserved1", "u1"), ("reserved", "<u4", 7)])
CELL_DTYPE = np.dtype([("voxels", "<u4"), ("cut_faces", "<u4"), ("lo", "u1", 3), ("reserved0", "u1"), ("hi", "u1", 3), ("reserved1", "u1"), ("sum", "<u8", 3)])


def refused(palette=-1, scale=(1, 1, 1), flags=0, reserved0=0, reserved=0, seeds=(), seed_reserved=0):
    """what dust_hip_model_fracture refuses in a query and its seeds (beyond nulls, sizes and counts)"""
    if any(not 1 <= int(s) <= MAX_SCALE for s in scale):
        return True
    if not -1 <= int(palette) <= 254 or flags != 0 or reserved0 != 0 or reserved != 0 or seed_reserved != 0:
        return True
    return any(not SEED_MIN <= int(c) <= SEED_MAX for s in seeds for c in s)


def apply_refused(where, value):
    return where not in (SEAMS, LABELLED) or not -1 <= value <= 254


def clip(region):
    """(lo, hi) clipped to the tree as dust_hip_model_columns clips it, or None for the empty region"""
    lo, hi = ((0, 0, 0), (EXTENT - 1,) * 3) if region is None else region
    lo, hi = [int(v) for v in lo], [min(int(v), EXTENT - 1) for v in hi]
    return None if any(a > b for a, b in zip(lo, hi)) else (lo, hi)


def counted(grid, region=None, palette=None):
    """the voxels a fracture counts: solid, inside the region, of the filter's palette index"""
    box = clip(region)
    out = np.zeros(grid.shape, bool)
    if box is None:
        return out
    (x0, y0, z0), (x1, y1, z1) = box
    part = grid[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1]
    out[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = (part != 0) if palette is None else (part == int(palette) + 1)
    return out


def nearest(points, seeds, scale=(1, 1, 1), chunk=64):
    """for each of the (n, 3) points the (d2, index) minimum over all seeds, lexicographic: brute force in chunks of seeds"""
    points = np.asarray(points, np.int64).reshape(-1, 3)
    seeds = np.asarray(seeds, np.int64).reshape(-1, 3)
    best = np.full(len(points), np.iinfo(np.int64).max, np.int64)
    index = np.full(len(points), NO_CELL, np.int64)
    s = np.asarray(scale, np.int64)
    for c0 in range(0, len(seeds), chunk):
        part = seeds[c0:c0 + chunk]
        d = points[:, None, :] - part[None, :, :]
        d2 = (d * d * s).sum(axis=2)
        k = d2.argmin(axis=1)                 # the first minimum: the lowest index of the chunk
        v = d2[np.arange(len(points)), k]
        better = v < best                     # strictly: an earlier chunk keeps its ties
        best[better] = v[better]
        index[better] = c0 + k[better]
    return best, index


def labels(grid, seeds, region=None, palette=None, scale=(1, 1, 1), max_distance2=None):
    """(labels, d2): a uint16 array of the grid's shape, NO_CELL where a voxel is not labelled, and the labelled voxels' d2 to their seed (0
    elsewhere)"""
    seeds = np.asarray(seeds, np.int64).reshape(-1, 3)
    out = np.full(grid.shape, NO_CELL, np.uint16)
    far = np.zeros(grid.shape, np.int64)
    xyz = np.argwhere(counted(grid, region, palette))
    if len(xyz) and len(seeds):
        best, index = nearest(xyz, seeds, scale)
        keep = np.ones(len(xyz), bool) if max_distance2 is None or max_distance2 == NO_LIMIT else best <= int(max_distance2)
        xyz, best, index = xyz[keep], best[keep], index[keep]
        out[xyz[:, 0], xyz[:, 1], xyz[:, 2]] = index
        far[xyz[:, 0], xyz[:, 1], xyz[:, 2]] = best
    return out, far


def at(lab, xyz):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return lab[xyz[:, 0], xyz[:, 1], xyz[:, 2]]


def face_counts(lab):
    """(other, higher): per voxel, its face-neighbours labelled with another cell / with a higher cell (0 for an unlabelled voxel; there
    is no neighbour outside the array). Shifted compares, on the labelled voxels' bounding box with a shell of NO_CELL around it."""
    other = np.zeros(lab.shape, np.uint8)
    higher = np.zeros(lab.shape, np.uint8)
    own = lab != NO_CELL
    if not own.any():
        return other, higher
    spans = [np.flatnonzero(own.any(axis=tuple(a for a in range(3) if a != r))) for r in range(3)]
    box = tuple(slice(int(s[0]), int(s[-1]) + 1) for s in spans)
    inner = (slice(1, -1),) * 3
    sub = np.full(tuple(b.stop - b.start + 2 for b in box), NO_CELL, lab.dtype)
    sub[inner] = lab[box]
    mid = sub[inner]
    o = np.zeros(mid.shape, np.uint8)
    h = np.zeros(mid.shape, np.uint8)
    for axis in range(3):
        for step in (0, 2):                           # the neighbour below / above on this axis
            shifted = list(inner)
            shifted[axis] = slice(step, sub.shape[axis] - 2 + step)
            n = sub[tuple(shifted)]
            both = (mid != NO_CELL) & (n != NO_CELL)
            o += both & (n != mid)
            h += both & (n > mid)
    other[box], higher[box] = o, h
    return other, higher


def seams(lab):
    return face_counts(lab)[1] != 0


def cells(lab, n_seeds):
    """the CELL_DTYPE records of the n_seeds cells"""
    out = np.zeros(n_seeds, CELL_DTYPE)
    out["lo"] = 255
    xyz = np.argwhere(lab != NO_CELL)
    if len(xyz) == 0:
        return out
    which = lab[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int64)
    other = face_counts(lab)[0][xyz[:, 0], xyz[:, 1], xyz[:, 2]]
    out["voxels"] = np.bincount(which, minlength=n_seeds)
    out["cut_faces"] = np.bincount(which, weights=other, minlength=n_seeds).astype(np.uint32)
    for r in range(3):
        out["sum"][:, r] = np.bincount(which, weights=xyz[:, r], minlength=n_seeds).astype(np.uint64)
        lo = np.full(n_seeds, 255, np.int64)
        hi = np.zeros(n_seeds, np.int64)
        np.minimum.at(lo, which, xyz[:, r])
        np.maximum.at(hi, which, xyz[:, r])
        out["lo"][:, r], out["hi"][:, r] = lo, hi
    return out


def result(grid, lab, far, region=None, palette=None, n_seeds=0):
    """the RESULT_DTYPE record"""
    r = np.zeros(1, RESULT_DTYPE)
    r["lo"] = 255
    r["largest_cell"] = 0xFFFFFFFF
    r["solid"] = np.count_nonzero(counted(grid, region, palette))
    xyz = np.argwhere(lab != NO_CELL)
    r["labelled"] = len(xyz)
    if len(xyz):
        r["max_d2"] = far.max()
        r["lo"], r["hi"] = xyz.min(axis=0), xyz.max(axis=0)
        r["cut_faces"] = int(face_counts(lab)[1].sum(dtype=np.int64))
        count = np.bincount(lab[lab != NO_CELL].astype(np.int64), minlength=n_seeds)
        r["cells"] = np.count_nonzero(count)
        r["largest_cell"] = int(count.argmax())          # the first maximum: the lowest index among equals
        r["largest_voxels"] = count.max()
    return r[0]


def detach(grid, lab, which):
    """(piece, rest, labels afterwards) of a carving detach of the cells `which`"""
    moves = (lab != NO_CELL) & np.isin(lab, np.asarray(which, np.int64)) & (grid != 0)
    piece = np.where(moves, grid, 0).astype(np.uint8)
    rest = np.where(moves, 0, grid).astype(np.uint8)
    return piece, rest, np.where(moves, NO_CELL, lab).astype(np.uint16)


def apply(grid, lab, where, value):
    """(grid afterwards, changed)"""
    chosen = seams(lab) if where == SEAMS else lab != NO_CELL
    byte = 0 if value < 0 else value + 1
    differs = chosen & (grid != byte)
    return np.where(differs, byte, grid).astype(np.uint8), int(np.count_nonzero(differs))


def to_xyzi(grid):
    """a grid's voxels as the .vox rows api.flatten_model takes: tree (x, y, z) is file (x, 255 - z, y)"""
    xyz = np.argwhere(np.asarray(grid) != 0)
    pal = grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int64) - 1
    return np.stack([xyz[:, 0], 255 - xyz[:, 2], xyz[:, 1], pal], axis=1).astype(np.uint8)


def seed_records(points):
    points = np.asarray(points, np.int64).reshape(-1, 3)
    out = np.zeros(len(points), SEED_DTYPE)
    out["x"], out["y"], out["z"] = points[:, 0], points[:, 1], points[:, 2]
    return out
