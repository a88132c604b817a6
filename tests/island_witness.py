"""The numpy witness of the model islands (dust_hip_model_find_islands / island_of / detach_islands; the contract is in
include/dust_hip.h). A helper module, not a test file: written from the header text alone, it shares no code with the device path.

Grids are uint8 [x, y, z] arrays of up to 256 per axis holding palette index + 1 (0 = empty), the convention of
tests/shape_edit_witness.py. An island is a maximal set of solid voxels connected through shared faces (FACES) or through shared faces,
edges and corners (CORNERS); its key is x << 16 | y << 8 | z of its voxel with the smallest such value.

Labelling is hooking and pointer jumping on flat indices, inside the bounding box of the solid voxels (C-order flat indices of a box
order voxels as the keys do): every round a voxel takes the smallest label among itself and its solid neighbours, the voxel its old
label names is handed that label as well (hooking), and every label is replaced by the label of the voxel it names (jumping), until
nothing changes. Labels only decrease, always name a voxel of the same island and never exceed the voxel's own index, so the fixed
point is the island's smallest voxel."""
import itertools

import numpy as np

FACES, CORNERS = 0, 1
ANCHORED = 1
NO_ISLAND = 0xFFFFFFFF
KEEP_SOURCE = 1
EXTENT = 256

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("connectivity", "<u4"), ("anchor_lo", "<u4", 3), ("anchor_hi", "<u4", 3)])
ISLAND_DTYPE = np.dtype([("key", "<u4"), ("voxels", "<u4"), ("lo", "u1", 3), ("flags", "u1"), ("hi", "u1", 3), ("reserved", "u1"),
                         ("sum", "<u8", 3)])


def offsets(connectivity):
    """half of the neighbourhood: one of every pair of opposite offsets"""
    if connectivity == FACES:
        return [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    assert connectivity == CORNERS
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]


def _pair(shape, d):
    """slices (a, b) of an array of `shape` with b = a shifted by the offset d"""
    a, b = [], []
    for n, s in zip(shape, d):
        a.append(slice(0, n - 1) if s == 1 else slice(1, n) if s == -1 else slice(0, n))
        b.append(slice(1, n) if s == 1 else slice(0, n - 1) if s == -1 else slice(0, n))
    return tuple(a), tuple(b)


def label(grid, connectivity=FACES):
    """uint32 array of the grid's shape: per voxel the key of its island, NO_ISLAND where the voxel is empty"""
    grid = np.asarray(grid)
    assert grid.ndim == 3 and max(grid.shape) <= EXTENT
    out = np.full(grid.shape, NO_ISLAND, np.uint32)
    solid_all = grid != 0
    if not solid_all.any():
        return out
    box = tuple(slice(int(np.flatnonzero(solid_all.any(axis=tuple(k for k in range(3) if k != r)))[0]),
                      int(np.flatnonzero(solid_all.any(axis=tuple(k for k in range(3) if k != r)))[-1]) + 1) for r in range(3))
    solid = solid_all[box]
    shape = solid.shape
    big = np.int64(solid.size)
    lab = np.where(solid, np.arange(solid.size, dtype=np.int64).reshape(shape), big)
    pairs = [_pair(shape, d) for d in offsets(connectivity)]
    where = np.flatnonzero(solid)
    while True:
        near = lab.copy()
        for a, b in pairs:
            both = solid[a] & solid[b]
            lo = np.minimum(lab[a], lab[b])
            np.copyto(near[a], np.minimum(near[a], lo), where=both)
            np.copyto(near[b], np.minimum(near[b], lo), where=both)
        flat, near_flat = lab.reshape(-1), near.reshape(-1)
        new = near_flat.copy()
        np.minimum.at(new, flat[where], near_flat[where])        # hooking: the voxel a label names hears of the smaller one
        while True:                                               # jumping
            jumped = new.copy()
            jumped[where] = new[new[where]]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, flat):
            break
        lab = new.reshape(shape)
    x, y, z = np.unravel_index(lab.reshape(-1)[where], shape)
    keys = ((x + box[0].start) << 16) | ((y + box[1].start) << 8) | (z + box[2].start)
    inside = np.full(shape, NO_ISLAND, np.uint32)
    inside.reshape(-1)[where] = keys.astype(np.uint32)
    out[box] = inside
    return out


def records(labels, anchor=None):
    """the 40-byte records of every island in ascending key order; anchor: (lo, hi), an inclusive voxel box clipped to the tree"""
    labels = np.asarray(labels, np.uint32)
    xyz = np.argwhere(labels != NO_ISLAND)
    of = labels[labels != NO_ISLAND]
    keys, inverse = np.unique(of, return_inverse=True)
    out = np.zeros(len(keys), ISLAND_DTYPE)
    out["key"] = keys
    if not len(keys):
        return out
    out["voxels"] = np.bincount(inverse, minlength=len(keys))
    order = np.argsort(inverse, kind="stable")
    starts = np.searchsorted(inverse[order], np.arange(len(keys)))
    for r in range(3):
        c = xyz[order, r]
        out["lo"][:, r] = np.minimum.reduceat(c, starts)
        out["hi"][:, r] = np.maximum.reduceat(c, starts)
        out["sum"][:, r] = np.add.reduceat(c.astype(np.uint64), starts)
    if anchor is not None:
        lo = np.asarray(anchor[0], np.int64)
        hi = np.minimum(np.asarray(anchor[1], np.int64), EXTENT - 1)
        if np.all(lo <= hi):
            inside = np.all((xyz >= lo) & (xyz <= hi), axis=1)
            out["flags"] = np.where(np.bincount(inverse, weights=inside, minlength=len(keys)) > 0, ANCHORED, 0)
    return out


def island_of(labels, xyz):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    return np.asarray(labels, np.uint32)[xyz[:, 0], xyz[:, 1], xyz[:, 2]]


def detach(grid, labels, keys):
    """(piece, rest): the grid of the named islands' voxels and the grid of everything else; a key that names no island is an error"""
    labels = np.asarray(labels, np.uint32)
    keys = np.unique(np.asarray(keys, np.uint32).reshape(-1))
    for k in keys:
        k = int(k)
        assert k < 1 << 24 and labels[k >> 16, (k >> 8) & 255, k & 255] == k, f"{k:#x} does not name an island"
    moves = np.isin(labels, keys) & (labels != NO_ISLAND)
    return np.where(moves, grid, 0).astype(np.uint8), np.where(moves, 0, grid).astype(np.uint8)


def voxels(grid):
    """(xyz [n, 3], palette index [n]) of a grid's solid voxels, in key order"""
    xyz = np.argwhere(np.asarray(grid) != 0)
    return xyz, grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int64) - 1


# ---------------------------------------------------------------- scenes the tests share
def to_xyzi(grid):
    """a grid's voxels as the .vox rows api.flatten_model takes: tree (x, y, z) is file (x, 255 - z, y) (loader.rs:248-253)"""
    xyz, pal = voxels(grid)
    return np.stack([xyz[:, 0], 255 - xyz[:, 2], xyz[:, 1], pal], axis=1).astype(np.uint8)


def full(grid):
    """the grid embedded at the origin of a 256^3 tree"""
    out = np.zeros((EXTENT,) * 3, np.uint8)
    out[tuple(slice(0, n) for n in grid.shape)] = grid
    return out


def random_fill(seed, density, size=64, origin=(24, 40, 56)):
    """a seeded random fill of a size^3 region (its origin off the brick lattice on purpose), random materials"""
    rng = np.random.default_rng(seed)
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    region = tuple(slice(o, o + size) for o in origin)
    grid[region] = np.where(rng.random((size,) * 3) < density, rng.integers(1, 256, (size,) * 3), 0)
    return grid


def snake_path():
    """A one-voxel-thick path: rows along x joined at alternating ends (every row runs against its predecessor), on three levels
    joined by columns, 5 root cells long, 3 wide and 3 high. Consecutive voxels share a face and rows keep two empty voxels between
    them, so it is one island under both connectivities and no edge or corner contact shortens the way along it."""
    path = []
    x0, x1 = 3, 77
    levels = (5, 21, 37)
    forward = True
    for level, y in enumerate(levels):
        rows = list(range(2, 45, 3))
        if level % 2:
            rows.reverse()
        for k, z in enumerate(rows):
            xs = range(x0, x1 + 1) if forward else range(x1, x0 - 1, -1)
            path += [(x, y, z) for x in xs]
            if k + 1 < len(rows):
                step = 1 if rows[k + 1] > z else -1
                path += [(path[-1][0], y, zz) for zz in range(z + step, rows[k + 1], step)]
            forward = not forward
        if level + 1 < len(levels):
            x, _, z = path[-1]
            path += [(x, yy, z) for yy in range(y + 1, levels[level + 1])]
    return path


def snake():
    path = snake_path()
    assert len(set(path)) == len(path)
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    p = np.array(path)
    grid[p[:, 0], p[:, 1], p[:, 2]] = 1 + np.arange(len(p)) % 200
    return grid, p


def checkerboard(size=64):
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    x, y, z = np.indices((size,) * 3)
    grid[:size, :size, :size] = np.where((x + y + z) % 2 == 0, 7, 0)
    return grid


PAIR_KINDS = (("face", (2, 0, 0), 1, 1), ("edge", (2, 2, 0), 2, 1), ("corner", (2, 2, 2), 2, 1), ("apart", (3, 0, 0), 2, 2))


def cube_pairs():
    """[(name, a voxel of cube A, a voxel of cube B, islands under FACES, under CORNERS)] and the grid: two 2^3 cubes per entry, A ending
    at a lattice boundary on every axis and B displaced from it by the kind's offset rotated onto each axis in turn -- the boundary
    a brick's (8 mod 16) and a root cell's (0 mod 16)."""
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    out = []
    i = 0
    for boundary, b in (("brick", 8), ("root", 16)):
        for axis in range(3):
            for kind, offset, faces, corners in PAIR_KINDS:
                base = np.array([32 * (i % 6), 32 * (i // 6), 32]) + b - 2
                d = np.roll(np.array(offset), axis)
                for cube, colour in ((base, 3), (base + d, 4)):
                    grid[cube[0]:cube[0] + 2, cube[1]:cube[1] + 2, cube[2]:cube[2] + 2] = colour
                out.append((f"{kind}/{boundary}/axis{axis}", tuple(base), tuple(base + d), faces, corners))
                i += 1
    return out, grid


def terrain():
    """the terrain block of tools/shape_edit_timing.py (y < 128, three layers of material) with a pillar on it whose top a carved
    slab has cut loose; returns (grid, a voxel of the floating top)"""
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    grid[:, :96, :] = 2
    grid[:, 96:120, :] = 3
    grid[:, 120:128, :] = 4
    grid[100:120, 128:200, 90:110] = 5
    grid[100:120, 150:154, 90:110] = 0
    return grid, (100, 154, 90)
