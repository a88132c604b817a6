"""The numpy witness of the model floods (dust_hip_model_flood / flood_at / flood_paths / flood_apply; the contract is in
include/dust_hip.h). A helper module, not a test file: written from the header text alone, it shares no code with the device path.

Grids are uint8 [x, y, z] arrays of up to 256 per axis holding palette index + 1 (0 = empty), the convention of
tests/island_witness.py; a grid smaller than the tree stands for a tree of its own size (the region is clipped to it).
steps() is a breadth-first search by frontier dilation: the frontier is a list of coordinates, every round its six face neighbours that
are inside the grid, passable and not yet reached take the round's number and become the next frontier. The cost of a round follows
the frontier, so a flood confined to a corner of a 256^3 tree costs what its reach costs."""
import numpy as np

EMPTY, SOLID, MATERIAL = 0, 1, 2
UNREACHED = 0xFFFF
MAX_STEPS = 65534
MAX_SEEDS = 65536
EXTENT = 256

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("medium", "<u4"), ("palette", "<i4"), ("max_steps", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3)])
RESULT_DTYPE = np.dtype([("reached", "<u4"), ("farthest", "<u4"), ("seeds_used", "<u4"), ("boundary", "<u4"), ("lo", "u1", 3), ("pad0", "u1"),
                         ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 2)])

# the order in which a path looks for its next voxel: -x, +x, -y, +y, -z, +z
NEIGHBOURS = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.int64)


def clip(region, shape):
    """(lo, hi) of the inclusive region clipped to a grid of `shape`, or None when it holds nothing; region None: the whole grid"""
    if region is None:
        return np.zeros(3, np.int64), np.array(shape, np.int64) - 1
    lo = np.asarray(region[0], np.int64)
    hi = np.minimum(np.asarray(region[1], np.int64), np.array(shape, np.int64) - 1)
    return None if np.any(lo > hi) else (lo, hi)


def passable(grid, medium=EMPTY, palette=0, region=None):
    grid = np.asarray(grid)
    ok = grid == 0 if medium == EMPTY else grid != 0 if medium == SOLID else grid == palette + 1
    assert medium in (EMPTY, SOLID, MATERIAL)
    box = clip(region, grid.shape)
    inside = np.zeros(grid.shape, bool)
    if box is not None:
        inside[tuple(slice(int(a), int(b) + 1) for a, b in zip(*box))] = True
    return ok & inside


def steps(grid, seeds, medium=EMPTY, palette=0, max_steps=MAX_STEPS, region=None):
    """uint16 array of the grid's shape: per voxel its step distance from the nearest seed, UNREACHED where there is none"""
    grid = np.asarray(grid)
    assert grid.ndim == 3 and max(grid.shape) <= EXTENT and 0 <= max_steps <= MAX_STEPS
    ok = passable(grid, medium, palette, region)
    out = np.full(grid.shape, UNREACHED, np.uint16)
    seeds = np.asarray(seeds, np.int64).reshape(-1, 3)
    assert len(seeds) <= MAX_SEEDS and np.all((seeds >= 0) & (seeds < EXTENT))
    seeds = seeds[np.all(seeds < np.array(grid.shape), axis=1)]
    frontier = np.unique(seeds[ok[seeds[:, 0], seeds[:, 1], seeds[:, 2]]], axis=0)
    out[frontier[:, 0], frontier[:, 1], frontier[:, 2]] = 0
    shape = np.array(grid.shape, np.int64)
    d = 0
    while len(frontier) and d < max_steps:
        d += 1
        n = (frontier[:, None, :] + NEIGHBOURS[None, :, :]).reshape(-1, 3)
        n = n[np.all((n >= 0) & (n < shape), axis=1)]
        n = n[ok[n[:, 0], n[:, 1], n[:, 2]] & (out[n[:, 0], n[:, 1], n[:, 2]] == UNREACHED)]
        key = np.unique((n[:, 0] << 16) | (n[:, 1] << 8) | n[:, 2])
        frontier = np.stack([key >> 16, (key >> 8) & 255, key & 255], axis=1)
        out[frontier[:, 0], frontier[:, 1], frontier[:, 2]] = d
    return out


def result(field, region=None):
    """the 32-byte result record of a field"""
    field = np.asarray(field, np.uint16)
    out = np.zeros((), RESULT_DTYPE)
    xyz = np.argwhere(field != UNREACHED)
    if not len(xyz):
        return out
    lo, hi = clip(region, field.shape)
    values = field[xyz[:, 0], xyz[:, 1], xyz[:, 2]]
    out["reached"] = len(xyz)
    out["farthest"] = values.max()
    out["seeds_used"] = np.count_nonzero(values == 0)
    out["boundary"] = np.count_nonzero(np.any((xyz == lo) | (xyz == hi), axis=1))
    out["lo"] = xyz.min(axis=0)
    out["hi"] = xyz.max(axis=0)
    return out


def at(field, xyz):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    return np.asarray(field, np.uint16)[xyz[:, 0], xyz[:, 1], xyz[:, 2]]


def paths(field, starts, capacity, keys=None):
    """(lengths, keys): per start the number of voxels of its path and the first `capacity` of them as x << 16 | y << 8 | z; the slots
    past a path's end keep what `keys` held (zero without one)"""
    field = np.asarray(field, np.uint16)
    starts = np.asarray(starts, np.int64).reshape(-1, 3)
    lengths = np.zeros(len(starts), np.uint32)
    keys = np.zeros((len(starts), capacity), np.uint32) if keys is None else np.array(keys, np.uint32).reshape(len(starts), capacity)
    for i, p in enumerate(starts):
        d = int(field[tuple(p)])
        if d == UNREACHED:
            continue
        lengths[i] = d + 1
        for k in range(min(d + 1, capacity)):
            keys[i, k] = (int(p[0]) << 16) | (int(p[1]) << 8) | int(p[2])
            if d == 0:
                break
            for off in NEIGHBOURS:
                q = p + off
                if np.all((q >= 0) & (q < field.shape)) and field[tuple(q)] == d - 1:
                    p, d = q, d - 1
                    break
            else:
                raise AssertionError("a reached voxel without a neighbour one step closer")
    return lengths, keys


def apply(grid, field, value, max_steps=None):
    """(grid afterwards, changed): every voxel with steps != UNREACHED and steps <= max_steps takes value (negative: None)"""
    grid = np.asarray(grid, np.uint8)
    field = np.asarray(field, np.uint16)
    hit = field != UNREACHED
    if max_steps is not None:
        hit &= field.astype(np.int64) <= max_steps
    byte = 0 if value < 0 else value + 1
    assert byte <= 255
    out = np.where(hit, byte, grid).astype(np.uint8)
    return out, int(np.count_nonzero(out != grid))


# ---------------------------------------------------------------- scenes the tests share
def to_xyzi(grid):
    """a grid's voxels as the .vox rows api.flatten_model takes: tree (x, y, z) is file (x, 255 - z, y) (loader.rs:248-253)"""
    xyz = np.argwhere(np.asarray(grid) != 0)
    pal = grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int64) - 1
    return np.stack([xyz[:, 0], 255 - xyz[:, 2], xyz[:, 1], pal], axis=1).astype(np.uint8)


def corridors():
    """(grid, empty corridors, solid corridors): a solid block with three one-voxel-wide empty corridors inside it, one along each axis,
    and three solid bars of the same shape in the air. Each runs from 10 to 40 on its axis (+100 for the bars): across brick boundaries
    and the root-cell boundaries at 16 and 32. A corridor is the list of its voxels from one end."""
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    grid[4:60, 4:60, 4:60] = 4
    fixed = ((21, 22), (45, 9), (50, 50))
    empty, solid = [], []
    for axis in range(3):
        run = np.zeros((31, 3), np.int64)
        run[:, axis] = np.arange(10, 41)
        run[:, [a for a in range(3) if a != axis]] = fixed[axis]
        empty.append(run)
        solid.append(run + 100)
        grid[run[:, 0], run[:, 1], run[:, 2]] = 0
        grid[run[:, 0] + 100, run[:, 1] + 100, run[:, 2] + 100] = 7 + axis
    return grid, empty, solid


def layer_snake():
    """ten cells of a 4 x 4 layer, from (0, 0) to (3, 0): two rows and what joins them, no two cells adjacent unless consecutive"""
    return [(0, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 3), (2, 2), (2, 1), (2, 0), (3, 0)]


def brick_snake(origin=(20, 36, 52)):
    """(grid, path): a snake of solid voxels inside ONE 4^3 brick in which only consecutive voxels share a face, so steps along it is the
    index. Every voxel of a full brick is within 9 steps of every other; the longest way through a brick needs walls of empty voxels,
    and this one has 22 voxels: a ten-cell layer, a joining voxel, the layer mirrored, a last voxel."""
    first = [(0, y, z) for y, z in layer_snake()]
    second = [(2, 3 - y, z) for y, z in layer_snake()]
    path = np.array(first + [(1, 3, 0)] + second + [(3, 0, 0)], np.int64) + np.array(origin)
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    grid[path[:, 0], path[:, 1], path[:, 2]] = 9
    return grid, path


def late_shortcut(origin=(32, 32, 32)):
    """(grid, seed, target, detour, shortcut): two ways of solid voxels from seed to target. The detour winds through four bricks in a
    row, ten voxels in each (40 voxels, 3 brick crossings); the shortcut leaves the layer, runs straight above it and comes back down
    (24 voxels, 5 brick crossings). A relaxation that advances a brick at a time reaches the target along the detour first."""
    detour = [(4 * b + x, y, 1) for b in range(4) for x, y in layer_snake()]
    shortcut = [(0, 0, z) for z in range(1, 6)] + [(x, 0, 5) for x in range(1, 16)] + [(15, 0, z) for z in range(4, 0, -1)]
    detour, shortcut = np.array(detour, np.int64) + np.array(origin), np.array(shortcut, np.int64) + np.array(origin)
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    for p in (detour, shortcut):
        grid[p[:, 0], p[:, 1], p[:, 2]] = 3
    return grid, detour[0], detour[-1], detour, shortcut


RANDOM_ORIGIN = (21, 38, 59)      # off the brick lattice on every axis
RANDOM_PALETTE = 1                # the palette index the MATERIAL flood of the random fill spreads through


def random_fill():
    """(grid, region, seeds per medium): a 64^3 block filled at 0.66, where the EMPTY voxels are just short of percolating freely, and
    three seeds among them; the materials are laid in columns and the seeds of the other two media drawn by a second generator. The region is the block."""
    rng = np.random.default_rng(71)
    solid = rng.random((64, 64, 64)) < 0.66
    empty = np.argwhere(~solid)
    seeds = rng.choice(empty, 3, replace=False)
    more = np.random.default_rng(72)
    x, y, _ = np.indices((64, 64, 64))
    material = (1 + (x // 6 + y // 5) % 3).astype(np.uint8)      # palette indices 0..2 in columns along z: a material's voxels hang together
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    o = RANDOM_ORIGIN
    grid[o[0]:o[0] + 64, o[1]:o[1] + 64, o[2]:o[2] + 64] = np.where(solid, material, 0)
    filled = np.argwhere(solid)
    solid_seeds = filled[more.choice(len(filled), 3, replace=False)]
    painted = np.argwhere(solid & (material == RANDOM_PALETTE + 1))
    material_seeds = painted[more.choice(len(painted), 3, replace=False)]
    region = (o, tuple(v + 63 for v in o))
    return grid, region, {EMPTY: seeds + o, SOLID: solid_seeds + o, MATERIAL: material_seeds + o}


def room(lo=(70, 70, 70), size=16):
    """(grid, inside voxel, region): a closed box of solid walls one voxel thick around size^3 voxels of air; the region is the box, walls
    included"""
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    a = np.array(lo)
    b = a + size + 2
    grid[a[0]:b[0], a[1]:b[1], a[2]:b[2]] = 6
    grid[a[0] + 1:b[0] - 1, a[1] + 1:b[1] - 1, a[2] + 1:b[2] - 1] = 0
    return grid, tuple(a + 1 + size // 2), (tuple(a), tuple(b - 1))


def crater():
    """(grid, seed, region): layered ground (y < 40) with a pit dug into it, a vein of material 9 through the ground and a patch of
    material 5 on the surface; water is poured in at the pit's bottom and may rise to y = 35"""
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    grid[8:72, 0:30, 8:72] = 2
    grid[8:72, 30:40, 8:72] = 3
    x, y, z = np.indices((64, 40, 64))
    pit = (x - 30) ** 2 + (z - 34) ** 2 + ((y - 40) * 2) ** 2 < 18 ** 2
    grid[8:72, 0:40, 8:72][pit] = 0
    grid[20:60, 12, 50] = 10                 # the vein: a bar ...
    grid[59, 12:25, 50] = 10                 # ... with a bend
    grid[12:20, 39, 12:18] = 6               # the patch
    grid[16:24, 39, 14:16] = 6
    return grid, (38, 32, 42), ((0, 0, 0), (255, 35, 255))
