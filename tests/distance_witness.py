"""The numpy witness of the model distances (dust_hip_model_distance / distance_at / distance_apply; the contract is in
include/dust_hip.h). A helper module, not a test file: written from the header text alone, it shares no code with the device path.

Grids are uint8 [x, y, z] arrays of up to 256 per axis holding palette index + 1 (0 = empty), the convention of
tests/flood_witness.py; a grid smaller than the tree stands for a tree of its own size (WALLS are its own faces).
field() is the definition, min over the targets t of the metric between v and t, evaluated one axis at a time on the whole array
(both metrics are separable: a minimum of sums of per-axis squares, or of maxima of per-axis offsets): along an axis
out[i] = min over j of combine(g[j], |i - j|), a min-plus (EUCLIDEAN) or min-max (CHEBYSHEV) over shifts. The shifts that matter are
few, and which ones depends on the input: where only a few slabs along the axis hold anything finite (the targets' bounding box), j
runs over those slabs and every i takes the shift i - j; where nearly every line is full of small values, the shifts k = 1, 2, ... are
applied to the whole array until k (k^2) is no smaller than any value of a line that holds something. Nothing is capped before the
end: values above the limit become FAR once, as the header states it. No offset beyond max_radius is ever looked at: it could only
give a value above the limit."""
import numpy as np

from flood_witness import crater, to_xyzi  # noqa: F401  (the apply tests' scene, and a grid's .vox rows)

TO_SOLID, TO_EMPTY, TO_MATERIAL = 0, 1, 2
EUCLIDEAN, CHEBYSHEV = 0, 1
WALLS = 1
FAR = 0xFFFF
MAX_RADIUS = 255
NO_KEY = 0xFFFFFFFF
EXTENT = 256
NONE = np.uint32(1 << 24)      # no target seen yet: above every value (3 * 255^2)

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("target", "<u4"), ("metric", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("max_radius", "<u4"),
                        ("reserved", "<u4", 2)])
RESULT_DTYPE = np.dtype([("targets", "<u4"), ("near", "<u4"), ("far", "<u4"), ("largest", "<u4"), ("largest_key", "<u4"), ("reserved", "<u4", 3)])


def targets(grid, target=TO_SOLID, palette=0):
    grid = np.asarray(grid)
    assert target in (TO_SOLID, TO_EMPTY, TO_MATERIAL)
    return grid != 0 if target == TO_SOLID else grid == 0 if target == TO_EMPTY else grid == palette + 1


def limit_of(metric, max_radius):
    assert metric in (EUCLIDEAN, CHEBYSHEV) and 1 <= max_radius <= MAX_RADIUS
    return max_radius * max_radius if metric == EUCLIDEAN else max_radius


def _cost(offset, metric):
    return (offset * offset if metric == EUCLIDEAN else offset).astype(np.uint32)


def _along(g, metric, max_radius):
    """one axis (the last one of g): out[..., i] = min over |i - j| <= max_radius of combine(g[..., j], |i - j|), with
    combine(g, d) = g + d^2 or max(g, d). Values at or above NONE stand for "no target": they stay there (NONE + NONE fits a uint32)."""
    n = g.shape[-1]
    has = g < NONE
    lines = has.any(axis=-1)
    if not lines.any():
        return g
    sub = g[lines]                                              # the lines that hold something, one per row; the others stay as they are
    slabs = np.flatnonzero(has[lines].any(axis=0))
    out = sub.copy()
    if len(slabs) <= 64 or len(slabs) * len(sub) <= 40 * 65536:    # few source slabs: every output takes each of them at its own shift
        tmp = np.empty_like(sub)
        for j in slabs:
            lo, hi = max(0, j - max_radius), min(n, j + max_radius + 1)
            cost = _cost(np.abs(np.arange(lo, hi, dtype=np.int64) - j), metric)
            (np.add if metric == EUCLIDEAN else np.maximum)(sub[:, j:j + 1], cost, out=tmp[:, lo:hi])
            np.minimum(out[:, lo:hi], tmp[:, lo:hi], out=out[:, lo:hi])
    else:                                                       # many: shift the lines outward until none can gain
        for k in range(1, min(max_radius, n - 1) + 1):
            cost = np.uint32(k * k if metric == EUCLIDEAN else k)
            if not (out > cost).any():
                break
            combine = (lambda a: a + cost) if metric == EUCLIDEAN else (lambda a: np.maximum(a, cost))
            np.minimum(out[:, k:], combine(sub[:, :-k]), out=out[:, k:])
            np.minimum(out[:, :-k], combine(sub[:, k:]), out=out[:, :-k])
    g = g.copy()
    g[lines] = out
    return g


def wall_distance(shape):
    """w of the header: per voxel, min over the axes of min(c + 1, extent - c)"""
    w = None
    for axis, n in enumerate(shape):
        c = np.arange(n, dtype=np.int64)
        d = np.minimum(c + 1, n - c).reshape([-1 if a == axis else 1 for a in range(3)])
        w = d if w is None else np.minimum(w, d)
    return np.broadcast_to(w, shape)


def field(grid, target=TO_SOLID, metric=EUCLIDEAN, max_radius=MAX_RADIUS, walls=False, palette=0):
    """uint16 array of the grid's shape: per voxel the distance to the nearest target, FAR above the limit"""
    grid = np.asarray(grid)
    assert grid.ndim == 3 and max(grid.shape) <= EXTENT
    limit = limit_of(metric, max_radius)
    g = np.where(targets(grid, target, palette), np.uint32(0), NONE)
    for axis in range(3):
        g = np.moveaxis(_along(np.ascontiguousarray(np.moveaxis(g, axis, -1)), metric, max_radius), -1, axis)
    if walls:
        w = wall_distance(grid.shape)
        g = np.minimum(g, (w * w if metric == EUCLIDEAN else w).astype(np.uint32))
    return np.where(g <= limit, g, FAR).astype(np.uint16)


def result(values):
    """the 32-byte result record of a field"""
    values = np.asarray(values, np.uint16)
    out = np.zeros((), RESULT_DTYPE)
    out["targets"] = np.count_nonzero(values == 0)
    out["far"] = np.count_nonzero(values == FAR)
    out["near"] = values.size - int(out["targets"]) - int(out["far"])
    out["largest_key"] = NO_KEY
    if int(out["targets"]) + int(out["near"]):
        largest = values[values != FAR].max()
        x, y, z = np.argwhere(values == largest)[0]             # (in x, y, z order: the lowest key first)
        out["largest"] = largest
        out["largest_key"] = (int(x) << 16) | (int(y) << 8) | int(z)
    return out


def at(values, xyz):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    return np.asarray(values, np.uint16)[xyz[:, 0], xyz[:, 1], xyz[:, 2]]


def apply(grid, values, value, lo=1, hi=0xFFFFFFFF):
    """(grid afterwards, changed): every voxel with value != FAR and lo <= value <= hi takes `value` (negative: None)"""
    grid = np.asarray(grid, np.uint8)
    values = np.asarray(values, np.uint16).astype(np.int64)
    hit = (values != FAR) & (values >= lo) & (values <= hi)
    byte = 0 if value < 0 else value + 1
    assert byte <= 255
    out = np.where(hit, byte, grid).astype(np.uint8)
    return out, int(np.count_nonzero(out != grid))


# ---------------------------------------------------------------- scenes the tests share
def key(x, y, z):
    return int(x) << 16 | int(y) << 8 | int(z)


def single_voxel():
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    grid[0, 0, 0] = 3
    return grid


SEAMS = (15, 16, 63, 64, 255)        # either side of a brick boundary that is a root-cell boundary, of one that is not, and the tree's edge
SEAM_LINES = ((0, (37, 90)), (1, (200, 41)), (2, (123, 170)))      # (axis, the two fixed coordinates in x, y, z order)


def seam_line(axis, fixed, positions=None):
    """the coordinates of a line along `axis` (all 256 positions, or the given ones)"""
    p = np.arange(EXTENT) if positions is None else np.asarray(positions)
    xyz = np.zeros((len(p), 3), np.int64)
    xyz[:, axis] = p
    xyz[:, [a for a in range(3) if a != axis]] = fixed
    return xyz


def seams():
    """targets at 15, 16, 63, 64 and 255 of one line along each axis: brick, root-cell and tree-edge seams in every pass"""
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    for axis, fixed in SEAM_LINES:
        xyz = seam_line(axis, fixed, SEAMS)
        grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]] = 5 + axis
    return grid


RANDOM_ORIGIN = (8, 8, 8)            # the 40^3 box straddles the root cells' boundaries at 16 and 32
RANDOM_SIZE = 40
RANDOM_PALETTES = (2, 11, 200)
RANDOM_PALETTE = 11                  # the one TO_MATERIAL measures to


def random_fill():
    """(grid, box): a 2 % fill of a 40^3 box, palettes drawn from three indices; box = the box grown by 6, inclusive"""
    rng = np.random.default_rng(91)
    n = RANDOM_SIZE
    solid = rng.random((n, n, n)) < 0.02
    palette = np.array(RANDOM_PALETTES)[rng.integers(0, 3, (n, n, n))]
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    o = RANDOM_ORIGIN
    grid[o[0]:o[0] + n, o[1]:o[1] + n, o[2]:o[2] + n] = np.where(solid, palette + 1, 0)
    return grid, (tuple(v - 6 for v in o), tuple(v + n + 5 for v in o))


def staircase():
    """solid voxels (i, i, 0) for i < 64 and one far voxel: most lines see many different nearest targets"""
    grid = np.zeros((EXTENT,) * 3, np.uint8)
    i = np.arange(64)
    grid[i, i, 0] = 4
    grid[200, 30, 90] = 4
    return grid


def box_coordinates(box):
    lo, hi = box
    return np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)
