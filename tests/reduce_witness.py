"""The numpy witness of the model reductions (dust_hip_model_reduce; the contract is in include/dust_hip.h). A helper module, not a
test file: written from the header text alone, it shares no code with the device path and works in the opposite direction -- the
kernel gathers eight children per coarse voxel, the witness folds the whole array.

Grids are uint8 [x, y, z] arrays holding palette index + 1 (0 = empty), the convention of tests/flood_witness.py. level() is the
header's one-level rule on an array of even sides: the array reshaped to (n, 2, n, 2, n, 2) and then to (n, n, n, 8), so that the
last axis holds a coarse voxel's eight children; per child the number of children equal to it, counted by all-pairs equality; the
winner picked by count * 256 + (255 - byte) among the solid children (the highest count, the lowest byte among equals); the coarse
voxel solid where at least min_solid children are. reduce() applies it level by level to a 256^3 grid and pads the result with zeros
to 256^3 again. A coarse voxel without a solid child is empty under every min_solid, so reduce() folds only the 32^3 tiles of the
tree that hold a voxel: the rule on each is the rule on the whole."""
import numpy as np

from flood_witness import to_xyzi  # noqa: F401  (a grid's .vox rows)

MAX_LEVELS = 8
EXTENT = 256
TILE = 32

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("levels", "<u4"), ("min_solid", "<u4"), ("flags", "<u4")])
RESULT_DTYPE = np.dtype([("src_voxels", "<u4"), ("voxels", "<u4"), ("extent", "<u4"), ("reserved", "<u4")])


def level(grid, min_solid):
    """one level: an array of sides (2a, 2b, 2c) -> (a, b, c)"""
    grid = np.asarray(grid, np.uint8)
    assert grid.ndim == 3 and all(n % 2 == 0 for n in grid.shape) and 1 <= min_solid <= 8
    a, b, c = (n // 2 for n in grid.shape)
    kids = grid.reshape(a, 2, b, 2, c, 2).transpose(0, 2, 4, 1, 3, 5).reshape(a, b, c, 8).astype(np.int32)
    same = (kids[..., :, None] == kids[..., None, :]).sum(axis=-1)
    key = np.where(kids != 0, same * 256 + (255 - kids), 0).max(axis=-1)
    solid = np.count_nonzero(kids, axis=-1)
    return np.where(solid >= min_solid, 255 - (key & 255), 0).astype(np.uint8)


def valid(levels, min_solid, flags=0):
    """the query validation table of the header"""
    return 1 <= levels <= MAX_LEVELS and 1 <= min_solid <= 8 and flags == 0


def reduce(grid, levels=1, min_solid=1):
    """a 256^3 grid -> the 256^3 grid of the new model: the reduction in [0, 256 >> levels)^3, zeros elsewhere"""
    grid = np.asarray(grid, np.uint8)
    assert grid.shape == (EXTENT,) * 3 and valid(levels, min_solid)
    side = EXTENT
    cur = grid
    for _ in range(levels):
        nxt = np.zeros((side // 2,) * 3, np.uint8)
        if side <= TILE:
            nxt[...] = level(cur, min_solid)
        else:
            t = side // TILE
            occupied = cur.reshape(t, TILE, t, TILE, t, TILE).any(axis=(1, 3, 5))
            for i, j, k in np.argwhere(occupied):
                src = cur[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE, k * TILE:(k + 1) * TILE]
                h = TILE // 2
                nxt[i * h:(i + 1) * h, j * h:(j + 1) * h, k * h:(k + 1) * h] = level(src, min_solid)
        cur, side = nxt, side // 2
    out = np.zeros((EXTENT,) * 3, np.uint8)
    out[:side, :side, :side] = cur
    return out


def result(grid, reduced, levels):
    """the call's result record"""
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["src_voxels"], r["voxels"], r["extent"] = np.count_nonzero(grid), np.count_nonzero(reduced), EXTENT >> levels
    return r
