"""The numpy witness of the model columns (dust_hip_model_columns, dust_hip_model_columns_apply; the contract is in
include/dust_hip.h). A helper module, not a test: tests/test_column_witness.py checks it against a plain per-voxel loop and two
identities, tests/test_column_rule.py holds the 256-bit column rule to it, tests/test_gpu_columns.py the device.

Written from the header text on whole arrays: the region's voxels are turned into [v][u][position along the walk, near end first]; the
columns that hold a counted voxel are gathered (the others have no run) and walked together: a run starts where a counted voxel follows
a not-counted one (or the near face); the running count of starts numbers every voxel's run, and a not-counted voxel carries the number
of the run whose gap it lies in. The grid holds palette index + 1 per voxel, 0 = None,
indexed [x, y, z]; it may be any box (the tree is 256^3)."""
import numpy as np

NEG_X, POS_X, NEG_Y, POS_Y, NEG_Z, POS_Z = 1, 2, 4, 8, 16, 32
FACES = (NEG_X, POS_X, NEG_Y, POS_Y, NEG_Z, POS_Z)
RUN, GAP = 0, 1
BINS = 256
NO_KEY = 0xFFFFFFFF
U_AXIS, V_AXIS = (2, 2, 1), (1, 0, 0)           # per axis of the walk: mesh's in-plane axes

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("face", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                        ("layer", "<u4"), ("reserved", "<u4")])
RESULT_DTYPE = np.dtype([("columns", "<u4"), ("hit", "<u4"), ("voxels", "<u4"), ("runs", "<u4"), ("depth_sum", "<u4"), ("nearest_key", "<u4"),
                         ("farthest_key", "<u4"), ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 7)])
CELL_DTYPE = np.dtype([("at", "u1"), ("palette", "u1"), ("length_minus_1", "u1"), ("runs", "u1")])


def refused(face, flags, palette, layer, reserved=0, where=RUN, depth=1, value=0):
    """what the calls refuse with DUST_ERR_INVALID_ARGUMENT (beyond null pointers, struct_size and a short capacity)"""
    return bool(face not in FACES or flags != 0 or reserved != 0 or palette < -1 or palette > 254 or layer > 255 or where > GAP or depth < 1
                or depth > 256 or value < -1 or value > 254)


def zero_result():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["lo"] = 255
    r["nearest_key"] = r["farthest_key"] = NO_KEY
    return r


def side(face):
    """(axis of the walk, whether it starts at the high end)"""
    d = FACES.index(face)
    return d >> 1, bool(d & 1)


def clip(grid, region):
    """the region's slices; None where lo > hi on an axis"""
    lo, hi = ((0, 0, 0), tuple(n - 1 for n in grid.shape)) if region is None else region
    hi = tuple(min(int(h), n - 1) for h, n in zip(hi, grid.shape))
    if any(int(l) > h for l, h in zip(lo, hi)):
        return None
    return tuple(slice(int(l), h + 1) for l, h in zip(lo, hi))


def turned(array, box, face):
    """the region of `array` as a VIEW indexed [v][u][position along the walk, the near end first]"""
    axis, from_high = side(face)
    view = np.transpose(array[box], (V_AXIS[axis], U_AXIS[axis], axis))
    return view[:, :, ::-1] if from_high else view


def walk(grid, face, palette, box, layer):
    """per column of the region, [v][u]: hit, the position of run `layer`'s first voxel, its length, its gap's length, the column's
    runs, the grid byte of the run's first voxel (0 for a miss). A column without a counted voxel has no run; the others are gathered
    into an (n, length) array and walked together."""
    axis, _ = side(face)
    counted_box = grid[box] != 0 if palette < 0 else grid[box] == palette + 1
    occupied = counted_box.any(axis=axis)                                  # [v][u]: v is the lower-numbered of the two axes that remain
    vs, us = np.nonzero(occupied)
    counted = turned(counted_box, (slice(None),) * 3, face)[vs, us]
    before = np.zeros_like(counted)
    before[:, 1:] = counted[:, :-1]
    starts = counted & ~before
    # a counted voxel: its run's number + 1; a not-counted one: the number of the run it lies in front of (at most 128: uint8 holds it)
    number = np.cumsum(starts, axis=1, dtype=np.uint8)
    first = starts & (number == layer + 1)
    has = first.any(axis=1)
    out = {name: np.zeros(occupied.shape, np.int64) for name in ("hit", "at", "length", "gap", "runs", "byte")}
    out["hit"][vs, us] = has
    out["at"][vs, us] = np.where(has, first.argmax(axis=1), 0)
    out["length"][vs, us] = np.where(has, (counted & (number == layer + 1)).sum(axis=1), 0)
    out["gap"][vs, us] = np.where(has, (~counted & (number == layer)).sum(axis=1), 0)
    out["runs"][vs, us] = starts.sum(axis=1)
    bytes_ = turned(grid, box, face)[vs, us]
    out["byte"][vs, us] = np.where(has, bytes_[np.arange(len(vs)), out["at"][vs, us]], 0)
    return out["hit"].astype(bool), out["at"], out["length"], out["gap"], out["runs"], out["byte"]


def columns(grid, face, palette=-1, region=None, layer=0):
    """(result, map, counts) of a call; the map (nv, nu), (0, 0) for the empty region"""
    assert not refused(face, 0, palette, layer)
    result, counts = zero_result(), np.zeros(BINS, np.uint32)
    box = clip(grid, region)
    if box is None:
        return result, np.zeros((0, 0), CELL_DTYPE), counts
    axis, from_high = side(face)
    hit, at, length, gap, runs, byte = walk(grid, face, palette, box, layer)
    nv, nu = hit.shape
    coord = np.where(hit, box[axis].stop - 1 - at if from_high else box[axis].start + at, 0)
    v, u = np.meshgrid(np.arange(nv) + box[V_AXIS[axis]].start, np.arange(nu) + box[U_AXIS[axis]].start, indexing="ij")
    xyz = [None] * 3
    xyz[axis], xyz[U_AXIS[axis]], xyz[V_AXIS[axis]] = coord, u, v
    palette_at = np.where(hit, byte - 1, 255)
    cells = np.zeros((nv, nu), CELL_DTYPE)
    cells["at"], cells["palette"], cells["length_minus_1"], cells["runs"] = coord, palette_at, np.where(hit, length - 1, 0), runs
    result["columns"], result["hit"], result["voxels"], result["runs"] = nv * nu, np.count_nonzero(hit), length.sum(), runs.sum()
    result["depth_sum"] = at[hit].sum()
    counts[:] = np.bincount(np.where(hit, palette_at + 1, 0).reshape(-1), minlength=BINS)
    if hit.any():
        x, y, z = (c[hit].astype(np.int64) for c in xyz)
        key, depth = (x << 16) | (y << 8) | z, at[hit].astype(np.int64)
        result["nearest_key"] = key[np.lexsort((key, depth))[0]]        # the smallest depth, among equals the lowest key
        result["farthest_key"] = key[np.lexsort((key, -depth))[0]]      # the largest depth, among equals the lowest key
        result["lo"], result["hi"] = (x.min(), y.min(), z.min()), (x.max(), y.max(), z.max())
    return result, cells, counts


def apply(grid, value, face, where=RUN, depth=1, palette=-1, region=None, layer=0):
    """(the grid after columns_apply, changed): decided on the grid as it is"""
    assert not refused(face, 0, palette, layer, 0, where, depth, value)
    out = grid.copy()
    box = clip(grid, region)
    if box is None:
        return out, 0
    hit, at, length, gap, _, _ = walk(grid, face, palette, box, layer)
    count = np.minimum(depth, gap if where == GAP else length)
    first = at - count if where == GAP else at
    target = turned(out, box, face)                                    # a view: writing it writes `out`
    vs, us = np.nonzero(hit)
    position = np.arange(target.shape[2])[None, :]
    spans = (position >= first[vs, us][:, None]) & (position < (first + count)[vs, us][:, None])
    target[vs, us] = np.where(spans, 0 if value < 0 else value + 1, target[vs, us])
    return out, int(np.count_nonzero(out != grid))
