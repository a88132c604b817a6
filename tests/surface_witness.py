"""The numpy witness of the model surfaces (dust_hip_model_surface, dust_hip_model_surface_apply; the contract is in
include/dust_hip.h). A helper module, not a test: tests/test_surface_witness.py checks it on hand-counted cases and against a per-voxel
loop, tests/test_surface_rule.py holds the brick-word rule to it, tests/test_gpu_surface.py the device.

Written from the header text on whole arrays: the solid voxels are padded by one voxel all round (empty, or solid under WALLS), a
face of direction d is exposed where the voxel is solid and the padded array moved one voxel against d is not; a voxel is listed when
it is solid, inside the clipped region, passes the palette filter and has an exposed face among the query's; the list is sorted by the
voxel's place in the model's block order, written out here from its definition. The grid holds palette index + 1 per voxel, 0 = None,
indexed [x, y, z]; it may be any box (the tree is 256^3)."""
import numpy as np

NEG_X, POS_X, NEG_Y, POS_Y, NEG_Z, POS_Z = 1, 2, 4, 8, 16, 32
FACES_ALL = 63
WALLS = 1
BINS = 256
STEPS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))      # bit d of a faces byte looks this way

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("faces", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                        ("reserved", "<u4", 2)])
RESULT_DTYPE = np.dtype([("voxels", "<u4"), ("faces", "<u4"), ("by_face", "<u4", 6), ("solid", "<u4"), ("lo", "u1", 3), ("pad0", "u1"),
                         ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 5)])
VOXEL_DTYPE = np.dtype([("key", "<u4"), ("faces", "u1"), ("palette", "u1"), ("reserved", "<u2")])


def refused(faces, flags, palette, lo, hi, value=0):
    """what the calls refuse with DUST_ERR_INVALID_ARGUMENT (beyond null pointers and struct_size)"""
    return bool(faces == 0 or faces > FACES_ALL or (flags & ~WALLS) or palette < -1 or palette > 254 or max(*lo, *hi) >= 256 or value > 254)


def zero_result():
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["lo"] = 255
    return r


def exposure(grid, walls=False):
    """per voxel the byte of its exposed faces (0 for an empty voxel)"""
    solid = grid != 0
    padded = np.pad(solid, 1, constant_values=bool(walls))
    nx, ny, nz = grid.shape
    out = np.zeros(grid.shape, np.uint8)
    for d, (sx, sy, sz) in enumerate(STEPS):
        across = padded[1 + sx:1 + sx + nx, 1 + sy:1 + sy + ny, 1 + sz:1 + sz + nz]
        out |= (solid & ~across).astype(np.uint8) << np.uint8(d)
    return out


def block_order(x, y, z):
    """a voxel's place in the model's block order: the 16^3 root cell (x slowest), the 4^3 brick inside it, the voxel inside that"""
    x, y, z = (np.asarray(v, np.int64) for v in (x, y, z))
    cell = ((x // 16) * 16 + (y // 16)) * 16 + (z // 16)
    brick = ((x // 4 % 4) * 4 + (y // 4 % 4)) * 4 + (z // 4 % 4)
    voxel = ((x % 4) * 4 + (y % 4)) * 4 + (z % 4)
    return (cell * 64 + brick) * 64 + voxel


def clip(grid, region):
    """the region's slices; None where lo > hi on an axis"""
    lo, hi = ((0, 0, 0), tuple(n - 1 for n in grid.shape)) if region is None else region
    if any(int(l) > int(h) for l, h in zip(lo, hi)):
        return None
    return tuple(slice(int(l), min(int(h), n - 1) + 1) for l, h, n in zip(lo, hi, grid.shape))


def surface(grid, faces=FACES_ALL, palette=-1, region=None, walls=False, exposed=None):
    """(result, voxels, counts) of a call with room for every voxel; `exposed`: exposure(grid, walls), if the caller has it already"""
    assert not refused(faces, 0, palette, (0, 0, 0), (0, 0, 0))
    result, counts = zero_result(), np.zeros((6, BINS), np.uint32)
    box = clip(grid, region)
    if box is None:
        return result, np.zeros(0, VOXEL_DTYPE), counts
    exposed = exposure(grid, walls) if exposed is None else exposed
    inside = grid[box]                                   # only the region's voxels are looked at; `exposed` saw their neighbours outside it
    looked_at = inside != 0 if palette < 0 else inside == palette + 1
    shown = np.where(looked_at, exposed[box] & np.uint8(faces), 0).astype(np.uint8)
    xyz = np.argwhere(shown != 0) + np.array([s.start for s in box])
    xyz = xyz[np.argsort(block_order(xyz[:, 0], xyz[:, 1], xyz[:, 2]), kind="stable")]
    voxels = np.zeros(len(xyz), VOXEL_DTYPE)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    voxels["key"] = (x << 16) | (y << 8) | z
    voxels["faces"] = exposed[x, y, z] & np.uint8(faces)
    voxels["palette"] = grid[x, y, z] - 1
    result["voxels"] = len(xyz)
    result["solid"] = np.count_nonzero(looked_at)
    for d in range(6):
        has = (voxels["faces"] >> d) & 1 == 1
        result["by_face"][d] = np.count_nonzero(has)
        counts[d] = np.bincount(voxels["palette"][has].astype(np.int64) + 1, minlength=BINS)
    result["faces"] = result["by_face"].sum()
    if len(xyz):
        result["lo"], result["hi"] = xyz.min(axis=0), xyz.max(axis=0)
    return result, voxels, counts


def apply(grid, value, faces=FACES_ALL, palette=-1, region=None, walls=False):
    """(the grid after surface_apply, changed): every listed voxel takes `value` (negative: None), decided on the grid as it is"""
    _, voxels, _ = surface(grid, faces, palette, region, walls)
    out = grid.copy()
    key = voxels["key"].astype(np.int64)
    out[key >> 16, (key >> 8) & 255, key & 255] = 0 if value < 0 else value + 1
    return out, int(np.count_nonzero(out != grid))
