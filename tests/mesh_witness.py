"""The numpy witness of the model meshes (dust_hip_model_mesh; the contract is in include/dust_hip.h). A helper module, not a test:
tests/test_mesh_witness.py holds it to a brute-force reading of the rule, tests/test_mesh_rule.py the row functions of
dust_amd/csrc/mesh_rule.hpp to it, tests/test_gpu_mesh.py the device.

Written from the header text on whole arrays. Exposure, the region and the refusals are surface_witness's. Per direction the faces
are sorted by (slice, v, u); a run starts at a face that does not follow a face of the same byte in its row and ends before the next
start; a run is named by (slice, u0, u1, byte), and runs of one name in consecutive rows are one quad. Only the solid voxels are
handled one by one; exposure is worked out on their bounding box plus one voxel, which is all that can hold a face. The grid holds
palette index + 1 per voxel, 0 = None, indexed [x, y, z]; it may be any box (the tree is 256^3)."""
import numpy as np

import surface_witness as S

WALLS = 1
ANY_PALETTE = 2
FACES_ALL = S.FACES_ALL
# per normal axis n: the grid's axes in the order (n, v, u) -- u the higher-numbered remaining axis, v the other one
AXES = ((0, 1, 2), (1, 0, 2), (2, 0, 1))

QUERY_DTYPE = S.QUERY_DTYPE
RESULT_DTYPE = np.dtype([("quads", "<u4"), ("faces", "<u4"), ("quads_by_face", "<u4", 6), ("faces_by_face", "<u4", 6), ("largest", "<u4"), ("reserved", "<u4")])
QUAD_DTYPE = np.dtype([("key", "<u4"), ("face", "u1"), ("palette", "u1"), ("du", "u1"), ("dv", "u1")])


def refused(faces, flags, palette, lo, hi):
    """what the call refuses with DUST_ERR_INVALID_ARGUMENT (beyond null pointers and struct_size)"""
    return bool(flags & ~(WALLS | ANY_PALETTE)) or S.refused(faces, flags & WALLS, palette, lo, hi)


def zero_result():
    return np.zeros(1, RESULT_DTYPE)[0]


def face_set(grid, faces=FACES_ALL, palette=-1, region=None, walls=False, exposed=None):
    """(xyz, shown): the voxels with a face in some F_d, in no particular order, and per voxel the byte of those faces. `exposed`:
    surface_witness.exposure(grid, walls), if the caller has it already; otherwise it is worked out on the bounding box of the solid
    voxels plus one voxel, which is all that can hold a face."""
    box = S.clip(grid, region)
    solid = np.argwhere(grid != 0)
    if box is None or len(solid) == 0:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.uint8)
    if exposed is None:
        lo = np.maximum(solid.min(axis=0) - 1, 0)
        hi = np.minimum(solid.max(axis=0) + 1, np.array(grid.shape) - 1)
        # (a solid voxel on the crop's border is on the tree's border: the padding is the walls')
        faces_of = S.exposure(grid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1], walls)[tuple((solid - lo).T)]
    else:
        faces_of = exposed[tuple(solid.T)]
    byte = grid[tuple(solid.T)]
    keep = np.ones(len(solid), bool) if palette < 0 else byte == palette + 1
    for axis, cut in enumerate(box):
        keep &= (solid[:, axis] >= cut.start) & (solid[:, axis] < cut.stop)
    shown = np.where(keep, faces_of & np.uint8(faces), 0).astype(np.uint8)
    return solid[shown != 0].astype(np.int64), shown[shown != 0]


def mesh(grid, faces=FACES_ALL, palette=-1, region=None, walls=False, any_palette=False, exposed=None):
    """(result, quads) of a call with room for every quad"""
    assert not refused(faces, 0, palette, (0, 0, 0), (0, 0, 0))
    result = zero_result()
    all_xyz, shown = face_set(grid, faces, palette, region, walls, exposed)
    parts = []
    for d in range(6):
        xyz = all_xyz[(shown >> d) & 1 == 1]
        if len(xyz) == 0:
            continue
        n_axis, v_axis, u_axis = AXES[d >> 1]
        s, v, u = xyz[:, n_axis], xyz[:, v_axis], xyz[:, u_axis]
        order = np.lexsort((u, v, s))                                            # row by row, along u
        s, v, u = s[order], v[order], u[order]
        byte = grid[tuple(xyz[order].T)].astype(np.int64)
        name = np.ones_like(byte) if any_palette else byte                      # what has to agree for two faces to merge
        joined = np.zeros(len(s), bool)                                          # ... with the face before it in the row
        joined[1:] = (s[1:] == s[:-1]) & (v[1:] == v[:-1]) & (u[1:] == u[:-1] + 1) & (name[1:] == name[:-1])
        starts = np.flatnonzero(~joined)
        ends = np.append(starts[1:], len(s)) - 1                                # a run ends where the next one starts
        s, v, u0, u1, b, pal = s[starts], v[starts], u[starts], u[ends], name[starts], byte[starts] - 1
        # runs of one name (slice, u0, u1, byte), by row: a row that does not follow its predecessor begins a quad
        order = np.lexsort((v, b, u1, u0, s))
        s, v, u0, u1, b, pal = s[order], v[order], u0[order], u1[order], b[order], pal[order]
        same = np.zeros(len(s), bool)
        same[1:] = (s[1:] == s[:-1]) & (u0[1:] == u0[:-1]) & (u1[1:] == u1[:-1]) & (b[1:] == b[:-1]) & (v[1:] == v[:-1] + 1)
        first = np.flatnonzero(~same)
        height = np.diff(np.append(first, len(s)))
        s, v0, u0, u1, pal = s[first], v[first], u0[first], u1[first], pal[first]
        order = np.lexsort((u0, v0, s))                                          # the documented order: slice, v0, u0
        s, v0, u0, u1, pal, height = s[order], v0[order], u0[order], u1[order], pal[order], height[order]
        quads = np.zeros(len(s), QUAD_DTYPE)
        corner = np.zeros((len(s), 3), np.int64)
        corner[:, n_axis], corner[:, v_axis], corner[:, u_axis] = s, v0, u0
        quads["key"] = (corner[:, 0] << 16) | (corner[:, 1] << 8) | corner[:, 2]
        quads["face"] = d
        quads["palette"] = pal                                                   # (under any_palette: that of the key voxel)
        quads["du"] = u1 - u0
        quads["dv"] = height - 1
        area = (u1 - u0 + 1) * height
        result["quads_by_face"][d] = len(s)
        result["faces_by_face"][d] = area.sum()
        result["largest"] = max(int(result["largest"]), int(area.max()))
        parts.append(quads)
    result["quads"] = result["quads_by_face"].sum()
    result["faces"] = result["faces_by_face"].sum()
    return result, np.concatenate(parts) if parts else np.zeros(0, QUAD_DTYPE)


def rasterise(quads, shape):
    """per voxel the byte of its faces the quads cover, and whether any face was covered twice"""
    out = np.zeros(shape, np.uint8)
    twice = False
    for q in quads:
        key, d = int(q["key"]), int(q["face"])
        lo = [key >> 16, (key >> 8) & 255, key & 255]
        ext = [1, 1, 1]
        n, v_axis, u_axis = AXES[d >> 1]
        ext[u_axis], ext[v_axis] = int(q["du"]) + 1, int(q["dv"]) + 1
        part = out[lo[0]:lo[0] + ext[0], lo[1]:lo[1] + ext[1], lo[2]:lo[2] + ext[2]]
        assert part.shape == tuple(ext), "a quad reaches past the tree"
        twice |= bool((part & (1 << d)).any())
        part |= np.uint8(1 << d)
    return out, twice
