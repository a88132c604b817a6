"""Thin Python handles over the C ABI (include/dust_hip.h) for tests and bench.py.

Names follow the reference's surface: Tree (crates/vdb/src/tree.rs), VoxLoader/VoxGeometry
(crates/vox/src/{loader,geometry}.rs), StandardPipeline/GBuffer/PinholeProjection/Sunlight
(crates/render/src/pipeline/standard.rs, projection.rs, pipeline/sky.rs). The C++ mirror of the same
surface, which is what a Rust maintainer would read, is include/dust_hip.hpp.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L

BLOCK_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("w", "<u2"), ("mask", "<u8"),
                        ("material_ptr", "<u4"), ("avg_albedo", "<u4")])
assert BLOCK_DTYPE.itemsize == 24
SURFEL_DTYPE = np.dtype([("pos", "<f4", 3), ("direction", "<u4")])
# scene ray queries (Scene.trace_rays): DustHipRay / DustHipRayHit
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direction", "<f4", 3), ("tmax", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("instance", "<u4"), ("block", "<u4"), ("voxel", "<u4"), ("xyz", "<u4", 3),
                      ("face", "u1"), ("palette", "u1"), ("reserved", "<u2")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 32
# scene box queries (Scene.overlap_boxes): DustHipBoxQuery / DustHipVoxelRef
BOX_QUERY_DTYPE = np.dtype([("lo", "<f4", 3), ("first", "<u4"), ("hi", "<f4", 3), ("capacity", "<u4")])
VOXEL_REF_DTYPE = np.dtype([("instance", "<u4"), ("block", "<u4"), ("xyz", "<u2", 3), ("palette", "u1"), ("voxel", "u1")])
assert BOX_QUERY_DTYPE.itemsize == 32 and VOXEL_REF_DTYPE.itemsize == 16
# scene box sweeps (Scene.sweep_boxes): DustHipBoxSweep / DustHipSweepHit
BOX_SWEEP_DTYPE = np.dtype([("lo", "<f4", 3), ("reserved0", "<u4"), ("hi", "<f4", 3), ("reserved1", "<u4"), ("delta", "<f4", 3),
                            ("reserved2", "<u4")])
SWEEP_HIT_DTYPE = np.dtype([("t", "<f4"), ("instance", "<u4"), ("block", "<u4"), ("xyz", "<u2", 3), ("palette", "u1"), ("voxel", "u1"),
                            ("normal", "<f4", 3)])
assert BOX_SWEEP_DTYPE.itemsize == 48 and SWEEP_HIT_DTYPE.itemsize == 32
# dust_hip_model_edit_shapes: a shape in a model's tree coordinates and its operation
EDIT_SHAPE_DTYPE = np.dtype([("a", "<f4", 3), ("kind", "<u4"), ("b", "<f4", 3), ("radius", "<f4"), ("op", "<u4"), ("palette", "<i4"),
                             ("reserved", "<u4", 2)])
# DustHipIsland, 40 bytes: one island of dust_hip_model_find_islands
STAMP_DTYPE = np.dtype([("offset", "<i4", 3), ("orient", "<u4"), ("op", "<u4"), ("src_lo", "u1", 3), ("pad0", "u1"), ("src_hi", "u1", 3), ("pad1", "u1"),
                        ("reserved", "<u4")])   # DustHipStamp
ORIENT_IDENTITY = 0x24   # p = (0, 1, 2), no flips
# DustHipResample, 96 bytes, and DustHipResampleCount, 16 bytes: a record of dust_hip_model_resample and its counts
RESAMPLE_DTYPE = np.dtype([("m", "<i4", (3, 3)), ("t", "<i4", 3), ("dst_lo", "<i4", 3), ("dst_hi", "<i4", 3), ("src_lo", "u1", 3), ("pad0", "u1"),
                           ("src_hi", "u1", 3), ("pad1", "u1"), ("op", "<u4"), ("reserved", "<u4", 3)])
RESAMPLE_COUNT_DTYPE = np.dtype([("changed", "<u4"), ("covered", "<u4"), ("solid", "<u4"), ("blocked", "<u4")])
# DustHipCast, 48 bytes, and DustHipCastHit, 32 bytes: a cast of dust_hip_model_cast and its answer
CAST_DTYPE = np.dtype([("offset", "<i4", 3), ("orient", "<u4"), ("step", "<i4", 3), ("max_steps", "<u4"), ("flags", "<u4"), ("src_lo", "u1", 3),
                       ("pad0", "u1"), ("src_hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4")])
CAST_HIT_DTYPE = np.dtype([("steps", "<u4"), ("flags", "<u4"), ("contacts", "<u4"), ("voxels", "<u4"), ("contact", "<i4", 3), ("src_key", "<u4")])
# DustHipFloodResult, 32 bytes: what a dust_hip_model_flood reached
FLOOD_RESULT_DTYPE = np.dtype([("reached", "<u4"), ("farthest", "<u4"), ("seeds_used", "<u4"), ("boundary", "<u4"), ("lo", "u1", 3), ("pad0", "u1"),
                               ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 2)])
# DustHipDistanceResult, 32 bytes: the counts of a dust_hip_model_distance field and where its largest value is
DISTANCE_RESULT_DTYPE = np.dtype([("targets", "<u4"), ("near", "<u4"), ("far", "<u4"), ("largest", "<u4"), ("largest_key", "<u4"), ("reserved", "<u4", 3)])
# DustHipReduceResult, 16 bytes: the voxel counts of a dust_hip_model_reduce and the extent of the new model
REDUCE_RESULT_DTYPE = np.dtype([("src_voxels", "<u4"), ("voxels", "<u4"), ("extent", "<u4"), ("reserved", "<u4")])
# DustHipCensus, 40 bytes: one shape's record of dust_hip_model_census
CENSUS_DTYPE = np.dtype([("covered", "<u4"), ("solid", "<u4"), ("lo", "u1", 3), ("reserved0", "u1"), ("hi", "u1", 3), ("reserved1", "u1"), ("sum", "<u8", 3)])
# DustHipSurfaceResult (64 bytes) and DustHipSurfaceVoxel (8 bytes): the result and the list entries of dust_hip_model_surface
SURFACE_RESULT_DTYPE = np.dtype([("voxels", "<u4"), ("faces", "<u4"), ("by_face", "<u4", 6), ("solid", "<u4"), ("lo", "u1", 3), ("pad0", "u1"),
                                 ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 5)])
SURFACE_VOXEL_DTYPE = np.dtype([("key", "<u4"), ("faces", "u1"), ("palette", "u1"), ("reserved", "<u2")])
# DustHipMeshResult (64 bytes) and DustHipMeshQuad (8 bytes): the result and the list entries of dust_hip_model_mesh
MESH_RESULT_DTYPE = np.dtype([("quads", "<u4"), ("faces", "<u4"), ("quads_by_face", "<u4", 6), ("faces_by_face", "<u4", 6), ("largest", "<u4"), ("reserved", "<u4")])
MESH_QUAD_DTYPE = np.dtype([("key", "<u4"), ("face", "u1"), ("palette", "u1"), ("du", "u1"), ("dv", "u1")])
# DustHipBoxesResult (64 bytes) and DustHipBox (8 bytes): the result and the list entries of dust_hip_model_boxes
BOXES_RESULT_DTYPE = np.dtype([("boxes", "<u4"), ("rects", "<u4"), ("voxels", "<u4"), ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"),
                               ("reserved", "<u4", 11)])
BOX_DTYPE = np.dtype([("key", "<u4"), ("palette", "u1"), ("dx", "u1"), ("dy", "u1"), ("dz", "u1")])
# DustHipDeltaResult (64 bytes) and DustHipDeltaVoxel (8 bytes): the result and the list entries of dust_hip_model_delta, and the
# records dust_hip_model_delta_apply takes
DELTA_RESULT_DTYPE = np.dtype([("voxels", "<u4"), ("added", "<u4"), ("removed", "<u4"), ("repainted", "<u4"), ("solid_before", "<u4"), ("solid_after", "<u4"),
                               ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 8)])
DELTA_VOXEL_DTYPE = np.dtype([("key", "<u4"), ("kind", "u1"), ("before", "u1"), ("after", "u1"), ("reserved", "u1")])
# DustHipColumnsResult (64 bytes) and DustHipColumnCell (4 bytes): the result and the map entries of dust_hip_model_columns
COLUMNS_RESULT_DTYPE = np.dtype([("columns", "<u4"), ("hit", "<u4"), ("voxels", "<u4"), ("runs", "<u4"), ("depth_sum", "<u4"), ("nearest_key", "<u4"),
                                 ("farthest_key", "<u4"), ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 7)])
COLUMN_CELL_DTYPE = np.dtype([("at", "u1"), ("palette", "u1"), ("length_minus_1", "u1"), ("runs", "u1")])
# DustHipNeighboursQuery (48 bytes), DustHipNeighboursResult and DustHipNeighboursApplied (64 bytes each): the query of
# dust_hip_model_neighbours and _neighbours_apply and what each of them returns
NEIGHBOURS_QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("neighbourhood", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                                   ("birth", "<u4"), ("survive", "<u4")])
NEIGHBOURS_RESULT_DTYPE = np.dtype([("voxels", "<u4"), ("solid", "<u4"), ("born", "<u4"), ("died", "<u4"), ("lo", "u1", 3), ("pad0", "u1"),
                                    ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 10)])
NEIGHBOURS_APPLIED_DTYPE = np.dtype([("generations", "<u4"), ("solid_before", "<u4"), ("solid_after", "<u4"), ("reserved0", "<u4"), ("born", "<u8"), ("died", "<u8"),
                                     ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 6)])
# DustHipSettleQuery (72 bytes), DustHipSettleResult and DustHipSettleApplied (64 bytes each): the query of dust_hip_model_settle and
# _settle_apply and what each of them returns
SETTLE_QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("toward", "<u4"), ("flags", "<u4"), ("reserved", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3), ("loose", "<u4", 8)])
SETTLE_RESULT_DTYPE = np.dtype([("columns", "<u4"), ("loose", "<u4"), ("fixed", "<u4"), ("moved", "<u4"), ("changed", "<u4"), ("fall_max", "<u4"), ("fall_sum", "<u8"),
                                ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("changed_columns", "<u4"), ("reserved", "<u4", 5)])
SETTLE_APPLIED_DTYPE = np.dtype([("generations", "<u4"), ("first_moved", "<u4"), ("loose", "<u4"), ("reserved0", "<u4"), ("slid", "<u8"), ("fell", "<u8"),
                                 ("fall_sum", "<u8"), ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 4)])
# DustHipTriangle / DustHipFillMeshResult (model voxelisation): integer vertices in 1/256 voxel
TRIANGLE_DTYPE = np.dtype([("v", "<i4", (3, 3)), ("op", "<u4"), ("palette", "<i4"), ("reserved", "<u4")])
FILL_MESH_RESULT_DTYPE = np.dtype([("covered", "<u4"), ("changed", "<u4"), ("live", "<u4"), ("crossing", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                                   ("reserved", "<u4", 2)])
# DustHipFractureSeed / DustHipFractureResult / DustHipFractureCell (model fracture)
FRACTURE_SEED_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("reserved", "<u4")])
FRACTURE_RESULT_DTYPE = np.dtype([("solid", "<u4"), ("labelled", "<u4"), ("cells", "<u4"), ("largest_cell", "<u4"), ("largest_voxels", "<u4"), ("cut_faces", "<u4"),
                                  ("max_d2", "<u4"), ("lo", "u1", 3), ("reserved0", "u1"), ("hi", "u1", 3), ("reserved1", "u1"), ("reserved", "<u4", 7)])
FRACTURE_CELL_DTYPE = np.dtype([("voxels", "<u4"), ("cut_faces", "<u4"), ("lo", "u1", 3), ("reserved0", "u1"), ("hi", "u1", 3), ("reserved1", "u1"), ("sum", "<u8", 3)])
# DustHipMidNode and DustHipL2Cell, 16 bytes each: the records of dust_hip_model_read_hierarchy
MID_NODE_DTYPE = np.dtype([("mask_lo", "<u4"), ("mask_hi", "<u4"), ("first_block", "<u4"), ("pad", "<u4")])
L2_CELL_DTYPE = np.dtype([("mid", "<u4"), ("bounds", "<u4"), ("child_mask", "<u8")])
# DustHipBody (96 bytes): one group of dust_hip_model_bodies -- key, counted voxels, bounds, mass, first and second moments
BODY_DTYPE = np.dtype([("key", "<u4"), ("voxels", "<u4"), ("lo", "u1", 3), ("reserved0", "u1"), ("hi", "u1", 3), ("reserved1", "u1"), ("mass", "<u8"),
                       ("m1", "<u8", 3), ("m2", "<u8", 6)])
# DustHipJoint (80 bytes): one pair of groups of dust_hip_model_joints -- the keys, the shared faces, by direction, bounds and sums of the face centres
JOINT_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("faces", "<u4"), ("reserved0", "<u4"), ("by_face", "<u4", 6), ("lo2", "<u2", 3), ("hi2", "<u2", 3),
                        ("reserved1", "<u4"), ("sum2", "<u8", 3)])
ISLAND_DTYPE = np.dtype([("key", "<u4"), ("voxels", "<u4"), ("lo", "u1", 3), ("flags", "u1"), ("hi", "u1", 3), ("reserved", "u1"), ("sum", "<u8", 3)])
FLT_MAX = float(np.finfo(np.float32).max)


def count_mask(*ranges):
    """The bit mask over neighbour counts that Model.neighbours and Model.neighbours_apply take as `birth` and `survive`: each argument a
    count or an inclusive (first, last) pair -- count_mask((14, 26)) is bits 14..26, count_mask(5, 6) bits 5 and 6, count_mask() 0."""
    mask = 0
    for r in ranges:
        first, last = (r, r) if isinstance(r, (int, np.integer)) else r
        for n in range(int(first), int(last) + 1):
            mask |= 1 << n
    return mask


def loose_mask(indices=None):
    """The eight words Model.settle and Model.settle_apply take as `loose`: bit p set for every palette index p named -- each item an
    index 0..254 or an inclusive (first, last) pair. None: all 255 indices, everything is loose."""
    bits = (1 << 255) - 1 if indices is None else 0
    for r in () if indices is None else indices:
        first, last = (r, r) if isinstance(r, (int, np.integer)) else r
        for p in range(int(first), int(last) + 1):
            bits |= 1 << p
    return tuple((bits >> (32 * w)) & 0xFFFFFFFF for w in range(8))


PLANE_DTYPES = {
    L.PLANE_ILLUMINANCE: (np.uint16, 4), L.PLANE_DENOISED: (np.uint16, 4), L.PLANE_ALBEDO: (np.uint32, 1),
    L.PLANE_NORMAL: (np.uint32, 1), L.PLANE_DEPTH: (np.float32, 1), L.PLANE_MOTION: (np.uint16, 4),
    L.PLANE_VOXEL_ID: (np.uint32, 1), L.PLANE_ACCUM: (np.float32, 4), L.PLANE_OUTPUT: (np.uint16, 4),
}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Tree:
    """dust_vdb::Tree<hierarchy!(...)> (crates/vdb/src/tree.rs:7-124)."""

    def __init__(self, *fanout_log2):
        self._lib = L.load()
        arr = (C.c_uint32 * len(fanout_log2))(*fanout_log2)
        self._h = C.c_void_p()
        L.check(self._lib.dust_vdb_tree_create(arr, len(fanout_log2), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_vdb_tree_destroy(self._h)
            self._h = None

    def set_value(self, xyz, value):
        v = -1 if value is None else (1 if value else 0)
        L.check(self._lib.dust_vdb_tree_set(self._h, int(xyz[0]), int(xyz[1]), int(xyz[2]), v))

    def get_value(self, xyz):
        out = C.c_int32()
        L.check(self._lib.dust_vdb_tree_get(self._h, int(xyz[0]), int(xyz[1]), int(xyz[2]), C.byref(out)))
        return None if out.value < 0 else bool(out.value)

    def iter(self):
        n = C.c_size_t()
        L.check(self._lib.dust_vdb_tree_iter(self._h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.uint32)
        L.check(self._lib.dust_vdb_tree_iter(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)))
        return out[: n.value]

    def iter_leaf(self):
        n = C.c_size_t()
        L.check(self._lib.dust_vdb_tree_iter_leaf(self._h, None, None, None, 0, C.byref(n)))
        k = max(n.value, 1)
        xyz = np.zeros((k, 3), np.uint32)
        occ = np.zeros(k, np.uint64)
        mat = np.zeros(k, np.uint32)
        L.check(self._lib.dust_vdb_tree_iter_leaf(self._h, xyz.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  occ.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  mat.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)))
        return xyz[: n.value], occ[: n.value], mat[: n.value]

    def meta(self):
        mask, lvl = C.c_uint32(), C.c_uint32()
        L.check(self._lib.dust_vdb_tree_meta(self._h, C.byref(mask), C.byref(lvl)))
        return mask.value, lvl.value

    def accessor(self):
        return Accessor(self)


class Accessor:
    """dust_vdb::Accessor (crates/vdb/src/accessor.rs:5-57)."""

    def __init__(self, tree):
        self._tree = tree
        self._lib = tree._lib
        self._h = C.c_void_p()
        L.check(self._lib.dust_vdb_accessor_create(tree._h, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_vdb_accessor_destroy(self._h)
            self._h = None

    def get(self, xyz):
        out = C.c_int32()
        L.check(self._lib.dust_vdb_accessor_get(self._h, int(xyz[0]), int(xyz[1]), int(xyz[2]), C.byref(out)))
        return None if out.value < 0 else bool(out.value)


def lca_level(a, b, mask, root_level):
    lib = L.load()
    aa = (C.c_uint32 * 3)(*[int(v) for v in a])
    bb = (C.c_uint32 * 3)(*[int(v) for v in b])
    return lib.dust_vdb_lca_level(aa, bb, mask, root_level)


def flatten_model(xyzi, size, palette256):
    """load_model + VoxGeometry::from_tree (loader.rs:238-308, geometry.rs:55-179) -> (blocks, materials)."""
    lib = L.load()
    xyzi = np.ascontiguousarray(xyzi, np.uint8).reshape(-1, 4)
    pal = np.ascontiguousarray(palette256, np.uint8).reshape(256, 4)
    sz = (C.c_uint32 * 3)(*[int(v) for v in size])
    blocks = C.POINTER(L.Block)()
    mats = C.POINTER(C.c_uint8)()
    nb, nm = C.c_uint32(), C.c_uint64()
    L.check(lib.dust_vox_flatten_model(_ptr(xyzi), xyzi.shape[0], sz, _ptr(pal), C.byref(blocks), C.byref(nb),
                                       C.byref(mats), C.byref(nm)))
    try:
        b = np.frombuffer(C.string_at(blocks, nb.value * 24), BLOCK_DTYPE).copy()
        m = np.frombuffer(C.string_at(mats, nm.value), np.uint8).copy()
    finally:
        lib.dust_vox_free(blocks)
        lib.dust_vox_free(mats)
    return b, m


class VoxScene:
    """What VoxLoader::load yields before upload (loader.rs:322-415): models, palette, instances."""

    def __init__(self, data: bytes, frame: int = 0):
        self._lib = L.load()
        self._h = C.c_void_p()
        buf = np.frombuffer(data, np.uint8)
        if frame:  # animation frame: multi-frame nTRN / multi-model nSHP nodes (loader.rs:103-105,149-151 are unimplemented!())
            L.check(self._lib.dust_vox_load_frame(_ptr(buf), buf.size, int(frame), C.byref(self._h)))
        else:
            L.check(self._lib.dust_vox_load(_ptr(buf), buf.size, C.byref(self._h)))
        nm, ni = C.c_uint32(), C.c_uint32()
        L.check(self._lib.dust_vox_scene_counts(self._h, C.byref(nm), C.byref(ni)))
        self.n_models, self.n_instances = nm.value, ni.value
        pal = C.POINTER(C.c_uint8)()
        L.check(self._lib.dust_vox_scene_palette(self._h, C.byref(pal)))
        self.palette = np.frombuffer(C.string_at(pal, 1024), np.uint8).reshape(256, 4).copy()
        inst = (L.VoxInstance * max(ni.value, 1))()
        L.check(self._lib.dust_vox_scene_instances(self._h, inst, ni.value))
        self.instances = [(inst[i].model, np.array(inst[i].obj_to_world, np.float32)) for i in range(ni.value)]

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_vox_scene_destroy(self._h)
            self._h = None

    def model_info(self, i):
        info = L.VoxModelInfo()
        L.check(self._lib.dust_vox_scene_model_info(self._h, i, C.byref(info)))
        return info

    def model_data(self, i):
        info = self.model_info(i)
        blocks = C.POINTER(L.Block)()
        mats = C.POINTER(C.c_uint8)()
        L.check(self._lib.dust_vox_scene_model_data(self._h, i, C.byref(blocks), C.byref(mats)))
        b = np.frombuffer(C.string_at(blocks, info.n_blocks * 24), BLOCK_DTYPE).copy() if info.n_blocks else np.zeros(0, BLOCK_DTYPE)
        m = np.frombuffer(C.string_at(mats, info.n_materials), np.uint8).copy() if info.n_materials else np.zeros(0, np.uint8)
        return b, m


class PinholeProjection:
    """crates/render/src/projection.rs:3-29"""

    def __init__(self, fov=math.pi / 4, near=0.1, far=10000.0):
        self.fov, self.near, self.far = fov, near, far


def look_at_rotation(eye, target, up=(0.0, 1.0, 0.0)):
    """Rotation of a camera looking from eye to target (columns = camera x, y, z axes; -z is forward),
    as Transform::looking_at builds it for the FPS camera of examples/castle.rs:120-129."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    up2 = np.cross(back, right)
    return np.stack([right, up2, back], axis=1).astype(np.float32)  # columns


def make_camera(eye, rotation_cols, projection: PinholeProjection):
    """CameraSettings members the shaders read (standard.rs:277-302)."""
    cam = L.Camera()
    r = np.asarray(rotation_cols, np.float32)
    cam.view_col0[:] = r[:, 0].tolist()
    cam.view_col1[:] = r[:, 1].tolist()
    cam.view_col2[:] = r[:, 2].tolist()
    cam.position[:] = [float(np.float32(v)) for v in eye]
    cam.tan_half_fov = float(np.float32(np.tan(np.float32(projection.fov) / np.float32(2.0))))
    cam.far_ = projection.far
    cam.near_ = projection.near
    return cam


# ColorSpacePrimaries (rhyolite/src/utils/format.rs:573-641): r, g, b, white point chromaticities
BT709 = ((0.64, 0.33), (0.3, 0.6), (0.15, 0.06), (0.3127, 0.3290))
ACES_AP1 = ((0.713, 0.293), (0.165, 0.830), (0.128, 0.044), (0.32168, 0.33767))
DCI_P3 = ((0.68, 0.32), (0.265, 0.69), (0.15, 0.06), (0.3127, 0.3290))


def primaries_to_xyz(p):
    """ColorSpacePrimaries::to_xyz (format.rs:651-664)."""
    x = np.array([p[0][0], p[1][0], p[2][0], p[3][0]], np.float64)
    y = np.array([p[0][1], p[1][1], p[2][1], p[3][1]], np.float64)
    X, Z = x / y, (1.0 - x - y) / y
    mat = np.stack([X[:3], np.ones(3), Z[:3]])          # rows X, Y, Z; columns r, g, b
    s = np.linalg.solve(mat, np.array([X[3], 1.0, Z[3]]))
    return mat * s[None, :]


def color_space_conversion(src=ACES_AP1, dst=BT709):
    """ColorSpacePrimaries::to_color_space (format.rs:666-679), no chromatic adaptation; returned column-major
    as the nine COLOR_SPACE_CONVERSION_* specialization constants of tone_map.comp."""
    m = np.linalg.inv(primaries_to_xyz(dst)) @ primaries_to_xyz(src)
    return m.T.reshape(9).astype(np.float32)


class SkyDataset:
    """The Hosek-Wilkie tables Sunlight::bake reads (sky.rs:25-64), handed over as the bytes of the reference's
    dataset.bin and datasetSolar.bin."""

    def __init__(self, dataset_bin: bytes, dataset_solar_bin: bytes):
        self._lib = L.load()
        self._h = C.c_void_p()
        a, b = np.frombuffer(dataset_bin, np.uint8), np.frombuffer(dataset_solar_bin, np.uint8)
        L.check(self._lib.dust_sky_dataset_create(_ptr(a), a.size, _ptr(b), b.size, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_sky_dataset_destroy(self._h)
            self._h = None


class Sunlight:
    """dust_render::Sunlight (crates/render/src/pipeline/sky.rs:6-23): turbidity, ground albedo, direction eye -> sun."""

    def __init__(self, turbidity=1.0, albedo=(0.2, 0.2, 0.2), direction=(0.0, 0.80114365, -0.5984721)):
        self.turbidity, self.albedo, self.direction = float(turbidity), tuple(albedo), tuple(direction)

    def bake(self, dataset: SkyDataset):
        """Sunlight::bake (sky.rs:90-132) -> the 56 floats of SkyModelState."""
        out = L.Sky()
        alb = (C.c_float * 3)(*self.albedo)
        d = (C.c_float * 3)(*self.direction)
        L.check(dataset._lib.dust_sky_bake(dataset._h, self.turbidity, alb, d, C.byref(out)))
        return np.array(out.state, np.float32)


class Context:
    def __init__(self, device=-1, timing=True, stream=None, lds_root_bytes=0, sparse_timing=False):
        self._lib = L.load()
        flags = (L.CONTEXT_TIMING if timing else 0) | (L.CONTEXT_TIMING_SPARSE if timing and sparse_timing else 0)
        cfg = L.Config(C.sizeof(L.Config), device, stream, lds_root_bytes, flags)
        self._h = C.c_void_p()
        L.check(self._lib.dust_hip_context_create(C.byref(cfg), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_hip_context_destroy(self._h)
            self._h = None

    def sync(self):
        L.check(self._lib.dust_hip_sync(self._h))

    def device_eval(self, fn, rows, out_words):
        """dust_hip_device_eval: rows is an (n, in_words) array of 32-bit words (float32 or uint32); returns (n, out_words) uint32.
        The functions and their rows are tabulated in include/dust_hip.h: 0..2 the brick walks, 3..11 the codecs, 12..14 the sorters, 15 sky and
        16 sun radiance of a direction (the 56 floats of the sky state in rows 0..18, three to a row; those rows come back zero), 17 the albedo
        modulation, 18 the spatial hash's fingerprint and location, 19 its insert on a three-entry probe window."""
        rows = np.ascontiguousarray(rows)
        assert rows.dtype.itemsize == 4 and rows.ndim == 2
        out = np.zeros((rows.shape[0], out_words), np.uint32)
        L.check(self._lib.dust_hip_device_eval(self._h, fn, _ptr(rows), rows.shape[1], _ptr(out), out_words, rows.shape[0]))
        return out


class Model:
    """VoxGeometry + PaletteMaterial on the device."""

    def __init__(self, ctx, blocks, materials, palette, tree_extent_log2=8):
        self._ctx = ctx
        self._lib = ctx._lib
        blocks = np.ascontiguousarray(blocks, BLOCK_DTYPE)
        materials = np.ascontiguousarray(materials, np.uint8)
        pal = np.ascontiguousarray(np.asarray(palette, np.uint8).reshape(-1, 4)[:255])
        self._h = C.c_void_p()
        L.check(self._lib.dust_hip_model_create(ctx._h, _ptr(blocks), blocks.size, _ptr(materials), materials.size,
                                                _ptr(pal), tree_extent_log2, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_hip_model_destroy(self._h)
            self._h = None

    def set_voxels(self, xyz, values):
        """VoxGeometry::set on the device copy: xyz (n, 3) tree coordinates, values (n,) palette index or -1 to clear.
        Scenes instancing the model must be committed again afterwards."""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        values = np.ascontiguousarray(values, np.int32).reshape(-1)
        assert len(values) == len(xyz)
        L.check(self._lib.dust_hip_model_set_voxels(self._h, _ptr(xyz), _ptr(values), len(values)))

    def get_voxels(self, xyz):
        """VoxGeometry::get: palette index per coordinate, -1 where the voxel is empty"""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        out = np.zeros(len(xyz), np.int32)
        L.check(self._lib.dust_hip_model_get_voxels(self._h, _ptr(xyz), _ptr(out), len(out)))
        return out

    def edit_shapes(self, shapes):
        """Carve / fill / paint / place boxes, spheres and capsules (dust_hip_model_edit_shapes): `shapes` an EDIT_SHAPE_DTYPE array
        (see edit_shapes()), in the model's tree coordinates; a shape covers the voxels whose centre (x + 0.5, y + 0.5, z + 0.5) it
        contains, and the shapes apply in order. Returns `changed`: per shape, the voxels whose value it changed. Scenes instancing
        the model must be committed again afterwards."""
        shapes = np.ascontiguousarray(shapes, EDIT_SHAPE_DTYPE).reshape(-1)
        changed = np.zeros(len(shapes), np.uint32)
        L.check(self._lib.dust_hip_model_edit_shapes(self._h, _ptr(shapes), len(shapes), _ptr(changed)))
        return changed

    def census(self, shapes, tables=True):
        """What the voxels inside shapes hold (dust_hip_model_census): `shapes` an EDIT_SHAPE_DTYPE array as Model.edit_shapes takes
        it (op and palette are ignored), each counted on its own against the model as it stands; nothing changes. Returns (records,
        counts): records a CENSUS_DTYPE array (covered, solid, the bounds lo / hi and the coordinate sums of the solid covered voxels),
        counts (n, 256) uint32 with counts[i, 0] the covered voxels that hold None and counts[i, 1 + p] those that hold palette index p
        -- or None with tables=False (then up to L.MAX_CENSUS_SHAPES shapes instead of L.MAX_CENSUS_TABLES)."""
        shapes = np.ascontiguousarray(shapes, EDIT_SHAPE_DTYPE).reshape(-1)
        records = np.zeros(len(shapes), CENSUS_DTYPE)
        counts = np.zeros((len(shapes), L.CENSUS_BINS), np.uint32) if tables else None
        L.check(self._lib.dust_hip_model_census(self._h, _ptr(shapes), len(shapes), _ptr(records), _ptr(counts) if tables else None))
        return records, counts

    def _surface_query(self, faces, palette, region, walls):
        q = L.SurfaceQuery(struct_size=C.sizeof(L.SurfaceQuery), faces=faces, flags=L.SURFACE_WALLS if walls else 0, palette=palette)
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        return q

    def surface(self, faces=L.FACES_ALL, palette=-1, region=None, walls=False, capacity=None, tables=False):
        """The exposed faces of the model's solid voxels (dust_hip_model_surface): a face is exposed when the voxel across it is empty
        (across a face of the tree: empty, or solid with walls=True). `faces` the L.FACE_* directions that count, `palette` -1 for every
        solid voxel or the one palette index that counts, region = (lo, hi) an inclusive voxel box (None: the whole tree; neighbours
        outside it are consulted as they are). Returns (result, voxels, counts): result a SURFACE_RESULT_DTYPE record (voxels, faces,
        by_face, solid, lo, hi); voxels a SURFACE_VOXEL_DTYPE array (key x << 16 | y << 8 | z, faces, palette) of the first
        min(result.voxels, capacity) listed voxels in the order of Model.read()'s blocks, then ascending voxel bit -- capacity=None makes
        two calls, one to count and one to list everything; counts (6, 256) uint32 with counts[d, 1 + p] the exposed faces of direction
        d on listed voxels of palette index p, or None with tables=False. The model is only read."""
        q = self._surface_query(faces, palette, region, walls)
        out = np.zeros(1, SURFACE_RESULT_DTYPE)
        counts = np.zeros((6, L.SURFACE_BINS), np.uint32) if tables else None
        if capacity is None:
            L.check(self._lib.dust_hip_model_surface(self._h, C.byref(q), _ptr(out), None, 0, None))
            capacity = int(out[0]["voxels"])
        voxels = np.zeros(int(capacity), SURFACE_VOXEL_DTYPE)
        L.check(self._lib.dust_hip_model_surface(self._h, C.byref(q), _ptr(out), _ptr(voxels) if capacity else None, int(capacity),
                                                 _ptr(counts) if tables else None))
        return out[0], voxels[: min(int(capacity), int(out[0]["voxels"]))], counts

    def surface_apply(self, value, faces=L.FACES_ALL, palette=-1, region=None, walls=False):
        """Every voxel Model.surface would list under the same query takes `value`, a palette index or -1 for None
        (dust_hip_model_surface_apply); what is listed is decided on the model as it stood when the call began, so -1 peels exactly one
        layer. Returns the number of voxels that changed. Scenes instancing the model must be committed again; both fields and the
        island labelling are invalid afterwards."""
        q = self._surface_query(faces, palette, region, walls)
        changed = C.c_uint32()
        L.check(self._lib.dust_hip_model_surface_apply(self._h, C.byref(q), int(value), C.byref(changed)))
        return changed.value

    def mesh(self, faces=L.FACES_ALL, palette=-1, region=None, walls=False, any_palette=False, capacity=None):
        """The exposed faces of the model's solid voxels merged into axis-aligned rectangles (dust_hip_model_mesh). `faces`, `palette`,
        `region` and `walls` select the faces exactly as in Model.surface. Per direction and slice of its normal axis a run is a maximal
        stretch of faces of one palette index along u (z for the x and y directions, y for the z directions), and a quad a maximal
        stack of identical runs along v (y for the x directions, x otherwise); any_palette=True merges across palette indices. This is
        a canonical partition, not the minimum-count greedy mesh. Returns (result, quads): result a MESH_RESULT_DTYPE record (quads,
        faces, quads_by_face, faces_by_face, largest); quads a MESH_QUAD_DTYPE array (key x << 16 | y << 8 | z of the lowest corner
        voxel, face 0..5, palette, du and dv the extents minus 1) of the first min(result.quads, capacity) quads in ascending (face,
        slice, v0, u0) -- capacity=None makes two calls, one to count and one to list everything. mesh_corners turns the records into
        corner positions. The model is only read."""
        q = L.MeshQuery(struct_size=C.sizeof(L.MeshQuery), faces=faces, palette=palette,
                        flags=(L.MESH_WALLS if walls else 0) | (L.MESH_ANY_PALETTE if any_palette else 0))
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        out = np.zeros(1, MESH_RESULT_DTYPE)
        if capacity is None:
            L.check(self._lib.dust_hip_model_mesh(self._h, C.byref(q), _ptr(out), None, 0))
            capacity = int(out[0]["quads"])
        quads = np.zeros(int(capacity), MESH_QUAD_DTYPE)
        L.check(self._lib.dust_hip_model_mesh(self._h, C.byref(q), _ptr(out), _ptr(quads) if capacity else None, int(capacity)))
        return out[0], quads[: min(int(capacity), int(out[0]["quads"]))]

    def boxes(self, axis=0, palette=-1, region=None, any_palette=False, capacity=None):
        """The model's solid voxels merged into axis-aligned boxes (dust_hip_model_boxes): the convex pieces of a compound collider, an
        exact snapshot, a replayable description. `palette` and `region` select the voxels as in Model.surface (nothing outside the
        region exists for the call). Per slice of `axis` (0 x, 1 y, 2 z) a run is a maximal stretch of voxels of one palette index
        along u, a rect a maximal stack of identical runs along v (Model.mesh's axes), and a box a maximal stack of identical rects
        along `axis`; any_palette=True merges across palette indices. A canonical partition, not the minimum-count decomposition.
        Returns (result, boxes): result a BOXES_RESULT_DTYPE record (boxes, rects, voxels, lo, hi); boxes a BOX_DTYPE array (key
        x << 16 | y << 8 | z of the lowest corner voxel, palette, dx, dy, dz the extents minus 1) of the first min(result.boxes,
        capacity) boxes in ascending (slice, v0, u0) -- capacity=None makes two calls, one to count and one to list everything.
        box_shapes turns the records into Model.edit_shapes records, box_bounds into inclusive bounds. The model is only read."""
        q = L.BoxesQuery(struct_size=C.sizeof(L.BoxesQuery), axis=int(axis), palette=palette, flags=L.BOXES_ANY_PALETTE if any_palette else 0)
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        out = np.zeros(1, BOXES_RESULT_DTYPE)
        if capacity is None:
            L.check(self._lib.dust_hip_model_boxes(self._h, C.byref(q), _ptr(out), None, 0))
            capacity = int(out[0]["boxes"])
        boxes = np.zeros(int(capacity), BOX_DTYPE)
        L.check(self._lib.dust_hip_model_boxes(self._h, C.byref(q), _ptr(out), _ptr(boxes) if capacity else None, int(capacity)))
        return out[0], boxes[: min(int(capacity), int(out[0]["boxes"]))]

    def delta(self, after, kinds=L.DELTA_ALL, palette=-1, region=None, capacity=None, tables=False):
        """The voxels in which `after` differs from this model at the same tree coordinates (dust_hip_model_delta). `kinds` the
        L.DELTA_ADDED / DELTA_REMOVED / DELTA_REPAINTED changes that count, `palette` -1 for every change or the one palette index a
        voxel's value before or after must be, region = (lo, hi) an inclusive voxel box (None: the whole tree). Returns (result, voxels,
        counts): result a DELTA_RESULT_DTYPE record (voxels, added, removed, repainted, solid_before, solid_after, lo, hi); voxels a
        DELTA_VOXEL_DTYPE array (key x << 16 | y << 8 | z, kind, before, after -- palette indices, L.DELTA_NONE for no voxel) of the
        first min(result.voxels, capacity) listed voxels in the order of Model.read()'s blocks, then ascending voxel bit --
        capacity=None makes two calls, one to count and one to list everything; counts (2, 256) uint32 with counts[0, b] the listed
        voxels whose value before has bin b and counts[1, b] the same for the value after (bin 0 None, bin 1 + p palette index p), or
        None with tables=False. Both models are only read; the same model twice gives the zero result."""
        q = L.DeltaQuery(struct_size=C.sizeof(L.DeltaQuery), kinds=kinds, flags=0, palette=palette)
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        out = np.zeros(1, DELTA_RESULT_DTYPE)
        counts = np.zeros((2, L.DELTA_BINS), np.uint32) if tables else None
        if capacity is None:
            L.check(self._lib.dust_hip_model_delta(self._h, after._h, C.byref(q), _ptr(out), None, 0, None))
            capacity = int(out[0]["voxels"])
        voxels = np.zeros(int(capacity), DELTA_VOXEL_DTYPE)
        L.check(self._lib.dust_hip_model_delta(self._h, after._h, C.byref(q), _ptr(out), _ptr(voxels) if capacity else None, int(capacity),
                                               _ptr(counts) if tables else None))
        return out[0], voxels[: min(int(capacity), int(out[0]["voxels"]))], counts

    def delta_apply(self, records, backward=False):
        """Play a DELTA_VOXEL_DTYPE list onto the model (dust_hip_model_delta_apply): every record's voxel takes `after` and is expected
        to hold `before`, or the other way round with backward=True; a key named more than once keeps its last record. Returns
        (changed, conflicts): the voxels whose value differs afterwards, and the records whose voxel did not hold the expected value
        when the call began (they are applied all the same). Scenes instancing the model must be committed again; both fields and the
        island labelling are invalid afterwards."""
        records = np.ascontiguousarray(records, DELTA_VOXEL_DTYPE)
        changed, conflicts = C.c_uint32(), C.c_uint32()
        L.check(self._lib.dust_hip_model_delta_apply(self._h, _ptr(records) if len(records) else None, len(records),
                                                     L.DELTA_BACKWARD if backward else 0, C.byref(changed), C.byref(conflicts)))
        return changed.value, conflicts.value

    def _columns_query(self, face, palette, region, layer):
        q = L.ColumnsQuery(struct_size=C.sizeof(L.ColumnsQuery), face=face, flags=0, palette=palette, layer=layer)
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        return q

    @staticmethod
    def columns_shape(face, region=None):
        """(nv, nu) of the map Model.columns returns for `face` and `region`: the clipped region's extent along v and along u (u = z
        and v = y for the x sides, u = z and v = x for the y sides, u = y and v = x for the z sides); (0, 0) for an empty region"""
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        extent = [min(int(h), 255) - int(l) + 1 for l, h in zip(lo, hi)]
        if min(extent) <= 0:
            return 0, 0
        axis = {L.FACE_NEG_X: 0, L.FACE_POS_X: 0, L.FACE_NEG_Y: 1, L.FACE_POS_Y: 1, L.FACE_NEG_Z: 2, L.FACE_POS_Z: 2}[face]
        return extent[1 if axis == 0 else 0], extent[1 if axis == 2 else 2]

    def columns(self, face, palette=-1, region=None, layer=0, cells=True, tables=False):
        """The model seen from one side, column by column (dust_hip_model_columns). `face` the one L.FACE_* side the columns are
        looked at from (L.FACE_POS_Y: from above, walking down), `palette` -1 for every solid voxel or the one palette index that counts
        (everything else is see-through), region = (lo, hi) an inclusive voxel box outside which nothing exists for the call (None: the
        whole tree), `layer` the run of every column that is asked for, 0 the nearest. Returns (result, map, counts): result a
        COLUMNS_RESULT_DTYPE record (columns, hit, voxels, runs, depth_sum, nearest_key, farthest_key, lo, hi); map a (nv, nu)
        COLUMN_CELL_DTYPE array (at, palette -- 255 for a miss --, length_minus_1, runs), or None with cells=False; counts (256,) uint32
        with counts[0] the missed columns and counts[1 + p] the hit columns whose nearest voxel has palette index p, or None with
        tables=False. The model is only read."""
        q = self._columns_query(face, palette, region, layer)
        out = np.zeros(1, COLUMNS_RESULT_DTYPE)
        counts = np.zeros(L.COLUMNS_BINS, np.uint32) if tables else None
        grid = np.zeros(self.columns_shape(face, region), COLUMN_CELL_DTYPE) if cells else None
        L.check(self._lib.dust_hip_model_columns(self._h, C.byref(q), _ptr(out), _ptr(grid) if cells and grid.size else None,
                                                 grid.size if cells else 0, _ptr(counts) if tables else None))
        return out[0], grid, counts

    def columns_apply(self, value, face, where=L.COLUMNS_RUN, depth=1, palette=-1, region=None, layer=0):
        """In every column Model.columns would report a hit for under the same query, the nearest min(depth, length) voxels of the run
        (where=L.COLUMNS_RUN) or the min(depth, gap) voxels of the gap directly in front of it (L.COLUMNS_GAP) take `value`, a palette
        index or -1 for None (dust_hip_model_columns_apply); decided on the model as it stood when the call began. Returns the number
        of voxels that changed. Scenes instancing the model must be committed again; both fields and the island labelling are invalid
        afterwards."""
        q = self._columns_query(face, palette, region, layer)
        changed = C.c_uint32()
        L.check(self._lib.dust_hip_model_columns_apply(self._h, C.byref(q), int(where), int(depth), int(value), C.byref(changed)))
        return changed.value

    def edit_triangles(self, triangles, count=True):
        """Carve / fill / paint / place the voxels triangles touch (dust_hip_model_edit_triangles): `triangles` a TRIANGLE_DTYPE array
        (see triangles()), integer vertices in 1/256 voxel of the model's tree coordinates; a triangle covers every voxel whose closed
        cube it shares a point with (exact: a 13-axis separating-axis test on integers), and the triangles apply in order. Returns
        `changed`: per triangle, the voxels whose value it changed (None with count=False). Scenes instancing the model must be
        committed again afterwards."""
        triangles = np.ascontiguousarray(triangles, TRIANGLE_DTYPE).reshape(-1)
        changed = np.zeros(len(triangles), np.uint32) if count else None
        L.check(self._lib.dust_hip_model_edit_triangles(self._h, _ptr(triangles), len(triangles), _ptr(changed) if count else None))
        return changed

    def fill_mesh(self, triangles, op=L.EDIT_FILL, palette=0, region=None):
        """The voxels whose centres lie inside a closed triangle mesh take `op` / `palette` (dust_hip_model_fill_mesh): `triangles` a
        TRIANGLE_DTYPE array (their own op and palette are ignored), region = (lo, hi) an inclusive voxel box (None: the whole tree).
        Inside is the parity of the triangles crossed above the centre along +z, exact on integers; winding and order do not matter.
        Returns a FILL_MESH_RESULT_DTYPE record (covered, changed, live, crossing, lo, hi). Scenes instancing the model must be
        committed again afterwards."""
        triangles = np.ascontiguousarray(triangles, TRIANGLE_DTYPE).reshape(-1)
        q = L.FillMeshQuery(struct_size=C.sizeof(L.FillMeshQuery), op=int(op), palette=int(palette), flags=0)
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        out = np.zeros(1, FILL_MESH_RESULT_DTYPE)
        L.check(self._lib.dust_hip_model_fill_mesh(self._h, _ptr(triangles), len(triangles), C.byref(q), _ptr(out)))
        return out[0]

    def _neighbours_query(self, neighbourhood, birth, survive, palette, flags, region):
        q = L.NeighboursQuery(struct_size=C.sizeof(L.NeighboursQuery), neighbourhood=neighbourhood, flags=flags, palette=palette, birth=birth, survive=survive)
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        return q

    def neighbours(self, neighbourhood, birth=0, survive=None, palette=0, region=None, walls=False, tables=True):
        """How many solid neighbours the voxels of a region have, and what one generation of a birth / survive rule would do to them
        (dust_hip_model_neighbours). `neighbourhood` L.NEIGHBOURS_FACES (6), L.NEIGHBOURS_EDGES (18) or L.NEIGHBOURS_CORNERS (26);
        `birth` / `survive` bit masks over the count (count_mask; survive None: every count survives); region = (lo, hi) an inclusive
        voxel box (None: the whole tree); walls: the outside of the tree counts as solid. Returns (result, counts): result a
        NEIGHBOURS_RESULT_DTYPE record (voxels, solid, born, died, lo, hi); counts (2, 27) uint32 with counts[0, n] the empty and
        counts[1, n] the solid voxels with n neighbours, or None with tables=False. The model is only read: no grid is made."""
        if survive is None:
            survive = (2 << neighbourhood) - 1 if neighbourhood in (6, 18, 26) else 0
        q = self._neighbours_query(neighbourhood, birth, survive, palette, L.NEIGHBOURS_WALLS if walls else 0, region)
        out = np.zeros(1, NEIGHBOURS_RESULT_DTYPE)
        counts = np.zeros((2, L.NEIGHBOURS_BINS), np.uint32) if tables else None
        L.check(self._lib.dust_hip_model_neighbours(self._h, C.byref(q), _ptr(out), _ptr(counts) if tables else None))
        return out[0], counts

    def neighbours_apply(self, neighbourhood, birth, survive, generations=1, palette=0, majority=False, region=None, walls=False, per_generation=False):
        """Run `generations` (1..256) synchronous generations of a birth / survive rule on the device (dust_hip_model_neighbours_apply):
        an empty voxel of the region with bit n of `birth` set becomes solid, a solid one with bit n of `survive` clear becomes empty, n
        its solid neighbours. A born voxel takes `palette`, or under majority=True the palette index most of its solid neighbours carry
        (the lowest among equals; `palette` where nobody votes). Returns the NEIGHBOURS_APPLIED_DTYPE record (generations -- 1 + the last
        one that changed a voxel --, solid_before, solid_after, born, died, lo, hi), with per_generation=True (record, table), table a
        (generations, 2) uint32 array of born and died per generation. Scenes instancing the model must be committed again; both fields
        and the island labelling are invalid afterwards."""
        flags = (L.NEIGHBOURS_WALLS if walls else 0) | (L.NEIGHBOURS_MAJORITY if majority else 0)
        q = self._neighbours_query(neighbourhood, birth, survive, palette, flags, region)
        out = np.zeros(1, NEIGHBOURS_APPLIED_DTYPE)
        table = np.zeros((max(int(generations), 0), 2), np.uint32) if per_generation else None
        L.check(self._lib.dust_hip_model_neighbours_apply(self._h, C.byref(q), int(generations), _ptr(out), _ptr(table) if per_generation and table.size else None))
        return (out[0], table) if per_generation else out[0]

    def _settle_query(self, toward, loose, lo, hi):
        q = L.SettleQuery(struct_size=C.sizeof(L.SettleQuery), toward=toward)
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        q.loose[:] = [int(w) for w in (loose_mask() if loose is None else loose)]
        return q

    def settle(self, toward, loose=None, lo=(0, 0, 0), hi=(255, 255, 255)):
        """What one fall of the loose voxels of a region toward a side would do (dust_hip_model_settle). `toward` one L.FACE_* bit
        (L.FACE_NEG_Y: ordinary gravity); `loose` the eight words of loose_mask (None: every palette index is loose); lo / hi an
        inclusive voxel box. Returns a SETTLE_RESULT_DTYPE record (columns, loose, fixed, moved, changed, fall_max, fall_sum, lo, hi,
        changed_columns). The model is only read; a grid is made only when `loose` is not all-ones."""
        q = self._settle_query(toward, loose, lo, hi)
        out = np.zeros(1, SETTLE_RESULT_DTYPE)
        L.check(self._lib.dust_hip_model_settle(self._h, C.byref(q), _ptr(out)))
        return out[0]

    def settle_apply(self, toward, loose=None, lo=(0, 0, 0), hi=(255, 255, 255), generations=0, per_generation=False):
        """Let the loose voxels of a region fall toward a side, then run `generations` (0..256) generations of a 45 degree slide in
        +u, -u, +v, -v by turns and a fall (dust_hip_model_settle_apply); 0 generations is a plain vertical settle. Returns the
        SETTLE_APPLIED_DTYPE record (generations -- 1 + the last one that moved a voxel --, first_moved, loose, slid, fell, fall_sum,
        lo, hi), with per_generation=True (record, table), table a (generations, 2) uint32 array of slid and fell per generation.
        Scenes instancing the model must be committed again; both fields and the island labelling are invalid afterwards."""
        q = self._settle_query(toward, loose, lo, hi)
        out = np.zeros(1, SETTLE_APPLIED_DTYPE)
        table = np.zeros((max(int(generations), 0), 2), np.uint32) if per_generation else None
        L.check(self._lib.dust_hip_model_settle_apply(self._h, C.byref(q), int(generations), _ptr(out), _ptr(table) if per_generation and table.size else None))
        return (out[0], table) if per_generation else out[0]

    def find_islands(self, connectivity=L.ISLANDS_FACES, anchor=None, capacity=None, records=None):
        """Label the model's connected solid voxels (dust_hip_model_find_islands): returns (n, records) -- n the number of islands,
        records the first min(n, capacity) of them as an ISLAND_DTYPE array in ascending key order (key: x << 16 | y << 8 | z of the
        island's smallest voxel). anchor: (lo, hi), an inclusive voxel box; islands with a voxel inside carry L.ISLAND_ANCHORED.
        capacity None: every island (counted first; the second call keeps the first one's labelling); 0: count only. records: an array to fill instead of a fresh one (slots past n
        are left as they are). The labelling stays on the device for island_of and detach_islands until the next edit."""
        q = L.IslandQuery(struct_size=C.sizeof(L.IslandQuery), connectivity=connectivity)
        lo, hi = ((1, 1, 1), (0, 0, 0)) if anchor is None else anchor
        q.anchor_lo[:] = [int(v) for v in lo]
        q.anchor_hi[:] = [int(v) for v in hi]
        n = C.c_uint32()
        if records is not None:
            assert records.dtype == ISLAND_DTYPE and records.flags.c_contiguous
            capacity = len(records)
        elif capacity is None:
            L.check(self._lib.dust_hip_model_find_islands(self._h, C.byref(q), C.byref(n), None, 0))
            capacity = n.value
        if records is None:
            records = np.zeros(capacity, ISLAND_DTYPE)
        L.check(self._lib.dust_hip_model_find_islands(self._h, C.byref(q), C.byref(n), _ptr(records) if capacity else None, capacity))
        return n.value, records[: min(n.value, capacity)]

    def island_of(self, xyz):
        """the key of each voxel's island under the last find_islands (dust_hip_model_island_of); L.NO_ISLAND where the voxel is empty"""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        keys = np.zeros(len(xyz), np.uint32)
        L.check(self._lib.dust_hip_model_island_of(self._h, _ptr(xyz), _ptr(keys), len(keys)))
        return keys

    def detach_islands(self, keys, keep_source=False, want_model=True):
        """Move the islands named by `keys` (of the last find_islands) out of the model (dust_hip_model_detach_islands). Returns a new
        Model holding exactly their voxels at the same tree coordinates -- or None with want_model=False (the islands are deleted) or
        with no keys. keep_source: copy, the source stays as it is. Otherwise scenes instancing the source must be committed again;
        its labelling stays valid for the islands that remain."""
        keys = np.ascontiguousarray(keys, np.uint32).reshape(-1)
        h = C.c_void_p()
        L.check(self._lib.dust_hip_model_detach_islands(self._h, _ptr(keys), len(keys), L.DETACH_KEEP_SOURCE if keep_source else 0,
                                                        C.byref(h) if want_model else None))
        if not h:
            return None
        piece = Model.__new__(Model)
        piece._ctx, piece._lib, piece._h = self._ctx, self._lib, h
        return piece

    def stamp(self, source, stamps, palette_map=None):
        """Paste voxels of `source` (another Model of the same context, or this one) into this model (dust_hip_model_stamp): `stamps` a
        STAMP_DTYPE array (see stamps()), applied in order; every stamp reads the source as it stood when the call began. palette_map:
        255 palette indices, the index a source voxel of index i arrives with (None: its own). Returns `changed`: per stamp, the
        voxels whose value it changed. The source is not modified; scenes instancing this model must be committed again afterwards."""
        stamps = np.ascontiguousarray(stamps, STAMP_DTYPE).reshape(-1)
        changed = np.zeros(len(stamps), np.uint32)
        pm = None
        if palette_map is not None:
            pm = np.ascontiguousarray(palette_map, np.uint8).reshape(-1)
            assert len(pm) == 255
        L.check(self._lib.dust_hip_model_stamp(self._h, source._h, _ptr(stamps), len(stamps), None if pm is None else _ptr(pm), _ptr(changed)))
        return changed

    def resample(self, source, records, palette_map=None, dry_run=False):
        """Paste voxels of `source` (another Model of the same context, or this one) into this model under any rotation, scale or shear
        (dust_hip_model_resample): `records` a RESAMPLE_DTYPE array (see resamples()), applied in order as stamps are; palette_map as
        in stamp(). Each destination voxel's centre is taken through the record's fixed-point inverse map and reads the source voxel it
        lands in; voxels that land outside the source sub-box keep their value. Returns a RESAMPLE_COUNT_DTYPE array: changed, covered,
        solid and blocked per record. dry_run: nothing is written and every record is counted against this model as it stands
        (blocked == 0: the piece fits). The result is defined by the integer record, not by the float matrix it was rounded from."""
        records = np.ascontiguousarray(records, RESAMPLE_DTYPE).reshape(-1)
        counts = np.zeros(len(records), RESAMPLE_COUNT_DTYPE)
        pm = None
        if palette_map is not None:
            pm = np.ascontiguousarray(palette_map, np.uint8).reshape(-1)
            assert len(pm) == 255
        L.check(self._lib.dust_hip_model_resample(self._h, source._h, _ptr(records), len(records), None if pm is None else _ptr(pm),
                                                  L.RESAMPLE_DRY_RUN if dry_run else 0, _ptr(counts)))
        return counts

    def cast(self, source, casts):
        """How far pieces of `source` (another Model of the same context, or this one) move inside this model before a voxel of them is
        blocked (dust_hip_model_cast): `casts` a CAST_DTYPE array (see casts()), each independent of the others. Returns a CAST_HIT_DTYPE
        array: steps (the free steps: the piece rests at offset + steps * step, ready for stamps()), flags (L.CAST_HIT, L.CAST_OVERLAP,
        L.CAST_HIT_WALL), contacts, voxels, contact and src_key. Both models are only read."""
        casts = np.ascontiguousarray(casts, CAST_DTYPE).reshape(-1)
        hits = np.zeros(len(casts), CAST_HIT_DTYPE)
        L.check(self._lib.dust_hip_model_cast(self._h, source._h, _ptr(casts) if len(casts) else None, len(casts), _ptr(hits) if len(casts) else None))
        return hits

    def flood(self, seeds, medium=L.FLOOD_EMPTY, palette=0, max_steps=L.FLOOD_MAX_STEPS, region=None):
        """Step distances from `seeds` (n, 3) through the passable voxels (dust_hip_model_flood): medium L.FLOOD_EMPTY (voxels holding
        None), L.FLOOD_SOLID (solid voxels) or L.FLOOD_MATERIAL (solid voxels of palette index `palette`); steps go through shared faces,
        at most max_steps of them, inside region = (lo, hi), an inclusive voxel box (None: the whole tree). Returns the result as a
        FLOOD_RESULT_DTYPE record (reached, farthest, seeds_used, boundary, lo, hi). The field stays on the device for flood_at,
        flood_paths and flood_apply until the next edit."""
        seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1, 3)
        q = L.FloodQuery(struct_size=C.sizeof(L.FloodQuery), medium=medium, palette=palette, max_steps=max_steps)
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        out = np.zeros(1, FLOOD_RESULT_DTYPE)
        L.check(self._lib.dust_hip_model_flood(self._h, C.byref(q), _ptr(seeds) if len(seeds) else None, len(seeds), _ptr(out)))
        return out[0]

    def flood_at(self, xyz):
        """steps of each voxel under the last flood (dust_hip_model_flood_at): uint16, L.FLOOD_UNREACHED where the flood did not get"""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        steps = np.zeros(len(xyz), np.uint16)
        L.check(self._lib.dust_hip_model_flood_at(self._h, _ptr(xyz), _ptr(steps), len(steps)))
        return steps

    def flood_paths(self, starts, capacity, keys=None):
        """Descend the last flood's field from each start to a seed (dust_hip_model_flood_paths). Returns (lengths, keys): lengths[i] the
        voxels of path i (steps + 1; 0 for an unreached start), keys (n, capacity) its first min(lengths[i], capacity) voxels as
        x << 16 | y << 8 | z, the start first (slots past them are left as they are: zero, or what the given `keys` array held).
        capacity 2: the next step toward the goal."""
        starts = np.ascontiguousarray(starts, np.uint32).reshape(-1, 3)
        lengths = np.zeros(len(starts), np.uint32)
        if keys is None:
            keys = np.zeros((len(starts), capacity), np.uint32)
        assert keys.dtype == np.uint32 and keys.flags.c_contiguous and keys.shape == (len(starts), capacity)
        L.check(self._lib.dust_hip_model_flood_paths(self._h, _ptr(starts), len(starts), capacity, _ptr(keys) if capacity else None, _ptr(lengths)))
        return lengths, keys

    def flood_apply(self, value, max_steps=None):
        """Every voxel the last flood reached within max_steps (None: all of them) takes `value`, a palette index or -1 for None
        (dust_hip_model_flood_apply). Returns the number of voxels that changed. Scenes instancing the model must be committed again;
        the field and the island labelling are invalid afterwards."""
        changed = C.c_uint32()
        L.check(self._lib.dust_hip_model_flood_apply(self._h, 0xFFFFFFFF if max_steps is None else int(max_steps), int(value), C.byref(changed)))
        return changed.value

    def fracture(self, seeds, region=None, palette=None, scale=(1, 1, 1), max_distance2=None, records=True):
        """Label every counted voxel with the index of its nearest seed (dust_hip_model_fracture): `seeds` an (n, 3) integer array or a
        FRACTURE_SEED_DTYPE array (see fracture_seeds()), coordinates -1024..1279; counted are the solid voxels of region = (lo, hi),
        an inclusive voxel box (None: the whole tree), of palette index `palette` (None: any); the metric is
        scale[0] dx^2 + scale[1] dy^2 + scale[2] dz^2, ties go to the lowest seed index; a voxel farther than max_distance2 (None: no
        limit) from every seed stays unlabelled. Returns (result, cells): a FRACTURE_RESULT_DTYPE record and a FRACTURE_CELL_DTYPE
        array with one record per seed -- or None with records=False, which only makes the labels. They stay on the device for
        fracture_at, fracture_detach and fracture_apply until the next edit."""
        seeds = fracture_seeds(seeds)
        q = L.FractureQuery(struct_size=C.sizeof(L.FractureQuery), flags=0, palette=-1 if palette is None else int(palette),
                            max_distance2=L.FRACTURE_NO_LIMIT if max_distance2 is None else int(max_distance2))
        q.scale[:] = [int(v) for v in scale]
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        result = np.zeros(1, FRACTURE_RESULT_DTYPE)
        cells = np.zeros(len(seeds), FRACTURE_CELL_DTYPE)
        L.check(self._lib.dust_hip_model_fracture(self._h, C.byref(q), _ptr(seeds) if len(seeds) else None, len(seeds), _ptr(result) if records else None,
                                                  _ptr(cells) if records and len(seeds) else None))
        return (result[0], cells) if records else None

    def fracture_at(self, xyz):
        """the cell of each voxel under the last fracture (dust_hip_model_fracture_at): uint16, L.NO_CELL where the voxel has none"""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        cells = np.zeros(len(xyz), np.uint16)
        L.check(self._lib.dust_hip_model_fracture_at(self._h, _ptr(xyz), _ptr(cells), len(cells)))
        return cells

    def fracture_detach(self, cells, keep_source=False, receive=True):
        """Move the union of the cells named by `cells` (indices of the last fracture's seeds) out of the model
        (dust_hip_model_fracture_detach). Returns a new Model holding exactly their voxels at the same tree coordinates -- or None with
        receive=False (the cells are deleted) or with no cells. keep_source: copy, the source stays as it is. Otherwise scenes
        instancing the source must be committed again; the removed voxels answer L.NO_CELL and the rest of the labelling stands. For
        chunks: one fracture, one keep_source detach per piece, then one deleting detach of all of them."""
        cells = np.ascontiguousarray(cells, np.uint32).reshape(-1)
        h = C.c_void_p()
        L.check(self._lib.dust_hip_model_fracture_detach(self._h, _ptr(cells) if len(cells) else None, len(cells), L.DETACH_KEEP_SOURCE if keep_source else 0,
                                                         C.byref(h) if receive else None))
        if not h:
            return None
        piece = Model.__new__(Model)
        piece._ctx, piece._lib, piece._h = self._ctx, self._lib, h
        return piece

    def fracture_apply(self, value, where=L.FRACTURE_SEAMS):
        """The seam voxels of the last fracture (where=L.FRACTURE_SEAMS: labelled voxels with a face-neighbour of a higher cell) or all
        its labelled voxels (L.FRACTURE_LABELLED) take `value`, a palette index or -1 for None (dust_hip_model_fracture_apply). Returns
        the number of voxels that changed. Scenes instancing the model must be committed again; the labelling, the fields and the
        island labelling are invalid afterwards."""
        changed = C.c_uint32()
        L.check(self._lib.dust_hip_model_fracture_apply(self._h, int(where), int(value), C.byref(changed)))
        return changed.value

    def bodies(self, group=L.BODIES_ALL, weights=None, palette=-1, region=None, capacity=None):
        """Mass, first and second moments per group of voxels (dust_hip_model_bodies): what a rigid-body solver needs of a piece.
        `group` L.BODIES_ALL (one record, key 0), L.BODIES_MATERIALS (255 records, key the palette index), L.BODIES_ISLANDS (one per
        island of the standing find_islands labelling, ascending keys) or L.BODIES_CELLS (one per seed of the standing fracture).
        `weights` 255 integers 0..65535 by palette index, None: every voxel weighs 1. `palette` and `region` select the voxels as in
        Model.surface. Returns a BODY_DTYPE array (key, voxels, lo, hi, mass, m1 = sums of w x, w y, w z, m2 = sums of w xx, w yy,
        w zz, w xy, w yz, w zx over integer voxel coordinates) of the first min(groups, capacity) groups -- capacity=None makes two
        calls, one to count. body_properties turns the records into mass, centre of mass and inertia tensor. The model is only read."""
        q = L.BodyQuery(struct_size=C.sizeof(L.BodyQuery), group=int(group), palette=int(palette))
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        w = None
        if weights is not None:
            wide = np.asarray(weights).reshape(-1)
            if wide.shape != (L.BODY_WEIGHTS,) or wide.min() < 0 or wide.max() > 65535:
                raise ValueError("weights must be 255 integers in 0..65535")
            w = np.ascontiguousarray(wide, dtype=np.uint16)
        n = C.c_uint32()
        if capacity is None:
            L.check(self._lib.dust_hip_model_bodies(self._h, C.byref(q), _ptr(w) if w is not None else None, C.byref(n), None, 0))
            capacity = n.value
        records = np.zeros(int(capacity), BODY_DTYPE)
        L.check(self._lib.dust_hip_model_bodies(self._h, C.byref(q), _ptr(w) if w is not None else None, C.byref(n),
                                                _ptr(records) if capacity else None, int(capacity)))
        return records[: min(int(capacity), n.value)]

    def joints(self, group, region=None, capacity=None):
        """The contact faces between neighbouring groups of voxels (dust_hip_model_joints): one JOINT_DTYPE record per pair of distinct
        groups that share at least one voxel face, in ascending (a, b). `group` L.JOINTS_MATERIALS (a voxel's group is its palette
        index) or L.JOINTS_CELLS (its cell of the standing fracture; a solid voxel beyond it has group L.JOINT_REST, always b). Only
        the solid voxels inside `region` (clipped to the tree) exist. A record holds faces, by_face (the direction from the a voxel to
        the b voxel: -x, +x, -y, +y, -z, +z), lo2 / hi2 and sum2 (bounds and sums of the face centres in half voxels). Returns the
        first min(pairs, capacity) records -- capacity=None makes two calls, one to count. joint_properties turns the records into
        area, anchor and normal. The model is only read."""
        q = L.JointQuery(struct_size=C.sizeof(L.JointQuery), group=int(group), palette=-1)
        lo, hi = ((0, 0, 0), (255, 255, 255)) if region is None else region
        q.lo[:] = [int(v) for v in lo]
        q.hi[:] = [int(v) for v in hi]
        n = C.c_uint32()
        if capacity is None:
            L.check(self._lib.dust_hip_model_joints(self._h, C.byref(q), C.byref(n), None, 0))
            capacity = n.value
        records = np.zeros(int(capacity), JOINT_DTYPE)
        L.check(self._lib.dust_hip_model_joints(self._h, C.byref(q), C.byref(n), _ptr(records) if capacity else None, int(capacity)))
        return records[: min(int(capacity), n.value)]

    def distance(self, target=L.DISTANCE_TO_SOLID, metric=L.DISTANCE_EUCLIDEAN, max_radius=L.DISTANCE_MAX_RADIUS, walls=False, palette=0):
        """The exact distance from every voxel to the nearest target (dust_hip_model_distance): target L.DISTANCE_TO_SOLID (the solid
        voxels), L.DISTANCE_TO_EMPTY (the voxels holding None) or L.DISTANCE_TO_MATERIAL (the solid voxels of palette index `palette`);
        metric L.DISTANCE_EUCLIDEAN (the SQUARED distance dx^2 + dy^2 + dz^2) or L.DISTANCE_CHEBYSHEV (max(|dx|, |dy|, |dz|)); values
        above max_radius^2 (max_radius under CHEBYSHEV) are L.DISTANCE_FAR; walls: the voxels outside the tree are targets too. Returns
        the result as a DISTANCE_RESULT_DTYPE record (targets, near, far, largest, largest_key). The field stays on the device for
        distance_at and distance_apply until the next edit."""
        q = L.DistanceQuery(struct_size=C.sizeof(L.DistanceQuery), target=target, metric=metric, flags=L.DISTANCE_WALLS if walls else 0,
                            palette=palette, max_radius=max_radius)
        out = np.zeros(1, DISTANCE_RESULT_DTYPE)
        L.check(self._lib.dust_hip_model_distance(self._h, C.byref(q), _ptr(out)))
        return out[0]

    def distance_at(self, xyz):
        """the value of each voxel in the last distance field (dust_hip_model_distance_at): uint16, L.DISTANCE_FAR beyond the radius"""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        values = np.zeros(len(xyz), np.uint16)
        L.check(self._lib.dust_hip_model_distance_at(self._h, _ptr(xyz), _ptr(values), len(values)))
        return values

    def distance_apply(self, value, lo=1, hi=0xFFFFFFFF):
        """Every voxel whose value in the last distance field is not FAR and lies in lo..hi (the field's units: squared under EUCLIDEAN)
        takes `value`, a palette index or -1 for None (dust_hip_model_distance_apply). Returns the number of voxels that changed.
        Scenes instancing the model must be committed again; the distance field, the flood field and the island labelling are invalid
        afterwards."""
        changed = C.c_uint32()
        L.check(self._lib.dust_hip_model_distance_apply(self._h, int(lo), int(hi), int(value), C.byref(changed)))
        return changed.value

    def reduce(self, levels=1, min_solid=1):
        """A coarser copy of the model as it stands on the device (dust_hip_model_reduce): halved `levels` times (1..L.REDUCE_MAX_LEVELS),
        a coarse voxel solid when at least min_solid (1..8) of its eight children are and carrying the palette index most of them carry
        (the lowest among equals). Returns (model, result): a new editable Model of the same context and palette whose voxels occupy
        [0, 256 >> levels)^3, and a REDUCE_RESULT_DTYPE record (src_voxels, voxels, extent). This model is only read. Instance the copy
        with lod_transform(obj_to_world, levels) to show it where this model stands."""
        q = L.Reduce(struct_size=C.sizeof(L.Reduce), levels=levels, min_solid=min_solid, flags=0)
        h = C.c_void_p()
        out = np.zeros(1, REDUCE_RESULT_DTYPE)
        L.check(self._lib.dust_hip_model_reduce(self._h, C.byref(q), C.byref(h), _ptr(out)))
        coarse = Model.__new__(Model)
        coarse._ctx, coarse._lib, coarse._h = self._ctx, self._lib, h
        return coarse, out[0]

    def read(self):
        """(blocks, materials) as they stand on the device"""
        nb, nm = C.c_uint32(), C.c_uint64()
        L.check(self._lib.dust_hip_model_info(self._h, C.byref(nb), C.byref(nm)))
        blocks = np.zeros(max(nb.value, 1), BLOCK_DTYPE)
        mats = np.zeros(max(nm.value, 1), np.uint8)
        L.check(self._lib.dust_hip_model_read(self._h, _ptr(blocks), len(blocks), _ptr(mats), len(mats)))
        return blocks[: nb.value], mats[: nm.value]

    def read_hierarchy(self):
        """The upper levels as they stand on the device (dust_hip_model_read_hierarchy), as a dict of numpy arrays: extent_log2, n_mid,
        n_l2, bmin / bmax (float32, 3), root (uint8, 656), host_root (uint8, 640: the copy a scene commit uses), mid (MID_NODE_DTYPE,
        n_mid), dense_mask (uint64, n_mid * 64), and for 4096^3 trees l2 (uint8, n_l2 * 656) and l2_cells (L2_CELL_DTYPE, n_l2 * 4096)."""
        info = L.HierarchyInfo(struct_size=C.sizeof(L.HierarchyInfo))
        L.check(self._lib.dust_hip_model_read_hierarchy(self._h, C.byref(info), None, 0, None, 0, None, None, None, 0, None, 0))
        n_mid, n_l2 = info.n_mid, info.n_l2
        mid = np.zeros(max(n_mid, 1), MID_NODE_DTYPE)
        dense = np.zeros(max(n_mid, 1) * 64, np.uint64)
        root, host_root = np.zeros(L.N16_BYTES, np.uint8), np.zeros(L.N16_ROOT_BYTES, np.uint8)
        l2 = np.zeros(max(n_l2, 1) * L.N16_BYTES, np.uint8)
        cells = np.zeros(max(n_l2, 1) * 4096, L2_CELL_DTYPE)
        L.check(self._lib.dust_hip_model_read_hierarchy(self._h, C.byref(info), _ptr(mid), len(mid), _ptr(dense), len(dense), _ptr(root), _ptr(host_root),
                                                        _ptr(l2), max(n_l2, 1), _ptr(cells), len(cells)))
        assert (info.n_mid, info.n_l2) == (n_mid, n_l2)
        return dict(extent_log2=info.extent_log2, n_mid=n_mid, n_l2=n_l2, bmin=np.array(info.bmin, np.float32), bmax=np.array(info.bmax, np.float32),
                    root=root, host_root=host_root, mid=mid[:n_mid], dense_mask=dense[: n_mid * 64], l2=l2[: n_l2 * L.N16_BYTES], l2_cells=cells[: n_l2 * 4096])


class Scene:
    def __init__(self, ctx):
        self._ctx = ctx
        self._lib = ctx._lib
        self._models = []
        self._h = C.c_void_p()
        L.check(self._lib.dust_hip_scene_create(ctx._h, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_hip_scene_destroy(self._h)
            self._h = None

    def add_instance(self, model, obj_to_world, prev=None):
        m = np.ascontiguousarray(obj_to_world, np.float32).reshape(12)
        p = None if prev is None else np.ascontiguousarray(prev, np.float32).reshape(16)
        idx = C.c_uint32()
        L.check(self._lib.dust_hip_scene_add_instance(
            self._h, model._h, m.ctypes.data_as(C.POINTER(C.c_float)),
            None if p is None else p.ctypes.data_as(C.POINTER(C.c_float)), C.byref(idx)))
        self._models.append(model)
        return idx.value

    def set_transform(self, instance, obj_to_world, prev=None):
        """New transform for an instance (castle.rs:287-291 moves the teapot every frame); prev = last frame's
        object-to-world mat4, column-major (standard.rs:845-878), which the motion vectors are measured against."""
        m = np.ascontiguousarray(obj_to_world, np.float32).reshape(12)
        p = None if prev is None else np.ascontiguousarray(prev, np.float32).reshape(16)
        L.check(self._lib.dust_hip_scene_set_transform(
            self._h, instance, m.ctypes.data_as(C.POINTER(C.c_float)),
            None if p is None else p.ctypes.data_as(C.POINTER(C.c_float))))

    def commit(self):
        L.check(self._lib.dust_hip_scene_commit(self._h))

    def trace_rays(self, origins, directions=None, tmin=0.0, tmax=math.inf, any_hit=False, hits=None):
        """What each ray hits in the committed scene (dust_hip_scene_trace_rays): origins / directions (n, 3) in world space, tmin /
        tmax scalars or (n,). Returns a HIT_DTYPE array: t, instance (L.NO_HIT on a miss), block, voxel, xyz (the voxel in the model's
        tree coordinates: what Model.set_voxels / get_voxels take), face (normal2FaceID of the hit face's model-space normal), palette.
        any_hit: some hit in [tmin, tmax], not necessarily the closest. An unbounded tmax (inf) is passed as FLT_MAX: the ABI reports
        a ray with a non-finite tmin or tmax as a miss.
        Device path (dust_hip_scene_trace_rays_async): `origins` a contiguous device tensor of DustHipRay rows ((n, 8) float32, see
        ray_records) and `hits` one of n DustHipRayHit rows; enqueued on the context's stream, valid after Context.sync()."""
        flags = L.QUERY_ANY_HIT if any_hit else 0
        if hits is not None:
            n = origins.numel() * origins.element_size() // RAY_DTYPE.itemsize
            assert directions is None and origins.is_contiguous() and hits.is_contiguous()
            assert origins.numel() * origins.element_size() == n * RAY_DTYPE.itemsize
            assert hits.numel() * hits.element_size() >= n * HIT_DTYPE.itemsize
            L.check(self._lib.dust_hip_scene_trace_rays_async(self._h, C.c_void_p(origins.data_ptr()), C.c_void_p(hits.data_ptr()), n, flags))
            return hits
        rays = ray_records(origins, directions, tmin, tmax)
        out = np.zeros(len(rays), HIT_DTYPE)
        L.check(self._lib.dust_hip_scene_trace_rays(self._h, _ptr(rays), _ptr(out), len(rays), flags))
        return out

    def overlap_boxes(self, lo, hi=None, capacity=64, any_hit=False, counts=None, records=None):
        """The solid voxels inside world-space boxes (dust_hip_scene_overlap_boxes): lo / hi (n, 3), capacity an int or (n,). Returns
        (counts, records_per_query): counts[i] every overlapping voxel, records_per_query[i] a VOXEL_REF_DTYPE array of the first
        min(counts[i], capacity[i]) of them in (instance, block, voxel) order -- instance, block, xyz (the voxel in the model's tree
        coordinates: what Model.set_voxels / get_voxels take), palette, voxel. any_hit: counts are 0 / 1, the record some overlapping voxel.
        Device path (dust_hip_scene_overlap_boxes_async): `lo` a contiguous device tensor of DustHipBoxQuery rows ((n, 8) 32-bit words,
        see box_queries), `counts` one of n uint32 and `records` one of DustHipVoxelRef rows ((m, 4) 32-bit words); enqueued on the
        context's stream, valid after Context.sync(). Returns (counts, records) as given."""
        flags = L.QUERY_ANY_HIT if any_hit else 0
        if counts is not None:
            assert hi is None and records is not None and lo.is_contiguous() and counts.is_contiguous() and records.is_contiguous()
            n = lo.numel() * lo.element_size() // BOX_QUERY_DTYPE.itemsize
            assert lo.numel() * lo.element_size() == n * BOX_QUERY_DTYPE.itemsize and counts.numel() * counts.element_size() >= 4 * n
            n_rec = records.numel() * records.element_size() // VOXEL_REF_DTYPE.itemsize
            L.check(self._lib.dust_hip_scene_overlap_boxes_async(self._h, C.c_void_p(lo.data_ptr()), n, C.c_void_p(counts.data_ptr()),
                                                                 C.c_void_p(records.data_ptr()), n_rec, flags))
            return counts, records
        boxes = box_queries(lo, hi, capacity)
        n_rec = int(boxes["capacity"].sum(dtype=np.int64))
        out_counts = np.zeros(len(boxes), np.uint32)
        out = np.zeros(max(n_rec, 1), VOXEL_REF_DTYPE)
        L.check(self._lib.dust_hip_scene_overlap_boxes(self._h, _ptr(boxes), len(boxes), _ptr(out_counts), _ptr(out), n_rec, flags))
        per = [out[int(f): int(f) + int(min(c, k))] for f, c, k in zip(boxes["first"], out_counts, boxes["capacity"])]
        return out_counts, per

    def sweep_boxes(self, lo, hi=None, delta=None, any_hit=False, ignore_start=False, hits=None):
        """The first solid voxel each world-space box touches as it moves by delta (dust_hip_scene_sweep_boxes): lo / hi / delta (n, 3).
        Returns a SWEEP_HIT_DTYPE array: t (first contact in [0, 1); 1 on a miss), instance (NO_HIT on a miss), block, xyz (the voxel
        in the model's tree coordinates), palette, voxel, normal (from the voxel toward the box; 0 when the box starts inside it).
        any_hit: some hit voxel, not necessarily the first; ignore_start: voxels the box is inside at t = 0 do not stop it.
        Device path (dust_hip_scene_sweep_boxes_async): `lo` a contiguous device tensor of DustHipBoxSweep rows ((n, 12) 32-bit words,
        see box_sweeps) and `hits` one of DustHipSweepHit rows ((n, 8) 32-bit words); enqueued on the context's stream, valid after
        Context.sync(). Returns `hits`."""
        flags = (L.QUERY_ANY_HIT if any_hit else 0) | (L.SWEEP_IGNORE_START if ignore_start else 0)
        if hits is not None:
            assert hi is None and delta is None and lo.is_contiguous() and hits.is_contiguous()
            n = lo.numel() * lo.element_size() // BOX_SWEEP_DTYPE.itemsize
            assert lo.numel() * lo.element_size() == n * BOX_SWEEP_DTYPE.itemsize
            assert hits.numel() * hits.element_size() >= n * SWEEP_HIT_DTYPE.itemsize
            L.check(self._lib.dust_hip_scene_sweep_boxes_async(self._h, C.c_void_p(lo.data_ptr()), C.c_void_p(hits.data_ptr()), n, flags))
            return hits
        sweeps = box_sweeps(lo, hi, delta)
        out = np.zeros(len(sweeps), SWEEP_HIT_DTYPE)
        L.check(self._lib.dust_hip_scene_sweep_boxes(self._h, _ptr(sweeps), _ptr(out), len(sweeps), flags))
        return out


def ray_records(origins, directions, tmin=0.0, tmax=math.inf):
    """DustHipRay records (RAY_DTYPE) for Scene.trace_rays; tmax = +inf becomes FLT_MAX (an unbounded ray)"""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    assert len(o) == len(d)
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    rays["tmin"] = np.broadcast_to(np.asarray(tmin, np.float32), (len(o),))
    tm = np.broadcast_to(np.asarray(tmax, np.float32), (len(o),))
    rays["tmax"] = np.where(tm == np.float32(np.inf), np.float32(FLT_MAX), tm)
    return rays


def box_queries(lo, hi, capacity=64):
    """DustHipBoxQuery records (BOX_QUERY_DTYPE) for Scene.overlap_boxes: the slices [first, first + capacity) laid end to end"""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    hi = np.asarray(hi, np.float32).reshape(-1, 3)
    assert len(lo) == len(hi)
    boxes = np.zeros(len(lo), BOX_QUERY_DTYPE)
    boxes["lo"], boxes["hi"] = lo, hi
    cap = np.broadcast_to(np.asarray(capacity, np.int64), (len(lo),))
    assert np.all(cap >= 0) and int(cap.sum()) < 2 ** 32
    boxes["capacity"] = cap
    boxes["first"] = np.concatenate([[0], np.cumsum(cap)[:-1]]) if len(lo) else 0
    return boxes


def box_sweeps(lo, hi, delta):
    """DustHipBoxSweep records (BOX_SWEEP_DTYPE) for Scene.sweep_boxes: the box [lo, hi] at t = 0, moving by delta over t in [0, 1]"""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    hi = np.asarray(hi, np.float32).reshape(-1, 3)
    delta = np.asarray(delta, np.float32).reshape(-1, 3)
    assert len(lo) == len(hi) == len(delta)
    sweeps = np.zeros(len(lo), BOX_SWEEP_DTYPE)
    sweeps["lo"], sweeps["hi"], sweeps["delta"] = lo, hi, delta
    return sweeps


def edit_shapes(kind, a, b=None, radius=0.0, op=L.EDIT_CARVE, palette=0):
    """DustHipEditShape records (EDIT_SHAPE_DTYPE) for Model.edit_shapes: a (n, 3) is a box's lo, a sphere's centre or a capsule's
    segment start; b (n, 3) a box's hi or a capsule's segment end (spheres: omitted); kind, radius, op and palette scalars or (n,).
    Tree coordinates: a crater at a picked voxel is a = hit["xyz"] + 0.5."""
    a = np.asarray(a, np.float32).reshape(-1, 3)
    b = a if b is None else np.asarray(b, np.float32).reshape(-1, 3)
    assert len(a) == len(b)
    shapes = np.zeros(len(a), EDIT_SHAPE_DTYPE)
    shapes["a"], shapes["b"] = a, b
    shapes["kind"] = np.broadcast_to(np.asarray(kind, np.uint32), (len(a),))
    shapes["radius"] = np.broadcast_to(np.asarray(radius, np.float32), (len(a),))
    shapes["op"] = np.broadcast_to(np.asarray(op, np.uint32), (len(a),))
    shapes["palette"] = np.broadcast_to(np.asarray(palette, np.int32), (len(a),))
    return shapes


def fracture_seeds(points):
    """DustHipFractureSeed records (FRACTURE_SEED_DTYPE) for Model.fracture: points an (n, 3) integer array of voxel coordinates (may lie
    outside the tree, -1024..1279; not clamped), or such records already"""
    if isinstance(points, np.ndarray) and points.dtype == FRACTURE_SEED_DTYPE:
        return np.ascontiguousarray(points).reshape(-1)
    points = np.asarray(points, np.int64).reshape(-1, 3)
    out = np.zeros(len(points), FRACTURE_SEED_DTYPE)
    out["x"], out["y"], out["z"] = points[:, 0], points[:, 1], points[:, 2]
    return out


def triangles(vertices, op=L.EDIT_FILL, palette=0):
    """DustHipTriangle records (TRIANGLE_DTYPE) for Model.edit_triangles and Model.fill_mesh: vertices a float (n, 3, 3) array in
    voxels of the model's tree coordinates, rounded to the ABI's integers as rint(v * 256) and not clamped (a triangle with a coordinate
    beyond +-1024 voxels covers nothing); op and palette scalars or (n,)."""
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3, 3)
    out = np.zeros(len(vertices), TRIANGLE_DTYPE)
    out["v"] = np.rint(vertices * L.TRIANGLE_UNIT).astype(np.int64).astype(np.int32)
    out["op"] = np.broadcast_to(np.asarray(op, np.uint32), (len(vertices),))
    out["palette"] = np.broadcast_to(np.asarray(palette, np.int32), (len(vertices),))
    return out


def quads_to_triangles(quads, op=L.EDIT_FILL, palette=0):
    """Model.mesh's quads (MESH_QUAD_DTYPE) as TRIANGLE_DTYPE records, two per quad -- (c0, c1, c2) and (c0, c2, c3) of mesh_corners, on
    integer voxel corners, so that Model.fill_mesh of a model's whole mesh gives the model's voxels back."""
    corners, _ = mesh_corners(quads)
    c = corners.astype(np.int32) * L.TRIANGLE_UNIT
    out = np.zeros(2 * len(c), TRIANGLE_DTYPE)
    out["v"][0::2] = c[:, [0, 1, 2]]
    out["v"][1::2] = c[:, [0, 2, 3]]
    out["op"] = np.broadcast_to(np.asarray(op, np.uint32), (len(out),))
    out["palette"] = np.broadcast_to(np.asarray(palette, np.int32), (len(out),))
    return out


def orientation(perm=(0, 1, 2), flips=(False, False, False)):
    """DustHipStamp.orient: destination axis r reads source axis perm[r], backwards where flips[r] (48 signed axis permutations)"""
    perm = [int(p) for p in perm]
    assert sorted(perm) == [0, 1, 2] and len(flips) == 3
    return perm[0] | (perm[1] << 2) | (perm[2] << 4) | sum((1 << (6 + r)) for r in range(3) if flips[r])


def stamps(offset, orient=ORIENT_IDENTITY, op=L.STAMP_PLACE, src_lo=(0, 0, 0), src_hi=(255, 255, 255)):
    """DustHipStamp records (STAMP_DTYPE) for Model.stamp: offset (n, 3), where the lowest corner of each image box lands in the
    destination; src_lo / src_hi (3,) or (n, 3), the inclusive sub-box of the source; orient (see orientation()) and op scalars or (n,)."""
    offset = np.asarray(offset, np.int32).reshape(-1, 3)
    out = np.zeros(len(offset), STAMP_DTYPE)
    out["offset"] = offset
    out["orient"] = np.broadcast_to(np.asarray(orient, np.uint32), (len(offset),))
    out["op"] = np.broadcast_to(np.asarray(op, np.uint32), (len(offset),))
    out["src_lo"] = np.broadcast_to(np.asarray(src_lo, np.uint8), (len(offset), 3))
    out["src_hi"] = np.broadcast_to(np.asarray(src_hi, np.uint8), (len(offset), 3))
    return out


def resamples(forward, op=L.STAMP_PLACE, src_lo=(0, 0, 0), src_hi=(255, 255, 255)):
    """DustHipResample records (RESAMPLE_DTYPE) for Model.resample from FORWARD maps: `forward` (3, 4) or (n, 3, 4) float matrices that
    take source voxel space to destination voxel space (voxel v covers [v, v + 1) on each axis; column 3 is the translation). Each is
    inverted in float64 and the inverse rounded to 1 / 65536 -- the record holds the inverse, and the result is defined by that integer
    record, not by the float matrix. The destination box is the forward image of [src_lo, src_hi + 1], padded by one voxel. op scalar
    or (n,); src_lo / src_hi (3,) or (n, 3), the inclusive sub-box of the source. ValueError: a singular matrix, or an inverse beyond
    the call's limits (|m| <= 8, |t| <= 4096 voxels)."""
    forward = np.asarray(forward, np.float64).reshape(-1, 3, 4)
    n = len(forward)
    out = np.zeros(n, RESAMPLE_DTYPE)
    out["op"] = np.broadcast_to(np.asarray(op, np.uint32), (n,))
    out["src_lo"] = np.broadcast_to(np.asarray(src_lo, np.uint8), (n, 3))
    out["src_hi"] = np.broadcast_to(np.asarray(src_hi, np.uint8), (n, 3))
    for i, f in enumerate(forward):
        a, b = f[:, :3], f[:, 3]
        if not np.isfinite(f).all() or abs(np.linalg.det(a)) < 1e-12:
            raise ValueError("resamples: the forward matrix is singular or not finite (write a singular inverse into the record directly)")
        inv = np.linalg.inv(a)
        m = np.rint(inv * L.RESAMPLE_ONE)
        t = np.rint(-(inv @ b) * L.RESAMPLE_ONE)
        if np.abs(m).max() > L.RESAMPLE_MAX_M or np.abs(t).max() > L.RESAMPLE_MAX_T:
            raise ValueError("resamples: the inverse map is beyond the limits (|m| <= 8.0, |t| <= 4096 voxels)")
        out["m"][i] = m.astype(np.int64)
        out["t"][i] = t.astype(np.int64)
        lo, hi = out["src_lo"][i].astype(np.float64), out["src_hi"][i].astype(np.float64) + 1.0
        corners = np.array([[(lo, hi)[(c >> r) & 1][r] for r in range(3)] for c in range(8)])
        image = corners @ a.T + b
        limit = float(2 ** 31 - 1)
        out["dst_lo"][i] = np.clip(np.floor(image.min(axis=0)) - 1.0, -limit - 1.0, limit).astype(np.int64)
        out["dst_hi"][i] = np.clip(np.ceil(image.max(axis=0)), -limit - 1.0, limit).astype(np.int64)
    return out


def rotation_about(axis, degrees, pivot_src, pivot_dst, scale=1.0):
    """A forward (3, 4) matrix for resamples(): the rotation by `degrees` about `axis` (0, 1, 2, "x", "y", "z" or any non-zero
    3-vector; right-handed), scaled by `scale`, that takes the source position pivot_src to the destination position pivot_dst
    (positions in voxel space: the centre of voxel v is v + 0.5)."""
    if isinstance(axis, str):
        axis = "xyz".index(axis)
    if np.ndim(axis) == 0:
        axis = np.eye(3)[int(axis)]
    u = np.asarray(axis, np.float64).reshape(3)
    u = u / np.linalg.norm(u)
    a = np.radians(float(degrees))
    k = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    r = (np.eye(3) + np.sin(a) * k + (1.0 - np.cos(a)) * (k @ k)) * float(scale)
    out = np.zeros((3, 4))
    out[:, :3] = r
    out[:, 3] = np.asarray(pivot_dst, np.float64) - r @ np.asarray(pivot_src, np.float64)
    return out


def casts(offset, step, max_steps, orient=ORIENT_IDENTITY, flags=0, src_lo=(0, 0, 0), src_hi=(255, 255, 255)):
    """DustHipCast records (CAST_DTYPE) for Model.cast: offset (n, 3), where the lowest corner of each image box is at placement 0; step (3,)
    or (n, 3), each component -1, 0 or 1; max_steps (0: a fit test), orient (see orientation()) and flags (L.CAST_WALLS) scalars or (n,);
    src_lo / src_hi (3,) or (n, 3), the inclusive sub-box of the source."""
    offset = np.asarray(offset, np.int32).reshape(-1, 3)
    out = np.zeros(len(offset), CAST_DTYPE)
    out["offset"] = offset
    out["orient"] = np.broadcast_to(np.asarray(orient, np.uint32), (len(offset),))
    out["step"] = np.broadcast_to(np.asarray(step, np.int32), (len(offset), 3))
    out["max_steps"] = np.broadcast_to(np.asarray(max_steps, np.uint32), (len(offset),))
    out["flags"] = np.broadcast_to(np.asarray(flags, np.uint32), (len(offset),))
    out["src_lo"] = np.broadcast_to(np.asarray(src_lo, np.uint8), (len(offset), 3))
    out["src_hi"] = np.broadcast_to(np.asarray(src_hi, np.uint8), (len(offset), 3))
    return out


def lod_transform(obj_to_world, levels):
    """The obj_to_world (3 x 4, row-major) of an instance of Model.reduce(levels)'s model that stands where an instance of the source
    with `obj_to_world` stands: columns 0..2 scaled by 2^levels, the translation unchanged."""
    m = np.array(obj_to_world, np.float32).reshape(3, 4)
    m[:, :3] *= np.float32(2 ** int(levels))
    return m


def mesh_corners(quads):
    """Host only: the corners and normals of Model.mesh's quads -> (corners int32 (N, 4, 3), normals int8 (N, 3)). Corner positions are
    on the voxel-corner lattice 0..256: voxel (x, y, z) spans x..x+1, y..y+1, z..z+1, and a face of a + direction lies on the plane
    coordinate + 1. The corners go counter-clockwise seen from outside: cross(c1 - c0, c3 - c0) is normal * area; c0 is the corner
    at the quad's lowest u and v."""
    quads = np.asarray(quads, MESH_QUAD_DTYPE)
    n_quads = len(quads)
    key = quads["key"].astype(np.int64)
    face = quads["face"].astype(np.int64)
    axis = face >> 1
    rows = np.arange(n_quads)
    base = np.stack([key >> 16, (key >> 8) & 255, key & 255], axis=1)
    base[rows, axis] += face & 1
    u_axis = np.where(axis == 2, 1, 2)                    # the higher-numbered remaining axis
    v_axis = np.where(axis == 0, 1, 0)
    along_u = np.zeros((n_quads, 3), np.int64)
    along_v = np.zeros((n_quads, 3), np.int64)
    along_u[rows, u_axis] = quads["du"].astype(np.int64) + 1
    along_v[rows, v_axis] = quads["dv"].astype(np.int64) + 1
    v_first = np.isin(face, (1, 2, 5))[:, None]           # e_v x e_u points along +n for n = x and z, e_u x e_v for n = y
    first, second = np.where(v_first, along_v, along_u), np.where(v_first, along_u, along_v)
    corners = np.stack([base, base + first, base + first + second, base + second], axis=1).astype(np.int32)
    normals = np.zeros((n_quads, 3), np.int8)
    normals[rows, axis] = np.where(face & 1, 1, -1)
    return corners, normals


def body_properties(records, voxel_size=1.0):
    """Host only: Model.bodies' records -> (mass, com, inertia): mass (n,) the sum of the weights; com (n, 3) the centre of mass,
    (m1 / mass + 0.5) * voxel_size; inertia (n, 3, 3) the tensor about the centre of mass with every voxel a solid cube of side
    voxel_size: C_ab = m2_ab - m1_a m1_b / mass, I_xx = (C_yy + C_zz + mass / 6) * voxel_size^2, I_xy = -C_xy * voxel_size^2. Computed
    in exact rational arithmetic and rounded once to float64. A record of mass 0 gives zeros."""
    from fractions import Fraction
    records = np.asarray(records, BODY_DTYPE).reshape(-1)
    n = len(records)
    mass, com, inertia = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3, 3))
    size = Fraction(voxel_size)
    pairs = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 2): 4, (0, 2): 5}   # m2's order: xx, yy, zz, xy, yz, zx
    for i, r in enumerate(records):
        m = int(r["mass"])
        if m == 0:
            continue
        m1 = [int(v) for v in r["m1"]]
        m2 = [int(v) for v in r["m2"]]
        c = {ab: Fraction(m2[k]) - Fraction(m1[ab[0]] * m1[ab[1]], m) for ab, k in pairs.items()}
        mass[i] = float(m)
        for a in range(3):
            com[i, a] = float((Fraction(m1[a], m) + Fraction(1, 2)) * size)
            others = [b for b in range(3) if b != a]
            inertia[i, a, a] = float((c[(others[0], others[0])] + c[(others[1], others[1])] + Fraction(m, 6)) * size * size)
        for a, b in ((0, 1), (1, 2), (0, 2)):
            inertia[i, a, b] = inertia[i, b, a] = float(-c[(a, b)] * size * size)
    return mass, com, inertia


def joint_properties(records, voxel_size=1.0):
    """Host only: Model.joints' records -> (area, anchor, normal): area (n,) faces * voxel_size^2; anchor (n, 3) the centroid of the
    face centres, sum2 / (2 faces) * voxel_size; normal (n, 3) the unnormalised area vector pointing from a to b, (by_face[+x] -
    by_face[-x], ...) * voxel_size^2. Computed in exact rational arithmetic and rounded once to float64."""
    from fractions import Fraction
    records = np.asarray(records, JOINT_DTYPE).reshape(-1)
    n = len(records)
    area, anchor, normal = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    size = Fraction(voxel_size)
    for i, r in enumerate(records):
        faces = int(r["faces"])
        if faces == 0:
            continue
        area[i] = float(faces * size * size)
        for k in range(3):
            anchor[i, k] = float(Fraction(int(r["sum2"][k]), 2 * faces) * size)
            normal[i, k] = float((int(r["by_face"][2 * k + 1]) - int(r["by_face"][2 * k])) * size * size)
    return area, anchor, normal


def box_bounds(boxes):
    """Host only: the inclusive voxel bounds of Model.boxes' records -> (lo, hi) int32 (N, 3)."""
    boxes = np.asarray(boxes, BOX_DTYPE).reshape(-1)
    key = boxes["key"].astype(np.int32)
    lo = np.stack([key >> 16, (key >> 8) & 255, key & 255], axis=1).astype(np.int32)
    hi = lo + np.stack([boxes["dx"], boxes["dy"], boxes["dz"]], axis=1).astype(np.int32)
    return lo, hi


def box_shapes(boxes, op=L.EDIT_PLACE, palette=None):
    """Host only: Model.boxes' records as EDIT_SHAPE_DTYPE BOX records for Model.edit_shapes: a the lowest corner, b the lowest corner
    plus the extents, so that the centres of exactly the box's voxels lie inside; palette the record's own unless one is given.
    Placing a model's boxes into an empty model of the same palette gives the model's voxels back. A call takes at most
    L.MAX_EDIT_SHAPES shapes: callers chunk."""
    boxes = np.asarray(boxes, BOX_DTYPE).reshape(-1)
    lo, hi = box_bounds(boxes)
    return edit_shapes(L.SHAPE_BOX, lo, hi + 1, op=op, palette=boxes["palette"].astype(np.int32) if palette is None else palette)


def top_level_build(boxes):
    """Host only: the grid and the slot order dust_hip_scene_commit builds over instance world boxes (n x 6: lo, hi) ->
    dict(dim, lo, cell, cells, items, ranges, slot_order, n_groups). For tests and tools."""
    lib = L.load()
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    n = len(b)
    info = L.TopLevelInfo()
    info.struct_size = C.sizeof(L.TopLevelInfo)
    fp = b.ctypes.data_as(C.POINTER(C.c_float))
    L.check(lib.dust_hip_top_level_build(fp, n, C.byref(info), None, 0, None, 0, None, None))
    cells, items = np.zeros(info.n_cells, np.uint32), np.zeros(max(1, info.n_items), np.uint16)
    ranges, order = np.zeros((n, 2), np.uint32), np.zeros(n, np.uint32)
    L.check(lib.dust_hip_top_level_build(fp, n, C.byref(info), cells.ctypes.data_as(C.POINTER(C.c_uint32)), len(cells),
                                     items.ctypes.data_as(C.POINTER(C.c_uint16)), len(items), ranges.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     order.ctypes.data_as(C.POINTER(C.c_uint32))))
    return {"dim": tuple(info.dim), "lo": np.array(info.lo[:], np.float32), "cell": np.array(info.cell[:], np.float32), "cells": cells,
            "items": items[:info.n_items], "ranges": ranges, "slot_order": order, "n_groups": info.n_groups}


def sky_struct(sky):
    """56 baked sky floats -> DustHipSky"""
    s = L.Sky()
    s.state[:] = np.asarray(sky, np.float32).reshape(56).tolist()
    return s


def _config_from_environment():
    """the production knobs of DustHipPipelineConfig as A/B scripts and the stress drivers spell them (read HERE, not by the library)"""
    import os
    e, cfg = os.environ, {}
    if "DUST_HIP_RAY_STREAM" in e:
        cfg["gi_path"] = "streams"
    elif "DUST_HIP_PACKET_GI" in e:
        cfg["gi_path"] = "packets"
    if "DUST_HIP_NO_SIDE_STREAM" in e:
        cfg["side_stream"] = "off"
    if e.get("DUST_HIP_SIDE_SHARE") and int(e["DUST_HIP_SIDE_SHARE"]) > 0:   # (0: calibrated, the default)
        cfg["side_share"] = min(90, max(5, int(e["DUST_HIP_SIDE_SHARE"])))
    if e.get("DUST_HIP_RESERVE_BLOCKS"):
        cfg["reserve_blocks"] = int(e["DUST_HIP_RESERVE_BLOCKS"])
    return cfg


class StandardPipeline:
    """StandardPipeline (crates/render/src/pipeline/standard.rs:51-60, :222-240) + its GBuffer (:881-917)."""

    PRIMARY_RAYTYPE = 0
    AMBIENT_OCCLUSION_RAYTYPE = 1
    FINAL_GATHER_RAYTYPE = 2
    SURFEL_RAYTYPE = 3

    def __init__(self, ctx, width, height, **config):
        """config: DustHipPipelineConfig fields (see configure). A/B runs and the stress drivers may also name them in the environment
        of THIS shim -- DUST_HIP_RAY_STREAM / DUST_HIP_PACKET_GI (gi_path), DUST_HIP_NO_SIDE_STREAM, DUST_HIP_SIDE_SHARE,
        DUST_HIP_RESERVE_BLOCKS --: the library itself reads no production knob from the environment."""
        self._ctx = ctx
        self._lib = ctx._lib
        self.width, self.height = width, height
        self._h = C.c_void_p()
        L.check(self._lib.dust_hip_pipeline_create(ctx._h, width, height, C.byref(self._h)))
        cfg = _config_from_environment()
        cfg.update(config)
        if cfg:
            self.configure(**cfg)

    def configure(self, reserve_blocks=None, gi_path=None, side_stream=None, side_share=None, frames_in_flight=None, in_flight_slots=None):
        """dust_hip_pipeline_configure: the fields given replace the pipeline's current ones.
        gi_path: "auto" | "packets" | "streams"; side_stream: "auto" | "off"; in_flight_slots: "share" | "all"; reserve_blocks: int or "auto"."""
        c = self.get_config(raw=True)
        if reserve_blocks is not None:
            c.reserve_blocks = L.RESERVE_AUTO if reserve_blocks == "auto" else int(reserve_blocks)
        if gi_path is not None:
            c.gi_path = {"auto": L.GI_PATH_AUTO, "packets": L.GI_PATH_PACKETS, "streams": L.GI_PATH_STREAMS}.get(gi_path, gi_path)
        if side_stream is not None:
            c.side_stream = {"auto": L.SIDE_STREAM_AUTO, "off": L.SIDE_STREAM_OFF}.get(side_stream, side_stream)
        if side_share is not None:
            c.side_share = int(side_share)
        if in_flight_slots is not None:
            c.in_flight_slots = {"share": L.IN_FLIGHT_SHARE, "all": L.IN_FLIGHT_ALL}.get(in_flight_slots, in_flight_slots)
        c.frames_in_flight = int(frames_in_flight) if frames_in_flight is not None else 0
        L.check(self._lib.dust_hip_pipeline_configure(self._h, C.byref(c)))

    def get_config(self, raw=False):
        c = L.PipelineConfig(C.sizeof(L.PipelineConfig))
        L.check(self._lib.dust_hip_pipeline_get_config(self._h, C.byref(c)))
        if raw:
            return c
        return {"reserve_blocks": "auto" if c.reserve_blocks == L.RESERVE_AUTO else c.reserve_blocks,
                "gi_path": ("auto", "packets", "streams")[c.gi_path], "side_stream": ("auto", "off")[c.side_stream], "side_share": c.side_share,
                "frames_in_flight": c.frames_in_flight, "in_flight_slots": ("share", "all")[c.in_flight_slots]}

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_hip_pipeline_destroy(self._h)
            self._h = None

    def set_noise(self, texture, texels):
        t = np.ascontiguousarray(texels, np.uint8)
        layers = t.size // (128 * 128 * (1 if texture == 0 else 4))
        L.check(self._lib.dust_hip_pipeline_set_noise(self._h, texture, _ptr(t), layers))

    def render(self, scene, camera, sky, passes, frame_index=1, rand=0, rows=(0, 0), surfel_shard=(0, 0)):
        """sky: 56 floats, or a DustHipSky made once with api.sky_struct() (a frame loop: the conversion is most of this call's host time).
        surfel_shard: (rank, world) -- with PASS_SURFEL | PASS_GI_SHARDED the pass only traces rank's share of the ordered pool (Comm.gi_surfel_exchange completes it)"""
        self.frame_call(scene, camera, sky, passes, frame_index, rand, rows, surfel_shard)()

    def frame_call(self, scene, camera, sky, passes, frame_index=1, rand=0, rows=(0, 0), surfel_shard=(0, 0)):
        """-> a callable that makes ONE dust_hip_render_frame call with the arguments marshalled HERE (a frame loop that knows its frames ahead builds
        the calls first: what is left per call is the C entry point -- a band-sized step of an N-GPU job is 30 us, of which render()'s marshalling was a third)"""
        s = sky if isinstance(sky, L.Sky) else sky_struct(sky)
        fp = L.FrameParams(C.sizeof(L.FrameParams), passes, frame_index, rand & 0xFFFFFFFF, rows[0], rows[1], surfel_shard[0], surfel_shard[1])
        fn, h, sh, cam_ref, sky_ref, fp_ref, check = self._lib.dust_hip_render_frame, self._h, scene._h, C.byref(camera), C.byref(s), C.byref(fp), L.check

        def call(_keep=(self, scene, camera, s, fp)):
            check(fn(h, sh, cam_ref, sky_ref, fp_ref))
        return call

    @staticmethod
    def render_frames(pipes, scene, cameras, skies, passes, frame_indices, rands, rows=(0, 0), moves=None):
        """frames_call(...)(): see there"""
        StandardPipeline.frames_call(pipes, scene, cameras, skies, passes, frame_indices, rands, rows, moves)()

    @staticmethod
    def frames_call(pipes, scene, cameras, skies, passes, frame_indices, rands, rows=(0, 0), moves=None):
        """-> a callable that makes ONE dust_hip_render_frames call with the arguments marshalled HERE (a frame loop that knows its frames ahead -- an
        offline render, bench.py's timed region -- builds the calls first: what is left per call is the C entry point).
        dust_hip_render_frames: frame i -- cameras[i], skies[i], frame_indices[i], rands[i] -- into pipes[i], the results of len(pipes)
        render() calls in that order; primary + AO frames of distinct pipelines of one context share ONE persistent launch (up to 8 frames each).
        cameras / skies: one per frame, or a single Camera / Sky for all of them. moves: per frame None or a list of (instance id, obj_to_world[12],
        prev_obj_to_world mat4[16] or None): what Scene.set_transform + Scene.commit would do before that frame."""
        n = len(pipes)
        # (a frame loop hands over ctypes arrays it made once -- at least n entries each: building them is most of this call's host time)
        if isinstance(cameras, C.Array) and getattr(cameras, "_type_", None) is L.Camera:
            cams = cameras
        else:
            cams = (L.Camera * n)(*[(cameras if isinstance(cameras, L.Camera) else cameras[i]) for i in range(n)])
        if isinstance(skies, C.Array) and getattr(skies, "_type_", None) is L.Sky:
            sk = skies
        else:
            one_sky = isinstance(skies, L.Sky) or (not isinstance(skies, (list, tuple)))
            sk = (L.Sky * n)(*[((skies if isinstance(skies, L.Sky) else sky_struct(skies)) if one_sky else
                                (skies[i] if isinstance(skies[i], L.Sky) else sky_struct(skies[i]))) for i in range(n)])
        assert len(cams) >= n and len(sk) >= n
        fps = (L.FrameParams * n)(*[L.FrameParams(C.sizeof(L.FrameParams), passes, int(frame_indices[i]), int(rands[i]) & 0xFFFFFFFF, rows[0], rows[1], 0, 0)
                                    for i in range(n)])
        hs = (C.c_void_p * n)(*[p._h for p in pipes])
        mv, keep = None, []
        if moves is not None:
            mv = (L.FrameMoves * n)()
            for i in range(n):
                ms = moves[i] or []
                if not ms:
                    continue
                ids = np.ascontiguousarray([m[0] for m in ms], np.uint32)
                xf = np.ascontiguousarray([np.asarray(m[1], np.float32).reshape(12) for m in ms], np.float32)
                have_prev = all(len(m) > 2 and m[2] is not None for m in ms)
                pv = np.ascontiguousarray([np.asarray(m[2], np.float32).reshape(16) for m in ms], np.float32) if have_prev else None
                keep += [ids, xf, pv]
                mv[i].n = len(ms)
                mv[i].instance_ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
                mv[i].obj_to_world = xf.ctypes.data_as(C.POINTER(C.c_float))
                mv[i].prev_obj_to_world = pv.ctypes.data_as(C.POINTER(C.c_float)) if pv is not None else None
        fn, sh, check = pipes[0]._lib.dust_hip_render_frames, scene._h, L.check

        def call(_keep=(keep, pipes, scene)):   # (the arrays above stay alive with the closure)
            check(fn(n, hs, sh, cams, sk, fps, mv))
        return call

    def pass_stats(self, index):
        st = L.PassStats()
        L.check(self._lib.dust_hip_pipeline_pass_stats(self._h, index, C.byref(st)))
        return st

    def read_plane(self, plane):
        dt, ch = PLANE_DTYPES[plane]
        shape = (self.height, self.width, ch) if ch > 1 else (self.height, self.width)
        out = np.zeros(shape, dt)
        L.check(self._lib.dust_hip_pipeline_read_plane(self._h, plane, _ptr(out), out.nbytes))
        return out

    def kernel_times(self, mark=True):
        """(ms_sum[4], launches[4]) per pass kind (primary/fused, AO, final gather, surfel pass) since the last mark"""
        ms, n = (C.c_float * 4)(), (C.c_uint32 * 4)()
        L.check(self._lib.dust_hip_pipeline_kernel_times(self._h, 1 if mark else 0, ms, n))
        return list(ms), list(n)

    def mark_kernel_times(self):
        """start of a timed region: later kernel_times() calls sum the launches from here on (no wait, nothing read back)"""
        L.check(self._lib.dust_hip_pipeline_kernel_times(self._h, 1, None, None))

    def tile_costs(self, pass_kind=0):
        """cycles per tile of the pass's last launch, shape (tiles_y, tiles_x); None before the first launch"""
        tx, ty = C.c_uint32(), C.c_uint32()
        L.check(self._lib.dust_hip_pipeline_tile_costs(self._h, pass_kind, None, 0, C.byref(tx), C.byref(ty)))
        if tx.value == 0:
            return None
        out = np.zeros((ty.value, tx.value), np.uint32)
        L.check(self._lib.dust_hip_pipeline_tile_costs(self._h, pass_kind, _ptr(out), out.size, C.byref(tx), C.byref(ty)))
        return out

    def plane_device_ptr(self, plane):
        p, n = C.c_void_p(), C.c_size_t()
        L.check(self._lib.dust_hip_pipeline_plane_device_ptr(self._h, plane, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bind_plane(self, plane, device_ptr, nbytes):
        """Redirect a plane to caller-owned device memory (device_ptr = 0 / None: back to the pipeline's own storage)."""
        L.check(self._lib.dust_hip_pipeline_bind_plane(self._h, plane, C.c_void_p(device_ptr or None), nbytes))

    def clear(self):
        L.check(self._lib.dust_hip_pipeline_clear(self._h))

    def set_frames_in_flight(self, n):
        """the caller keeps n frames in flight on this device (a pipeline and a context each): launches take 1/n of the workgroup slots"""
        L.check(self._lib.dust_hip_pipeline_set_frames_in_flight(self._h, n))

    def set_denoiser(self, max_accumulated_frames=30, disocclusion_threshold=0.01, antilag_sigma_scale=2.0, antilag_power=0.8,
                     max_blur_radius=15.0):
        """ReblurSettings (nrd.rs:768-785) for DUST_PASS_DENOISE"""
        dp = L.DenoiseParams(C.sizeof(L.DenoiseParams), max_accumulated_frames, disocclusion_threshold, antilag_sigma_scale,
                             antilag_power, max_blur_radius)
        L.check(self._lib.dust_hip_pipeline_set_denoiser(self._h, C.byref(dp)))

    def restart_denoiser(self):
        """DenoiserEvent::Restart"""
        L.check(self._lib.dust_hip_pipeline_restart_denoiser(self._h))

    def tone_map(self, transfer_function=1, conversion=None, min_log=-6.0, max_log=8.5, time_coefficient=0.2):
        """AutoExposurePipeline + ToneMappingPipeline on the denoised plane -> PLANE_OUTPUT."""
        tp = L.ToneMapParams()
        tp.struct_size = C.sizeof(L.ToneMapParams)
        tp.transfer_function = transfer_function
        tp.color_space_conversion[:] = (color_space_conversion() if conversion is None else np.asarray(conversion, np.float32)).tolist()
        tp.min_log_luminance, tp.max_log_luminance, tp.time_coefficient = min_log, max_log, time_coefficient
        L.check(self._lib.dust_hip_tone_map(self._h, C.byref(tp)))

    def exposure(self, set_to=None):
        out = C.c_float()
        s = None if set_to is None else C.byref(C.c_float(set_to))
        L.check(self._lib.dust_hip_pipeline_exposure(self._h, C.byref(out), s))
        return out.value

    def configure_gi(self, hash_capacity=32 * 1024 * 1024, surfel_pool_size=720 * 480):
        self._gi = (hash_capacity, surfel_pool_size)
        L.check(self._lib.dust_hip_pipeline_configure_gi(self._h, hash_capacity, surfel_pool_size))

    def gi_exchange(self, padded_rows=None):
        """Device buffers of the multi-GPU GI exchange (dust_hip.h): a _lib.GiExchange with raw device pointers."""
        out = L.GiExchange()
        out.struct_size = C.sizeof(L.GiExchange)
        L.check(self._lib.dust_hip_pipeline_gi_exchange(self._h, padded_rows or self.height, C.byref(out)))
        self._gi = (self._gi[0] if getattr(self, "_gi", None) else 32 * 1024 * 1024, out.pool_size)
        return out

    def gi_export(self, row_begin, row_end):
        L.check(self._lib.dust_hip_gi_export(self._h, row_begin, row_end))

    def gi_import(self, row_begin, row_end, frame_index):
        L.check(self._lib.dust_hip_gi_import(self._h, row_begin, row_end, frame_index))

    def gi_surfel_finish(self, frame_index):
        """completes a sharded surfel trace WITHOUT an exchange (dust_hip_gi_surfel_exchange_run with no communicator): a world of one, or
        one emulated rank of N -- the other ranks' records are whatever the staging arrays hold"""
        L.check(self._lib.dust_hip_gi_surfel_exchange_run(self._h, None, frame_index))

    def read_gi(self):
        """(hash entries as uint32[capacity+2, 3], surfel pool as structured array)"""
        cap, pool = getattr(self, "_gi", None) or (32 * 1024 * 1024, 720 * 480)  # the defaults of an implicit configuration
        h = np.zeros((cap + 2, 3), np.uint32)
        L.check(self._lib.dust_hip_pipeline_read_gi(self._h, 0, _ptr(h), h.nbytes))
        s = np.zeros(pool, SURFEL_DTYPE)
        L.check(self._lib.dust_hip_pipeline_read_gi(self._h, 1, _ptr(s), s.nbytes))
        return h, s


def _write_gi(self, hash_entries, pool):
    """Restore a state saved with read_gi() into a pipeline configured with the same capacity and pool size."""
    h = np.ascontiguousarray(hash_entries, np.uint32)
    s = np.ascontiguousarray(pool, SURFEL_DTYPE)
    L.check(self._lib.dust_hip_pipeline_write_gi(self._h, 0, _ptr(h), h.nbytes))
    L.check(self._lib.dust_hip_pipeline_write_gi(self._h, 1, _ptr(s), s.nbytes))


StandardPipeline.write_gi = _write_gi


class Comm:
    """One rank's end of the multi-GPU partition: an RCCL communicator on the context's device (create), or the ranks of a loopback
    group on one device (local). Band gather and GI exchange run inside the library (comm.hip)."""

    def __init__(self, ctx, handle):
        self._ctx, self._lib, self._h = ctx, ctx._lib, handle

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        L.check(L.load().dust_hip_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    @classmethod
    def create(cls, ctx, rank, world, unique_id: bytes):
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        L.check(ctx._lib.dust_hip_comm_create(ctx._h, rank, world, C.cast(buf, C.c_void_p), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def local(cls, ctx, world):
        hs = (C.c_void_p * world)()
        L.check(ctx._lib.dust_hip_comm_create_local(ctx._h, world, hs))
        return [cls(ctx, C.c_void_p(h)) for h in hs]

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.dust_hip_comm_destroy(self._h)
            self._h = None

    def info(self):
        r, w, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
        L.check(self._lib.dust_hip_comm_info(self._h, C.byref(r), C.byref(w), C.byref(l)))
        return r.value, w.value, bool(l.value)

    def _cuts(self, cuts):
        """world + 1 row indices as the C array the library reads cuts[0..world] of (a shorter list would be an out-of-bounds host read)"""
        world = self.info()[1]
        if len(cuts) != world + 1:
            raise ValueError(f"band cuts: {len(cuts)} entries for a communicator of {world} ranks (want world + 1)")
        return cuts if isinstance(cuts, C.Array) else (C.c_uint32 * len(cuts))(*[int(v) for v in cuts])

    def gather_bands(self, pipe, plane, cuts, root=0, dst_ptr=None, dst_bytes=0):
        """-> the gather's ticket (wait(ticket) before its source target or destination is used again)"""
        c = self._cuts(cuts)
        t = C.c_uint64()
        L.check(self._lib.dust_hip_gather_bands(pipe._h, self._h, plane, c, root, C.c_void_p(dst_ptr) if dst_ptr else None, dst_bytes, C.byref(t)))
        return t.value

    def gather_planes(self, pipe, planes, cuts, root=0):
        """several planes (an iterable of DUST_PLANE_* indices) in one collective, each into the root pipeline's own plane -> ticket"""
        c = self._cuts(cuts)
        mask = 0
        for pl in planes:
            mask |= 1 << int(pl)
        t = C.c_uint64()
        L.check(self._lib.dust_hip_gather_planes(pipe._h, self._h, mask, c, root, C.byref(t)))
        return t.value

    def gi_exchange(self, pipe, row_begin, row_end, band_rows, frame_index):
        L.check(self._lib.dust_hip_gi_exchange_run(pipe._h, self._h, row_begin, row_end, band_rows, frame_index))

    def gi_surfel_exchange(self, pipe, frame_index):
        """completes a surfel pass whose trace was sharded (render(..., surfel_shard=(rank, world))): all-gather of the records, stamps, ordered apply"""
        L.check(self._lib.dust_hip_gi_surfel_exchange_run(pipe._h, self._h, frame_index))

    def wait(self, ticket=0):
        L.check(self._lib.dust_hip_comm_wait(self._h, ticket))

    def sync(self):
        L.check(self._lib.dust_hip_comm_sync(self._h))


def load_png_array(data: bytes):
    """PNG / APNG -> array (layers, height, width, channels), uint8 (big-endian uint16 for 16-bit files): the reference's
    PngLoader (rhyolite_bevy/src/loaders/png.rs:70-200). RGB comes back as RGBA with a zero fourth channel."""
    lib = L.load()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    info = L.PngInfo()
    out = C.POINTER(C.c_uint8)()
    L.check(lib.dust_png_load_array(C.cast(buf, C.c_void_p), len(data), C.byref(info), C.byref(out)))
    try:
        n = info.layers * info.height * info.width * info.channels * info.bytes_per_channel
        raw = np.ctypeslib.as_array(out, shape=(n,)).copy()
    finally:
        lib.dust_vox_free(out)
    dt = np.uint8 if info.bytes_per_channel == 1 else np.dtype(">u2")
    return raw.view(dt).reshape(info.layers, info.height, info.width, info.channels)

