"""ctypes binding of libdust_hip.so -- the C ABI declared in include/dust_hip.h.

The library is the product; there is no Python or CPU fallback behind it. If the shared object is
missing the import raises, and every device entry point fails with DUST_ERR_NO_DEVICE when no GPU is
visible.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DUST_HIP_LIB selects another build of the SAME library (tools/kernel_sections.py uses its -DDUST_PROFILE build)
LIB_PATH = os.environ.get("DUST_HIP_LIB") or os.path.join(_HERE, "libdust_hip.so")

OK = 0
ERR_INVALID_ARGUMENT = -1
ERR_NO_DEVICE = -2
ERR_HIP = -3
ERR_OUT_OF_MEMORY = -4
ERR_PARSE = -5
ERR_UNSUPPORTED = -6
ERR_NOT_READY = -7

PASS_PRIMARY = 1 << 0
PASS_AMBIENT_OCCLUSION = 1 << 1
PASS_FINAL_GATHER = 1 << 2
PASS_SURFEL = 1 << 3
PASS_ACCUMULATE = 1 << 4
PASS_DENOISE = 1 << 5
PASS_COUNT_STATS = 1 << 16
PASS_GI_ORDERED = 1 << 17
PASS_GI_SHARDED = 1 << 18
GI_PATH_AUTO, GI_PATH_PACKETS, GI_PATH_STREAMS = 0, 1, 2
SIDE_STREAM_AUTO, SIDE_STREAM_OFF = 0, 1
IN_FLIGHT_SHARE, IN_FLIGHT_ALL = 0, 1
RESERVE_AUTO = 0xFFFFFFFF
CONTEXT_TIMING = 1
CONTEXT_TIMING_SPARSE = 2

PLANE_ILLUMINANCE, PLANE_DENOISED, PLANE_ALBEDO, PLANE_NORMAL, PLANE_DEPTH, PLANE_MOTION, PLANE_VOXEL_ID, PLANE_ACCUM, PLANE_OUTPUT = range(9)
PLANE_BYTES_PER_PIXEL = (8, 8, 4, 4, 4, 8, 4, 16, 8)


class Block(C.Structure):  # DustHipBlock, 24 bytes
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("z", C.c_uint16), ("w", C.c_uint16),
                ("mask", C.c_uint64), ("material_ptr", C.c_uint32), ("avg_albedo", C.c_uint32)]


class VoxModelInfo(C.Structure):
    _fields_ = [("size", C.c_uint32 * 3), ("n_voxels", C.c_uint32), ("n_blocks", C.c_uint32),
                ("n_materials", C.c_uint64), ("used", C.c_uint32)]


class PngInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("layers", C.c_uint32), ("channels", C.c_uint32),
                ("bytes_per_channel", C.c_uint32)]


class VoxInstance(C.Structure):
    _fields_ = [("model", C.c_uint32), ("obj_to_world", C.c_float * 12)]


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("stream", C.c_void_p),
                ("lds_root_bytes", C.c_uint32), ("flags", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("view_col0", C.c_float * 3), ("view_col1", C.c_float * 3), ("view_col2", C.c_float * 3),
                ("position", C.c_float * 3), ("tan_half_fov", C.c_float), ("far_", C.c_float), ("near_", C.c_float)]


class TopLevelInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("dim", C.c_uint32 * 3), ("lo", C.c_float * 3), ("cell", C.c_float * 3),
                ("n_cells", C.c_uint32), ("n_items", C.c_uint32), ("n_groups", C.c_uint32)]


class Sky(C.Structure):
    _fields_ = [("state", C.c_float * 56)]


class FrameParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("passes", C.c_uint32), ("frame_index", C.c_uint32),
                ("rand", C.c_uint32), ("row_begin", C.c_uint32), ("row_end", C.c_uint32), ("surfel_rank", C.c_uint32), ("surfel_world", C.c_uint32)]


class FrameMoves(C.Structure):   # DustHipFrameMoves: the instances moved before a frame of dust_hip_render_frames
    _fields_ = [("n", C.c_uint32), ("instance_ids", C.POINTER(C.c_uint32)), ("obj_to_world", C.POINTER(C.c_float)), ("prev_obj_to_world", C.POINTER(C.c_float))]


class ToneMapParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("transfer_function", C.c_uint32), ("color_space_conversion", C.c_float * 9),
                ("min_log_luminance", C.c_float), ("max_log_luminance", C.c_float), ("time_coefficient", C.c_float)]


class DenoiseParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_accumulated_frames", C.c_uint32), ("disocclusion_threshold", C.c_float),
                ("antilag_sigma_scale", C.c_float), ("antilag_power", C.c_float), ("max_blur_radius", C.c_float)]


class PipelineConfig(C.Structure):  # DustHipPipelineConfig
    _fields_ = [("struct_size", C.c_uint32), ("reserve_blocks", C.c_uint32), ("gi_path", C.c_uint32), ("side_stream", C.c_uint32),
                ("side_share", C.c_uint32), ("frames_in_flight", C.c_uint32), ("in_flight_slots", C.c_uint32)]


class GiExchange(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pool_size", C.c_uint32), ("width", C.c_uint32), ("touched_rows", C.c_uint32),
                ("slot_owner", C.c_void_p), ("touched", C.c_void_p), ("merged", C.c_void_p)]


class Ray(C.Structure):       # DustHipRay, 32 bytes: a scene query's ray (world space; t in units of |direction|)
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RayHit(C.Structure):    # DustHipRayHit, 32 bytes: instance == NO_HIT on a miss
    _fields_ = [("t", C.c_float), ("instance", C.c_uint32), ("block", C.c_uint32), ("voxel", C.c_uint32), ("xyz", C.c_uint32 * 3),
                ("face", C.c_uint8), ("palette", C.c_uint8), ("reserved", C.c_uint16)]


NO_HIT = 0xFFFFFFFF
QUERY_ANY_HIT = 1


class BoxQuery(C.Structure):  # DustHipBoxQuery, 32 bytes: a world-space box and its slice [first, first + capacity) of the records
    _fields_ = [("lo", C.c_float * 3), ("first", C.c_uint32), ("hi", C.c_float * 3), ("capacity", C.c_uint32)]


class VoxelRef(C.Structure):  # DustHipVoxelRef, 16 bytes: one solid voxel inside a box
    _fields_ = [("instance", C.c_uint32), ("block", C.c_uint32), ("xyz", C.c_uint16 * 3), ("palette", C.c_uint8), ("voxel", C.c_uint8)]


class BoxSweep(C.Structure):  # DustHipBoxSweep, 48 bytes: a world-space box at t = 0 and its displacement over t in [0, 1]
    _fields_ = [("lo", C.c_float * 3), ("reserved0", C.c_uint32), ("hi", C.c_float * 3), ("reserved1", C.c_uint32),
                ("delta", C.c_float * 3), ("reserved2", C.c_uint32)]


class SweepHit(C.Structure):  # DustHipSweepHit, 32 bytes: the first voxel a sweep touches
    _fields_ = [("t", C.c_float), ("instance", C.c_uint32), ("block", C.c_uint32), ("xyz", C.c_uint16 * 3), ("palette", C.c_uint8),
                ("voxel", C.c_uint8), ("normal", C.c_float * 3)]


SWEEP_IGNORE_START = 2


class EditShape(C.Structure):  # DustHipEditShape, 48 bytes: a box, sphere or capsule in a model's tree coordinates and what it does to the voxels it covers
    _fields_ = [("a", C.c_float * 3), ("kind", C.c_uint32), ("b", C.c_float * 3), ("radius", C.c_float),
                ("op", C.c_uint32), ("palette", C.c_int32), ("reserved", C.c_uint32 * 2)]


SHAPE_BOX, SHAPE_SPHERE, SHAPE_CAPSULE = 0, 1, 2
EDIT_CARVE, EDIT_FILL, EDIT_PAINT, EDIT_PLACE = 0, 1, 2, 3
MAX_EDIT_SHAPES = 65536


class IslandQuery(C.Structure):  # DustHipIslandQuery, 32 bytes: the connectivity of a labelling and the inclusive voxel box that anchors islands
    _fields_ = [("struct_size", C.c_uint32), ("connectivity", C.c_uint32), ("anchor_lo", C.c_uint32 * 3), ("anchor_hi", C.c_uint32 * 3)]


class Island(C.Structure):  # DustHipIsland, 40 bytes: one connected set of solid voxels, named by its smallest x << 16 | y << 8 | z
    _fields_ = [("key", C.c_uint32), ("voxels", C.c_uint32), ("lo", C.c_uint8 * 3), ("flags", C.c_uint8), ("hi", C.c_uint8 * 3),
                ("reserved", C.c_uint8), ("sum", C.c_uint64 * 3)]


ISLANDS_FACES, ISLANDS_CORNERS = 0, 1
ISLAND_ANCHORED = 1
NO_ISLAND = 0xFFFFFFFF
DETACH_KEEP_SOURCE = 1


class Stamp(C.Structure):  # DustHipStamp, 32 bytes: a sub-box of a source model, a signed axis permutation and where its image lands in the destination
    _fields_ = [("offset", C.c_int32 * 3), ("orient", C.c_uint32), ("op", C.c_uint32), ("src_lo", C.c_uint8 * 3), ("pad0", C.c_uint8),
                ("src_hi", C.c_uint8 * 3), ("pad1", C.c_uint8), ("reserved", C.c_uint32)]


STAMP_PLACE, STAMP_OVERWRITE, STAMP_REPLACE, STAMP_CARVE, STAMP_PAINT = 0, 1, 2, 3, 4
MAX_STAMPS = 65536


class Resample(C.Structure):  # DustHipResample, 96 bytes: the fixed-point inverse map, the destination box, the source sub-box and the stamp op
    _fields_ = [("m", (C.c_int32 * 3) * 3), ("t", C.c_int32 * 3), ("dst_lo", C.c_int32 * 3), ("dst_hi", C.c_int32 * 3), ("src_lo", C.c_uint8 * 3),
                ("pad0", C.c_uint8), ("src_hi", C.c_uint8 * 3), ("pad1", C.c_uint8), ("op", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class ResampleCount(C.Structure):  # DustHipResampleCount, 16 bytes
    _fields_ = [("changed", C.c_uint32), ("covered", C.c_uint32), ("solid", C.c_uint32), ("blocked", C.c_uint32)]


RESAMPLE_ONE = 65536
RESAMPLE_MAX_M = 8 * 65536
RESAMPLE_MAX_T = 1 << 28
RESAMPLE_DRY_RUN = 1
MAX_RESAMPLES = 65536


class Cast(C.Structure):  # DustHipCast, 48 bytes: a sub-box of a source model, its orientation and offset in the destination, a step and a step limit
    _fields_ = [("offset", C.c_int32 * 3), ("orient", C.c_uint32), ("step", C.c_int32 * 3), ("max_steps", C.c_uint32), ("flags", C.c_uint32),
                ("src_lo", C.c_uint8 * 3), ("pad0", C.c_uint8), ("src_hi", C.c_uint8 * 3), ("pad1", C.c_uint8), ("reserved", C.c_uint32)]


class CastHit(C.Structure):  # DustHipCastHit, 32 bytes: the free steps of a cast and what it touches first
    _fields_ = [("steps", C.c_uint32), ("flags", C.c_uint32), ("contacts", C.c_uint32), ("voxels", C.c_uint32), ("contact", C.c_int32 * 3),
                ("src_key", C.c_uint32)]


CAST_WALLS = 1
CAST_HIT, CAST_OVERLAP, CAST_HIT_WALL = 1, 2, 4
CAST_MAX_STEPS = 65535
MAX_CASTS = 65536
CAST_NO_KEY = 0xFFFFFFFF


class FloodQuery(C.Structure):  # DustHipFloodQuery, 40 bytes: the medium a flood spreads through, its step limit and its inclusive region box
    _fields_ = [("struct_size", C.c_uint32), ("medium", C.c_uint32), ("palette", C.c_int32), ("max_steps", C.c_uint32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3)]


class FloodResult(C.Structure):  # DustHipFloodResult, 32 bytes: what a flood reached
    _fields_ = [("reached", C.c_uint32), ("farthest", C.c_uint32), ("seeds_used", C.c_uint32), ("boundary", C.c_uint32),
                ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8), ("hi", C.c_uint8 * 3), ("pad1", C.c_uint8), ("reserved", C.c_uint32 * 2)]


FLOOD_EMPTY, FLOOD_SOLID, FLOOD_MATERIAL = 0, 1, 2
FLOOD_UNREACHED = 0xFFFF
FLOOD_MAX_STEPS = 65534
MAX_FLOOD_SEEDS = 65536


class DistanceQuery(C.Structure):  # DustHipDistanceQuery, 32 bytes: the targets a distance field measures to, its metric and its radius
    _fields_ = [("struct_size", C.c_uint32), ("target", C.c_uint32), ("metric", C.c_uint32), ("flags", C.c_uint32),
                ("palette", C.c_int32), ("max_radius", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class DistanceResult(C.Structure):  # DustHipDistanceResult, 32 bytes: the counts of a distance field and where its largest value is
    _fields_ = [("targets", C.c_uint32), ("near", C.c_uint32), ("far", C.c_uint32), ("largest", C.c_uint32),
                ("largest_key", C.c_uint32), ("reserved", C.c_uint32 * 3)]


DISTANCE_TO_SOLID, DISTANCE_TO_EMPTY, DISTANCE_TO_MATERIAL = 0, 1, 2
DISTANCE_EUCLIDEAN, DISTANCE_CHEBYSHEV = 0, 1
DISTANCE_WALLS = 1
DISTANCE_FAR = 0xFFFF
DISTANCE_MAX_RADIUS = 255
DISTANCE_NO_KEY = 0xFFFFFFFF


class Reduce(C.Structure):  # DustHipReduce, 16 bytes: how many times a model is halved and how many solid children make a coarse voxel solid
    _fields_ = [("struct_size", C.c_uint32), ("levels", C.c_uint32), ("min_solid", C.c_uint32), ("flags", C.c_uint32)]


class ReduceResult(C.Structure):  # DustHipReduceResult, 16 bytes: the solid voxels of the source and of its reduction, and the reduction's extent
    _fields_ = [("src_voxels", C.c_uint32), ("voxels", C.c_uint32), ("extent", C.c_uint32), ("reserved", C.c_uint32)]


REDUCE_MAX_LEVELS = 8


class Census(C.Structure):  # DustHipCensus, 40 bytes: what the voxels a shape covers hold -- counts, the bounds and the coordinate sums of the solid ones
    _fields_ = [("covered", C.c_uint32), ("solid", C.c_uint32), ("lo", C.c_uint8 * 3), ("reserved0", C.c_uint8), ("hi", C.c_uint8 * 3),
                ("reserved1", C.c_uint8), ("sum", C.c_uint64 * 3)]


MAX_CENSUS_SHAPES = 65536
MAX_CENSUS_TABLES = 4096
CENSUS_BINS = 256


class SurfaceQuery(C.Structure):  # DustHipSurfaceQuery, 48 bytes: the directions that count, the palette filter and the inclusive region box
    _fields_ = [("struct_size", C.c_uint32), ("faces", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


class SurfaceResult(C.Structure):  # DustHipSurfaceResult, 64 bytes: listed voxels, their exposed faces (in all, per direction), solid voxels, bounds
    _fields_ = [("voxels", C.c_uint32), ("faces", C.c_uint32), ("by_face", C.c_uint32 * 6), ("solid", C.c_uint32),
                ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8), ("hi", C.c_uint8 * 3), ("pad1", C.c_uint8), ("reserved", C.c_uint32 * 5)]


class SurfaceVoxel(C.Structure):  # DustHipSurfaceVoxel, 8 bytes: a listed voxel's key, its exposed faces and its palette index
    _fields_ = [("key", C.c_uint32), ("faces", C.c_uint8), ("palette", C.c_uint8), ("reserved", C.c_uint16)]


FACE_NEG_X, FACE_POS_X, FACE_NEG_Y, FACE_POS_Y, FACE_NEG_Z, FACE_POS_Z = 1, 2, 4, 8, 16, 32
FACES_ALL = 63
SURFACE_WALLS = 1
SURFACE_BINS = 256


class MeshQuery(C.Structure):  # DustHipMeshQuery, 48 bytes: field for field a SurfaceQuery; flags MESH_WALLS | MESH_ANY_PALETTE
    _fields_ = [("struct_size", C.c_uint32), ("faces", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


class MeshQuad(C.Structure):  # DustHipMeshQuad, 8 bytes: the key of the quad's lowest corner voxel, its direction index, palette index and extents - 1
    _fields_ = [("key", C.c_uint32), ("face", C.c_uint8), ("palette", C.c_uint8), ("du", C.c_uint8), ("dv", C.c_uint8)]


class MeshResult(C.Structure):  # DustHipMeshResult, 64 bytes: quads and their area, in all and per direction, the largest quad's area
    _fields_ = [("quads", C.c_uint32), ("faces", C.c_uint32), ("quads_by_face", C.c_uint32 * 6), ("faces_by_face", C.c_uint32 * 6),
                ("largest", C.c_uint32), ("reserved", C.c_uint32)]


MESH_WALLS = 1
MESH_ANY_PALETTE = 2


class BoxesQuery(C.Structure):  # DustHipBoxesQuery, 48 bytes: a SurfaceQuery's layout with the stacking axis where its faces stand; flags BOXES_ANY_PALETTE
    _fields_ = [("struct_size", C.c_uint32), ("axis", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


class Box(C.Structure):  # DustHipBox, 8 bytes: the key of the box's lowest corner voxel, its palette index and its extents - 1 along x, y, z
    _fields_ = [("key", C.c_uint32), ("palette", C.c_uint8), ("dx", C.c_uint8), ("dy", C.c_uint8), ("dz", C.c_uint8)]


class BoxesResult(C.Structure):  # DustHipBoxesResult, 64 bytes: boxes, the rects of all slices, the voxels they hold, their bounds
    _fields_ = [("boxes", C.c_uint32), ("rects", C.c_uint32), ("voxels", C.c_uint32), ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8),
                ("hi", C.c_uint8 * 3), ("pad1", C.c_uint8), ("reserved", C.c_uint32 * 11)]


BOXES_ANY_PALETTE = 1


class DeltaQuery(C.Structure):  # DustHipDeltaQuery, 48 bytes: a SurfaceQuery's layout with the kinds that count where its faces stand
    _fields_ = [("struct_size", C.c_uint32), ("kinds", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


class DeltaResult(C.Structure):  # DustHipDeltaResult, 64 bytes: listed voxels, in all and per kind, both models' solid voxels, the listed voxels' bounds
    _fields_ = [("voxels", C.c_uint32), ("added", C.c_uint32), ("removed", C.c_uint32), ("repainted", C.c_uint32), ("solid_before", C.c_uint32),
                ("solid_after", C.c_uint32), ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8), ("hi", C.c_uint8 * 3), ("pad1", C.c_uint8),
                ("reserved", C.c_uint32 * 8)]


class DeltaVoxel(C.Structure):  # DustHipDeltaVoxel, 8 bytes: a voxel's key, the kind of its change, its value before and after (DELTA_NONE: no voxel)
    _fields_ = [("key", C.c_uint32), ("kind", C.c_uint8), ("before", C.c_uint8), ("after", C.c_uint8), ("reserved", C.c_uint8)]


DELTA_ADDED, DELTA_REMOVED, DELTA_REPAINTED = 1, 2, 4
DELTA_ALL = 7
DELTA_NONE = 255
DELTA_BACKWARD = 1
DELTA_BINS = 256
MAX_DELTA_RECORDS = 1 << 24


class ColumnsQuery(C.Structure):  # DustHipColumnsQuery, 48 bytes: a SurfaceQuery's layout with the one side looked from where its faces stand, and the layer
    _fields_ = [("struct_size", C.c_uint32), ("face", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("layer", C.c_uint32), ("reserved", C.c_uint32)]


class ColumnsResult(C.Structure):  # DustHipColumnsResult, 64 bytes: columns, those with the layer, their runs' voxels, every run, depths, the two keys, bounds
    _fields_ = [("columns", C.c_uint32), ("hit", C.c_uint32), ("voxels", C.c_uint32), ("runs", C.c_uint32), ("depth_sum", C.c_uint32),
                ("nearest_key", C.c_uint32), ("farthest_key", C.c_uint32), ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8), ("hi", C.c_uint8 * 3),
                ("pad1", C.c_uint8), ("reserved", C.c_uint32 * 7)]


class ColumnCell(C.Structure):  # DustHipColumnCell, 4 bytes: where a column's run starts, the palette index there (255: a miss), its length - 1, the column's runs
    _fields_ = [("at", C.c_uint8), ("palette", C.c_uint8), ("length_minus_1", C.c_uint8), ("runs", C.c_uint8)]


COLUMNS_RUN, COLUMNS_GAP = 0, 1
COLUMNS_BINS = 256
COLUMNS_NO_KEY = 0xFFFFFFFF


class NeighboursQuery(C.Structure):  # DustHipNeighboursQuery, 48 bytes: a SurfaceQuery's layout with the neighbourhood where its faces stand, and the two masks
    _fields_ = [("struct_size", C.c_uint32), ("neighbourhood", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("birth", C.c_uint32), ("survive", C.c_uint32)]


class NeighboursResult(C.Structure):  # DustHipNeighboursResult, 64 bytes: the region's voxels, the solid ones, what one generation would do, its bounds
    _fields_ = [("voxels", C.c_uint32), ("solid", C.c_uint32), ("born", C.c_uint32), ("died", C.c_uint32), ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8),
                ("hi", C.c_uint8 * 3), ("pad1", C.c_uint8), ("reserved", C.c_uint32 * 10)]


class NeighboursApplied(C.Structure):  # DustHipNeighboursApplied, 64 bytes: the generations that changed something, solid before and after, the sums, the bounds
    _fields_ = [("generations", C.c_uint32), ("solid_before", C.c_uint32), ("solid_after", C.c_uint32), ("reserved0", C.c_uint32),
                ("born", C.c_uint64), ("died", C.c_uint64), ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8), ("hi", C.c_uint8 * 3), ("pad1", C.c_uint8),
                ("reserved", C.c_uint32 * 6)]


NEIGHBOURS_FACES, NEIGHBOURS_EDGES, NEIGHBOURS_CORNERS = 6, 18, 26
NEIGHBOURS_WALLS, NEIGHBOURS_MAJORITY = 1, 2
NEIGHBOURS_BINS = 27
NEIGHBOURS_MAX_GENERATIONS = 256


class SettleQuery(C.Structure):  # DustHipSettleQuery, 72 bytes: the side things fall toward, the region, and the palette indices that are loose as 256 bits
    _fields_ = [("struct_size", C.c_uint32), ("toward", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("loose", C.c_uint32 * 8)]


class SettleResult(C.Structure):  # DustHipSettleResult, 64 bytes: what one fall would do
    _fields_ = [("columns", C.c_uint32), ("loose", C.c_uint32), ("fixed", C.c_uint32), ("moved", C.c_uint32), ("changed", C.c_uint32), ("fall_max", C.c_uint32),
                ("fall_sum", C.c_uint64), ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8), ("hi", C.c_uint8 * 3), ("pad1", C.c_uint8), ("changed_columns", C.c_uint32),
                ("reserved", C.c_uint32 * 5)]


class SettleApplied(C.Structure):  # DustHipSettleApplied, 64 bytes: the generations that moved something, the sums over the slides and the falls, the bounds
    _fields_ = [("generations", C.c_uint32), ("first_moved", C.c_uint32), ("loose", C.c_uint32), ("reserved0", C.c_uint32), ("slid", C.c_uint64),
                ("fell", C.c_uint64), ("fall_sum", C.c_uint64), ("lo", C.c_uint8 * 3), ("pad0", C.c_uint8), ("hi", C.c_uint8 * 3), ("pad1", C.c_uint8),
                ("reserved", C.c_uint32 * 4)]


SETTLE_MAX_GENERATIONS = 256


class Triangle(C.Structure):  # DustHipTriangle, 48 bytes: three integer vertices in 1/256 voxel of a model's tree coordinates and what the triangle does to the voxels it touches
    _fields_ = [("v", (C.c_int32 * 3) * 3), ("op", C.c_uint32), ("palette", C.c_int32), ("reserved", C.c_uint32)]


class FillMeshQuery(C.Structure):  # DustHipFillMeshQuery, 48 bytes: what the voxels inside a mesh take, and the region
    _fields_ = [("struct_size", C.c_uint32), ("op", C.c_uint32), ("palette", C.c_int32), ("flags", C.c_uint32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


class FillMeshResult(C.Structure):  # DustHipFillMeshResult, 48 bytes: the inside voxels of the region, those that changed, the triangles that counted, the bounds
    _fields_ = [("covered", C.c_uint32), ("changed", C.c_uint32), ("live", C.c_uint32), ("crossing", C.c_uint32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


TRIANGLE_UNIT = 256
TRIANGLE_MAX_COORD = 262144
MAX_EDIT_TRIANGLES = 65536
MAX_MESH_TRIANGLES = 1 << 20


class FractureSeed(C.Structure):  # DustHipFractureSeed, 16 bytes: a seed point in voxel coordinates, -1024..1279 per axis
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("z", C.c_int32), ("reserved", C.c_uint32)]


class FractureQuery(C.Structure):  # DustHipFractureQuery, 48 bytes: the filter, the distance limit, the per-axis scales and the region of a fracture
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32), ("max_distance2", C.c_uint32),
                ("scale", C.c_uint8 * 3), ("reserved0", C.c_uint8), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class FractureResult(C.Structure):  # DustHipFractureResult, 64 bytes: the counted and labelled voxels, the cells, the cut faces, the bounds
    _fields_ = [("solid", C.c_uint32), ("labelled", C.c_uint32), ("cells", C.c_uint32), ("largest_cell", C.c_uint32), ("largest_voxels", C.c_uint32),
                ("cut_faces", C.c_uint32), ("max_d2", C.c_uint32), ("lo", C.c_uint8 * 3), ("reserved0", C.c_uint8), ("hi", C.c_uint8 * 3),
                ("reserved1", C.c_uint8), ("reserved", C.c_uint32 * 7)]


class FractureCell(C.Structure):  # DustHipFractureCell, 40 bytes, laid out like DustHipCensus: one cell's voxels, shared faces, bounds and coordinate sums
    _fields_ = [("voxels", C.c_uint32), ("cut_faces", C.c_uint32), ("lo", C.c_uint8 * 3), ("reserved0", C.c_uint8), ("hi", C.c_uint8 * 3),
                ("reserved1", C.c_uint8), ("sum", C.c_uint64 * 3)]


MAX_FRACTURE_SEEDS = 4096
FRACTURE_SEED_MIN, FRACTURE_SEED_MAX = -1024, 1279
FRACTURE_MAX_SCALE = 16
FRACTURE_NO_LIMIT = 0xFFFFFFFF
NO_CELL = 0xFFFF
FRACTURE_SEAMS, FRACTURE_LABELLED = 0, 1


class BodyQuery(C.Structure):  # DustHipBodyQuery, 48 bytes: a SurfaceQuery's layout with the kind of group where its faces stand
    _fields_ = [("struct_size", C.c_uint32), ("group", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


class Body(C.Structure):  # DustHipBody, 96 bytes: a group's key, counted voxels and bounds; the sums of w, of w x, y, z and of w xx, yy, zz, xy, yz, zx
    _fields_ = [("key", C.c_uint32), ("voxels", C.c_uint32), ("lo", C.c_uint8 * 3), ("reserved0", C.c_uint8), ("hi", C.c_uint8 * 3),
                ("reserved1", C.c_uint8), ("mass", C.c_uint64), ("m1", C.c_uint64 * 3), ("m2", C.c_uint64 * 6)]


BODIES_ALL, BODIES_MATERIALS, BODIES_ISLANDS, BODIES_CELLS = 0, 1, 2, 3
BODY_WEIGHTS = 255


class JointQuery(C.Structure):  # DustHipJointQuery, 48 bytes: a SurfaceQuery's layout with the kind of group where its faces stand
    _fields_ = [("struct_size", C.c_uint32), ("group", C.c_uint32), ("flags", C.c_uint32), ("palette", C.c_int32),
                ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


class Joint(C.Structure):  # DustHipJoint, 80 bytes: the two groups, the faces they share, by direction from a to b, the bounds and sums of the face centres in half voxels
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("faces", C.c_uint32), ("reserved0", C.c_uint32), ("by_face", C.c_uint32 * 6),
                ("lo2", C.c_uint16 * 3), ("hi2", C.c_uint16 * 3), ("reserved1", C.c_uint32), ("sum2", C.c_uint64 * 3)]


JOINTS_MATERIALS, JOINTS_CELLS = 0, 1
JOINT_REST = 0xFFFF


class HierarchyInfo(C.Structure):  # DustHipHierarchyInfo, 48 bytes: what dust_hip_model_read_hierarchy reports besides the arrays
    _fields_ = [("struct_size", C.c_uint32), ("extent_log2", C.c_uint32), ("n_mid", C.c_uint32), ("n_l2", C.c_uint32),
                ("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("reserved", C.c_uint32 * 2)]


N16_BYTES, N16_ROOT_BYTES = 656, 640


class PassStats(C.Structure):
    _fields_ = [("ms", C.c_float), ("rays", C.c_uint64), ("instances_tested", C.c_uint64),
                ("upper_descents", C.c_uint64), ("mid_descents", C.c_uint64), ("bricks_tested", C.c_uint64),
                ("hits", C.c_uint64)]


# every symbol include/dust_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)
_f32p = C.POINTER(C.c_float)
SYMBOLS = {
    "dust_hip_last_error": (C.c_char_p, []),
    "dust_hip_device_count": (C.c_int, []),
    "dust_vdb_tree_create": (C.c_int, [_u32p, C.c_uint32, C.POINTER(_P)]),
    "dust_vdb_tree_destroy": (None, [_P]),
    "dust_vdb_tree_set": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32]),
    "dust_vdb_tree_get": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]),
    "dust_vdb_tree_iter": (C.c_int, [_P, _u32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dust_vdb_tree_iter_leaf": (C.c_int, [_P, _u32p, _u64p, _u32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dust_vdb_tree_meta": (C.c_int, [_P, _u32p, _u32p]),
    "dust_vdb_lca_level": (C.c_uint32, [_u32p, _u32p, C.c_uint32, C.c_uint32]),
    "dust_vdb_accessor_create": (C.c_int, [_P, C.POINTER(_P)]),
    "dust_vdb_accessor_destroy": (None, [_P]),
    "dust_vdb_accessor_get": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]),
    "dust_vdb_pool_create": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_P)]),
    "dust_vdb_pool_destroy": (None, [_P]),
    "dust_vdb_pool_alloc": (C.c_uint32, [_P]),
    "dust_vdb_pool_free": (None, [_P, C.c_uint32]),
    "dust_vdb_pool_num_chunks": (C.c_size_t, [_P]),
    "dust_vdb_bitmask_set": (None, [_u64p, C.c_size_t, C.c_int32]),
    "dust_vdb_bitmask_iter_set_bits": (C.c_size_t, [_u64p, C.c_size_t, _u32p, C.c_size_t]),
    "dust_vox_load": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "dust_vox_load_frame": (C.c_int, [_P, C.c_size_t, C.c_uint32, C.POINTER(_P)]),
    "dust_vox_scene_destroy": (None, [_P]),
    "dust_vox_scene_counts": (C.c_int, [_P, _u32p, _u32p]),
    "dust_vox_scene_model_info": (C.c_int, [_P, C.c_uint32, C.POINTER(VoxModelInfo)]),
    "dust_vox_scene_model_data": (C.c_int, [_P, C.c_uint32, C.POINTER(C.POINTER(Block)), C.POINTER(_u8p)]),
    "dust_vox_scene_palette": (C.c_int, [_P, C.POINTER(_u8p)]),
    "dust_vox_scene_instances": (C.c_int, [_P, C.POINTER(VoxInstance), C.c_uint32]),
    "dust_vox_flatten_model": (C.c_int, [_P, C.c_size_t, _u32p, _P, C.POINTER(C.POINTER(Block)), _u32p,
                                         C.POINTER(_u8p), _u64p]),
    "dust_vox_free": (None, [_P]),
    "dust_png_load_array": (C.c_int, [_P, C.c_size_t, C.POINTER(PngInfo), C.POINTER(_u8p)]),
    "dust_sky_dataset_create": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(_P)]),
    "dust_sky_dataset_destroy": (None, [_P]),
    "dust_sky_bake": (C.c_int, [_P, C.c_float, _f32p, _f32p, C.POINTER(Sky)]),
    "dust_hip_context_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "dust_hip_context_destroy": (None, [_P]),
    "dust_hip_sync": (C.c_int, [_P]),
    "dust_hip_model_create": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, _P, C.c_uint32, C.POINTER(_P)]),
    "dust_hip_model_destroy": (None, [_P]),
    "dust_hip_model_set_voxels": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "dust_hip_model_get_voxels": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "dust_hip_model_edit_shapes": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "dust_hip_model_find_islands": (C.c_int, [_P, _P, _u32p, _P, C.c_uint32]),
    "dust_hip_model_island_of": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "dust_hip_model_detach_islands": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "dust_hip_model_stamp": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P]),
    "dust_hip_model_resample": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, _P]),
    "dust_hip_model_cast": (C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    "dust_hip_model_flood": (C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    "dust_hip_model_flood_at": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "dust_hip_model_flood_paths": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    "dust_hip_model_flood_apply": (C.c_int, [_P, C.c_uint32, C.c_int32, _u32p]),
    "dust_hip_model_distance": (C.c_int, [_P, _P, _P]),
    "dust_hip_model_distance_at": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "dust_hip_model_distance_apply": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int32, _u32p]),
    "dust_hip_model_reduce": (C.c_int, [_P, _P, C.POINTER(_P), _P]),
    "dust_hip_model_census": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "dust_hip_model_surface": (C.c_int, [_P, _P, _P, _P, C.c_uint32, _P]),
    "dust_hip_model_surface_apply": (C.c_int, [_P, _P, C.c_int32, _u32p]),
    "dust_hip_model_mesh": (C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    "dust_hip_model_boxes": (C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    "dust_hip_model_delta": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P]),
    "dust_hip_model_delta_apply": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _u32p, _u32p]),
    "dust_hip_model_columns": (C.c_int, [_P, _P, _P, _P, C.c_uint32, _P]),
    "dust_hip_model_columns_apply": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int32, _u32p]),
    "dust_hip_model_neighbours": (C.c_int, [_P, _P, _P, _P]),
    "dust_hip_model_neighbours_apply": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "dust_hip_model_settle": (C.c_int, [_P, _P, _P]),
    "dust_hip_model_settle_apply": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "dust_hip_model_edit_triangles": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "dust_hip_model_fill_mesh": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "dust_hip_model_fracture": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P]),
    "dust_hip_model_fracture_at": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "dust_hip_model_fracture_detach": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "dust_hip_model_fracture_apply": (C.c_int, [_P, C.c_uint32, C.c_int32, _u32p]),
    "dust_hip_model_bodies": (C.c_int, [_P, _P, _P, _u32p, _P, C.c_uint32]),
    "dust_hip_model_joints": (C.c_int, [_P, _P, _u32p, _P, C.c_uint32]),
    "dust_hip_model_info": (C.c_int, [_P, _u32p, _u64p]),
    "dust_hip_model_read": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64]),
    "dust_hip_model_read_hierarchy": (C.c_int, [_P, C.POINTER(HierarchyInfo), _P, C.c_uint32, _P, C.c_uint64, _P, _P, _P, C.c_uint32, _P, C.c_uint64]),
    "dust_hip_scene_create": (C.c_int, [_P, C.POINTER(_P)]),
    "dust_hip_scene_destroy": (None, [_P]),
    "dust_hip_scene_add_instance": (C.c_int, [_P, _P, _f32p, _f32p, _u32p]),
    "dust_hip_scene_set_transform": (C.c_int, [_P, C.c_uint32, _f32p, _f32p]),
    "dust_hip_scene_commit": (C.c_int, [_P]),
    "dust_hip_scene_trace_rays": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32]),
    "dust_hip_scene_trace_rays_async": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32]),
    "dust_hip_scene_overlap_boxes": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32]),
    "dust_hip_scene_overlap_boxes_async": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32]),
    "dust_hip_scene_sweep_boxes": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32]),
    "dust_hip_scene_sweep_boxes_async": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32]),
    "dust_hip_top_level_build": (C.c_int, [C.POINTER(C.c_float), C.c_uint32, _P, _u32p, C.c_size_t, C.POINTER(C.c_uint16), C.c_size_t, _u32p, _u32p]),
    "dust_hip_pipeline_create": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "dust_hip_pipeline_destroy": (None, [_P]),
    "dust_hip_pipeline_set_noise": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32]),
    "dust_hip_render_frame": (C.c_int, [_P, _P, C.POINTER(Camera), C.POINTER(Sky), C.POINTER(FrameParams)]),
    "dust_hip_render_frames": (C.c_int, [C.c_uint32, C.POINTER(C.c_void_p), _P, C.POINTER(Camera), C.POINTER(Sky), C.POINTER(FrameParams), C.POINTER(FrameMoves)]),
    "dust_hip_pipeline_pass_stats": (C.c_int, [_P, C.c_uint32, C.POINTER(PassStats)]),
    "dust_hip_pipeline_kernel_times": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "dust_hip_pipeline_tile_costs": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _u32p, _u32p]),
    "dust_hip_pipeline_plane_device_ptr": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "dust_hip_pipeline_bind_plane": (C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    "dust_hip_pipeline_read_plane": (C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    "dust_hip_pipeline_configure_gi": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "dust_hip_pipeline_read_gi": (C.c_int, [_P, C.c_uint32, _P, C.c_size_t]),
    "dust_hip_pipeline_write_gi": (C.c_int, [_P, C.c_uint32, _P, C.c_size_t]),
    "dust_hip_pipeline_gi_exchange": (C.c_int, [_P, C.c_uint32, C.POINTER(GiExchange)]),
    "dust_hip_gi_export": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "dust_hip_gi_import": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "dust_hip_tone_map": (C.c_int, [_P, C.POINTER(ToneMapParams)]),
    "dust_hip_pipeline_exposure": (C.c_int, [_P, _f32p, _f32p]),
    "dust_hip_pipeline_clear": (C.c_int, [_P]),
    "dust_hip_pipeline_set_frames_in_flight": (C.c_int, [_P, C.c_uint32]),
    "dust_hip_pipeline_configure": (C.c_int, [_P, C.POINTER(PipelineConfig)]),
    "dust_hip_pipeline_get_config": (C.c_int, [_P, C.POINTER(PipelineConfig)]),
    "dust_hip_pipeline_set_denoiser": (C.c_int, [_P, C.POINTER(DenoiseParams)]),
    "dust_hip_pipeline_restart_denoiser": (C.c_int, [_P]),
    "dust_hip_device_eval": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32]),
    # multi-GPU: RCCL communicator (or a loopback group on one device), band gather, GI exchange
    "dust_hip_comm_unique_id": (C.c_int, [_P]),
    "dust_hip_comm_create": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.POINTER(_P)]),
    "dust_hip_comm_create_local": (C.c_int, [_P, C.c_uint32, C.POINTER(_P)]),
    "dust_hip_comm_destroy": (None, [_P]),
    "dust_hip_comm_info": (C.c_int, [_P, _u32p, _u32p, _u32p]),
    "dust_hip_gather_bands": (C.c_int, [_P, _P, C.c_int, _u32p, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_uint64)]),
    "dust_hip_gather_planes": (C.c_int, [_P, _P, C.c_uint32, _u32p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "dust_hip_comm_wait": (C.c_int, [_P, C.c_uint64]),
    "dust_hip_comm_sync": (C.c_int, [_P]),
    "dust_hip_gi_exchange_run": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "dust_hip_gi_surfel_exchange_run": (C.c_int, [_P, _P, C.c_uint32]),
}

_lib = None


class DustError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"dust_hip status {status}: {message}")
        self.status = status


def load():
    """dlopen libdust_hip.so (built by dust_amd.build.build()); raises if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build the HIP extension first "
                          "(python -c 'import __graft_entry__ as g; g.build()'); there is no fallback path")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status):
    if status != OK:
        raise DustError(status, load().dust_hip_last_error().decode("utf-8", "replace"))
