/*
 * dust_hip.h -- C ABI of the MI355X-native replacement for Dust's ray-tracing hot path.
 *
 * Every entry point names the reference interface it stands in for (paths relative to the
 * dust-engine/dust checkout). Plain pointers and sizes only; no C++ or torch types cross this
 * boundary; no exception or panic crosses it either: every function returns a DustStatus and
 * dust_hip_last_error() holds the message of the calling thread's last failure.
 *
 * Ownership: handles are owned by the library and released by the matching *_destroy; input
 * arrays are borrowed for the duration of the call only (the library copies what it keeps).
 * Device-side handles (context, model, scene, pipeline) are reference-counted inside the library
 * the way the reference's are Arc / Handle<T> (Handle<VoxGeometry>, Arc<PipelineLayout> ...):
 * *_destroy gives up the caller's reference, and an object lives until its last user is gone, so
 * the destroy calls may come in ANY order (a garbage-collected host may finalise a context before
 * the models made from it).
 * Threading: a context and everything created from it is externally synchronised (one thread
 * at a time), matching the reference's single render system per frame (examples/castle.rs:139-236).
 */
#ifndef DUST_HIP_H
#define DUST_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum DustStatus {
  DUST_OK = 0,
  DUST_ERR_INVALID_ARGUMENT = -1,
  DUST_ERR_NO_DEVICE = -2,      /* no HIP device / HIP runtime failure at context creation */
  DUST_ERR_HIP = -3,            /* a HIP call or kernel launch failed; see dust_hip_last_error() */
  DUST_ERR_OUT_OF_MEMORY = -4,
  DUST_ERR_PARSE = -5,          /* VoxLoadingError::ParseError (crates/vox/src/loader.rs:311-317) */
  DUST_ERR_UNSUPPORTED = -6,    /* paths the reference leaves todo!() (node/internal.rs:121-124) / image kinds its loader rejects */
  DUST_ERR_NOT_READY = -7       /* StandardPipeline::render returning None (standard.rs:254-266) */
} DustStatus;

const char* dust_hip_last_error(void);
/* number of HIP devices visible; 0 when there is no GPU (never fails) */
int dust_hip_device_count(void);

/* ===================================================================== vdb tree builder (host)
 * Replaces dust_vdb::Tree<hierarchy!(...)> (crates/vdb/src/tree.rs:7-124) and Accessor
 * (accessor.rs:5-139). The hierarchy is given at run time as per-level fan-out log2s, root first:
 * hierarchy!(4,2,2) == {4,2,2}. */
typedef struct DustVdbTree DustVdbTree;
typedef struct DustVdbAccessor DustVdbAccessor;

DustStatus dust_vdb_tree_create(const uint32_t* fanout_log2, uint32_t n_levels, DustVdbTree** out); /* Tree::new, tree.rs:30-48 */
void dust_vdb_tree_destroy(DustVdbTree*);
/* Tree::set_value (tree.rs:83-85). value: 1 = Some(true), 0 = Some(false), -1 = None.
 * None returns DUST_ERR_UNSUPPORTED where the reference is todo!() (node/internal.rs:121-124). */
DustStatus dust_vdb_tree_set(DustVdbTree*, uint32_t x, uint32_t y, uint32_t z, int32_t value);
/* Tree::get_value (tree.rs:78-80). *value: 1 Some(true), 0 Some(false), -1 None */
DustStatus dust_vdb_tree_get(const DustVdbTree*, uint32_t x, uint32_t y, uint32_t z, int32_t* value);
/* Tree::iter (tree.rs:102-104): writes up to cap (x,y,z) triples in iteration order, *count = total */
DustStatus dust_vdb_tree_iter(const DustVdbTree*, uint32_t* xyz, size_t cap, size_t* count);
/* Tree::iter_leaf (tree.rs:106-113): leaf origins, 64-bit occupancy and material_ptr per leaf */
DustStatus dust_vdb_tree_iter_leaf(const DustVdbTree*, uint32_t* xyz, uint64_t* occupancy, uint32_t* material_ptr,
                                   size_t cap, size_t* count);
/* TreeMeta::META_MASK (tree.rs:154-167) and ROOT::LEVEL */
DustStatus dust_vdb_tree_meta(const DustVdbTree*, uint32_t* meta_mask, uint32_t* root_level);
/* lowest_common_ancestor_level (accessor.rs:15-30) */
uint32_t dust_vdb_lca_level(const uint32_t a[3], const uint32_t b[3], uint32_t meta_mask, uint32_t root_level);
/* Tree::accessor + Accessor::get (accessor.rs:37-57,125-131) */
DustStatus dust_vdb_accessor_create(const DustVdbTree*, DustVdbAccessor** out);
void dust_vdb_accessor_destroy(DustVdbAccessor*);
DustStatus dust_vdb_accessor_get(DustVdbAccessor*, uint32_t x, uint32_t y, uint32_t z, int32_t* value);

/* BitMask / Pool of crates/vdb (bitmask.rs:3-124, pool.rs:3-176), exposed for the reference's doctests */
typedef struct DustVdbPool DustVdbPool;
DustStatus dust_vdb_pool_create(size_t item_size, uint32_t chunk_size_log2, DustVdbPool** out); /* Pool::new */
void dust_vdb_pool_destroy(DustVdbPool*);
uint32_t dust_vdb_pool_alloc(DustVdbPool*);            /* Pool::alloc */
void dust_vdb_pool_free(DustVdbPool*, uint32_t index); /* Pool::free */
size_t dust_vdb_pool_num_chunks(const DustVdbPool*);   /* Pool::num_chunks */
/* BitMask::set / iter_set_bits over n_words 64-bit words */
void dust_vdb_bitmask_set(uint64_t* words, size_t index, int32_t value);
size_t dust_vdb_bitmask_iter_set_bits(const uint64_t* words, size_t n_words, uint32_t* out, size_t cap);

/* ===================================================================== .vox loader (host)
 * Replaces VoxLoader::load up to the point where it uploads (crates/vox/src/loader.rs:322-415):
 * file parse (dot_vox 5.1.1 in the reference), scene-graph walk (loader.rs:60-204), per-model
 * tree build + palette-index collector (loader.rs:238-288, collector.rs:2-88) and
 * VoxGeometry::from_tree (geometry.rs:55-179). */
typedef struct DustVoxScene DustVoxScene;

/* GPUVoxNode / shader `Block`, 24 bytes (geometry.rs:40-49, assets/shaders/headers/sbt.glsl:1-19) */
typedef struct DustHipBlock {
  uint16_t x, y, z, w;
  uint64_t mask;
  uint32_t material_ptr;
  uint32_t avg_albedo; /* R10 G10 B10 A2, sRGB-encoded */
} DustHipBlock;

typedef struct DustVoxModelInfo {
  uint32_t size[3]; /* model.size in file axes */
  uint32_t n_voxels;
  uint32_t n_blocks;      /* leaves of the tree == primitives of the reference BLAS */
  uint64_t n_materials;   /* bytes in the material buffer */
  uint32_t used;          /* referenced by at least one instance (loader.rs:360-372 only loads those) */
} DustVoxModelInfo;

typedef struct DustVoxInstance {
  uint32_t model;
  float obj_to_world[12]; /* 3x4 row-major, the TLAS instance transform (accel_struct/tlas.rs:99-105) */
} DustVoxInstance;

DustStatus dust_vox_load(const uint8_t* bytes, size_t n_bytes, DustVoxScene** out);
/* The same at animation frame `frame`. Where the reference stops at unimplemented!() -- transform nodes with several
 * frames (loader.rs:103-105) and shape nodes with several models (loader.rs:149-151), i.e. MagicaVoxel animations -- the
 * entry in force at `frame` is used: the one with the largest "_f" attribute <= frame, or the first one before the
 * animation starts. dust_vox_load is frame 0; files without animation give the same scene at every frame. */
DustStatus dust_vox_load_frame(const uint8_t* bytes, size_t n_bytes, uint32_t frame, DustVoxScene** out);
void dust_vox_scene_destroy(DustVoxScene*);
DustStatus dust_vox_scene_counts(const DustVoxScene*, uint32_t* n_models, uint32_t* n_instances);
DustStatus dust_vox_scene_model_info(const DustVoxScene*, uint32_t model, DustVoxModelInfo* out);
/* pointers stay valid until the scene is destroyed */
DustStatus dust_vox_scene_model_data(const DustVoxScene*, uint32_t model, const DustHipBlock** blocks,
                                     const uint8_t** materials);
DustStatus dust_vox_scene_palette(const DustVoxScene*, const uint8_t** rgba255x4); /* load_palette, loader.rs:208-236 */
DustStatus dust_vox_scene_instances(const DustVoxScene*, DustVoxInstance* out, uint32_t cap);

/* load_model + from_tree on caller-provided voxels (file axes, i = 0-based palette index).
 * Outputs are malloc'ed by the library; release with dust_vox_free(). */
DustStatus dust_vox_flatten_model(const uint8_t* xyzi, size_t n_voxels, const uint32_t size[3],
                                  const uint8_t* palette_rgba256, DustHipBlock** blocks, uint32_t* n_blocks,
                                  uint8_t** materials, uint64_t* n_materials);
void dust_vox_free(void*);

/* ---- PNG / APNG -> sliced image array ----
 * PngLoader::load (crates/rhyolite_bevy/src/loaders/png.rs:70-200), the loader behind the six spatiotemporal blue-noise
 * textures (crates/render/src/noise.rs:16-29, 128 x 128 x 64-frame APNGs): every animation frame becomes one layer;
 * grey and grey+alpha keep 1 / 2 channels, RGB is widened to RGBA with a zero fourth byte, 16-bit samples stay
 * big-endian. DUST_ERR_UNSUPPORTED for indexed colour, sub-byte samples, interlacing and partial frames.
 * The result feeds dust_hip_pipeline_set_noise directly (texture 0: 1 channel, texture 5: 4 channels). */
typedef struct DustPngInfo {
  uint32_t width, height, layers;
  uint32_t channels;           /* 1, 2 or 4 */
  uint32_t bytes_per_channel;  /* 1 or 2 */
} DustPngInfo;
DustStatus dust_png_load_array(const uint8_t* bytes, size_t n_bytes, DustPngInfo* info, uint8_t** texels /* dust_vox_free */);

/* ===================================================================== sky bake (host)
 * Sunlight::bake (crates/render/src/pipeline/sky.rs:90-268): Hosek-Wilkie sky + solar-disc state for a sun direction,
 * turbidity (1..10) and ground albedo -- the 56 floats DustHipSky carries to the shaders. The reference embeds the
 * model's tables with include_bytes! (sky.rs:34-63: dataset.bin, 1200 x vec3 = 14400 bytes; datasetSolar.bin,
 * 1806 x vec3 = 21672 bytes); this library does not contain them: the host passes the two files' bytes once.
 * (A host without the tables can use the pre-baked sweep under dust_amd/data/, see INTEGRATION.md.) */
typedef struct DustSkyDataset DustSkyDataset;
/* SkyModelState as Sunlight::bake() produces it, 56 floats (pipeline/sky.rs:66-132; layout.playout:35-51) */
typedef struct DustHipSky { float state[56]; } DustHipSky;
DustStatus dust_sky_dataset_create(const uint8_t* dataset_bin, size_t n_dataset, const uint8_t* dataset_solar_bin, size_t n_solar,
                                   DustSkyDataset** out);
void dust_sky_dataset_destroy(DustSkyDataset*);
/* direction: unit vector from eye to sun, y up, y > 0; albedo: ground albedo per XYZ channel (Sunlight::albedo) */
DustStatus dust_sky_bake(const DustSkyDataset*, float turbidity, const float albedo[3], const float direction[3], DustHipSky* out);

/* ===================================================================== device side
 * Replaces the Vulkan objects the render plugin owns (crates/render/src/lib.rs:58-134): device,
 * BLAS/TLAS stores, SBT, the four ray-tracing pipelines and their persistent buffers. */
typedef struct DustHipContext DustHipContext;
typedef struct DustHipModel DustHipModel;
typedef struct DustHipScene DustHipScene;
typedef struct DustHipPipeline DustHipPipeline;

typedef struct DustHipConfig {
  uint32_t struct_size;     /* sizeof(DustHipConfig) */
  int32_t device;           /* HIP device ordinal; -1 = current device */
  void* stream;             /* hipStream_t to launch on; NULL = a non-blocking stream owned by the context (note that the
                               legacy default stream IS the null handle: to share a stream with other code, create one) */
  uint32_t lds_root_bytes;  /* LDS budget for staged root nodes per workgroup; 0 = default (64 KiB) */
  uint32_t flags;           /* DUST_HIP_CONTEXT_* */
} DustHipConfig;
#define DUST_HIP_CONTEXT_TIMING 1u /* record hipEvents around every pass (dust_hip_pipeline_pass_stats) */
#define DUST_HIP_CONTEXT_TIMING_SPARSE 2u /* with TIMING: around the launches of every 4th frame only (dust_hip_pipeline_kernel_times then
                                             averages over those): an event record costs the stream ~6 us, 5 % of a 0.23 ms frame */

/* RenderPlugin::build -> device creation (crates/render/src/lib.rs:58-134) */
DustStatus dust_hip_context_create(const DustHipConfig*, DustHipContext** out);
void dust_hip_context_destroy(DustHipContext*);
DustStatus dust_hip_sync(DustHipContext*); /* waits for everything submitted on the context's stream */

/* Geometry + Material registration: VoxGeometry (AABB buffer + Block buffer, vox/src/geometry.rs:129-165),
 * PaletteMaterial parameters {geometry_ptr, material_ptr, palette_ptr} (vox/src/material.rs:30-41,106-119),
 * and the BLAS build (render/src/accel_struct/blas.rs:125-230), which here is the device-side VDB hierarchy.
 * tree_extent_log2: 8 for hierarchy!(4,2,2), 12 for (4,4,2,2). */
DustStatus dust_hip_model_create(DustHipContext*, const DustHipBlock* blocks, uint32_t n_blocks,
                                 const uint8_t* materials, uint64_t n_materials, const uint8_t* palette_rgba255x4,
                                 uint32_t tree_extent_log2, DustHipModel** out);
void dust_hip_model_destroy(DustHipModel*);
/* VoxGeometry::set / VoxGeometry::get (vox/src/geometry.rs:180-185; Tree::set_value / get_value, vdb/src/tree.rs:78-85) on the
 * DEVICE copy of a hierarchy (4,2,2) model. The reference's set only touches the CPU tree -- a loaded model's GPU buffers never
 * change -- so an edited voxel needs what that call does not carry, a material: values[i] >= 0 is Some(true) with palette
 * index values[i] (0..254), values[i] < 0 is None (the voxel is removed; the reference's todo!() for clearing through internal
 * nodes, node/internal.rs:121-124, does not apply: nothing is pointer-chased here). xyz: n coordinate triples in tree axes
 * (what Tree::set_value takes), < 256 each; a voxel named twice takes its last value. The first edit of a model moves it into
 * an editable form (a dense voxel grid on the device, ~44 MB); every batch then rewrites root, mid nodes, brick masks, Block
 * records (material_ptr, avg_albedo) and the material stream on the GPU with scans over the brick lattice -- afterwards the
 * device arrays are byte for byte what dust_hip_model_create builds from the same voxels (held by tests/test_gpu_edit.py and
 * its siblings for the Block records and the material stream, and by tests/test_gpu_hierarchy.py, through
 * dust_hip_model_read_hierarchy, for the root, the mid nodes, the dense masks, their count and the bounds). Asynchronous edits are not
 * offered: the call returns when the model is rebuilt (it reads sizes and bounds back). Scenes that instance the model must
 * be committed again (dust_hip_scene_commit) before they render: bounds and the staged root may have changed.
 * DUST_ERR_UNSUPPORTED for 4096^3 models. */
DustStatus dust_hip_model_set_voxels(DustHipModel*, const uint32_t* xyz, const int32_t* values, uint32_t n);
DustStatus dust_hip_model_get_voxels(DustHipModel*, const uint32_t* xyz, int32_t* values /* palette index, or -1 = None */, uint32_t n);
/* Shape edits: the edit the scene queries lead up to -- dig a crater where a picking ray hit, place a block, paint a region -- from a
 * description of the shape (48 bytes) instead of one set_voxels entry per voxel; the device decides which voxels the shape covers and
 * reports how many it changed (debris, resources, damage).
 *
 * Coordinates: the model's tree coordinates -- what set_voxels takes and DustHipRayHit.xyz / DustHipVoxelRef.xyz report. Voxel (x, y, z)
 * is the cube [x, x+1]^3; a shape covers a voxel when it contains the voxel's centre c = (x + 0.5, y + 0.5, z + 0.5) (exact in float32),
 * so a crater at a picked voxel has a = hit.xyz + 0.5. Shapes are clipped to the tree.
 * Membership is EXACT on float32: every -, *, +, / below is one float32 operation rounded to nearest (IEEE division, no contraction),
 * and dot(u, v) = ((u0*v0 + u1*v1) + u2*v2).
 *   BOX:      a[r] <= c[r] && c[r] <= b[r] on every axis (comparisons only; radius is ignored).
 *   SPHERE:   d = c - a; covered when dot(d, d) <= radius*radius (b is ignored).
 *   CAPSULE:  ab = b - a, ap = c - a, l = dot(ab, ab); h = (l == 0) ? 0 : min(max(dot(ap, ab) / l, 0), 1); q = ap - ab*h, per component
 *             one multiply and one subtract; covered when dot(q, q) <= radius*radius.
 * Shapes that cover nothing (changed[i] = 0, not an error, as the queries' degenerate inputs): a non-finite value in a field the kind
 * reads; a[r] > b[r] on a box; radius < 0 on a sphere or capsule; and, for spheres and capsules, any |coordinate| or radius above
 * 65 536 (every intermediate of the formulas stays finite, so they need no NaN rule). Boxes have no such limit: [-1e30, 1e30]^3 is
 * the whole model.
 * Operations on a covered voxel (values are a palette index or None): CARVE solid -> None; FILL every voxel -> palette; PAINT solid ->
 * palette, empty stays empty; PLACE empty -> palette, solid keeps its material.
 * Order: the shapes of a call apply in array order, as n successive calls would. changed[i] is the number of voxels whose value after
 * shape i differs from their value before it (a FILL that repaints a voxel in its own colour does not count; neither does a PLACE over
 * solid or a CARVE of nothing). Deterministic: two runs give the same bytes and the same counts. `changed` may be NULL.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything changes: a null model; null shapes with n > 0; n > DUST_HIP_MAX_EDIT_SHAPES; an
 * unknown kind or op; a palette outside 0..254 on an op that uses it. n == 0 is a no-op, whatever the arrays (as with set_voxels, it
 * may move the model into its editable form). DUST_ERR_UNSUPPORTED exactly where set_voxels returns it: 4096^3 trees, and models that
 * hold material byte 255.
 * Synchronous, like set_voxels: the call returns with the model rebuilt -- the device arrays byte for byte what dust_hip_model_create
 * builds from the same voxels -- and changed written. Scenes that instance the model must be committed again; until then frames and
 * queries answer DUST_ERR_NOT_READY, exactly as after set_voxels. A model is shared by its instances: an edit shows in all of them. */
#define DUST_HIP_SHAPE_BOX     0u
#define DUST_HIP_SHAPE_SPHERE  1u
#define DUST_HIP_SHAPE_CAPSULE 2u
#define DUST_HIP_EDIT_CARVE 0u   /* solid -> None                      (palette ignored) */
#define DUST_HIP_EDIT_FILL  1u   /* every voxel -> palette                               */
#define DUST_HIP_EDIT_PAINT 2u   /* solid -> palette, empty stays empty                  */
#define DUST_HIP_EDIT_PLACE 3u   /* empty -> palette, solid keeps its material           */
#define DUST_HIP_MAX_EDIT_SHAPES 65536u
typedef struct DustHipEditShape {   /* 48 bytes */
  float a[3]; uint32_t kind;        /* BOX: lo;  SPHERE: centre;  CAPSULE: segment start */
  float b[3]; float radius;         /* BOX: hi (radius ignored);  SPHERE: b ignored;  CAPSULE: segment end */
  uint32_t op; int32_t palette;     /* palette 0..254 for FILL / PAINT / PLACE */
  uint32_t reserved[2];             /* ignored */
} DustHipEditShape;
DustStatus dust_hip_model_edit_shapes(DustHipModel*, const DustHipEditShape* shapes, uint32_t n,
                                      uint32_t* changed /* n entries, may be NULL */);
/* Model islands: what a destructive edit leaves behind -- which solid voxels still hang together, which pieces were cut loose, and the
 * loose pieces as models of their own (debris that falls, a tower whose base was blown out).
 *
 * An island is a maximal set of solid voxels connected under the query's connectivity: DUST_HIP_ISLANDS_FACES joins voxels that share
 * a face (6 neighbours), DUST_HIP_ISLANDS_CORNERS voxels that share a face, an edge or a corner (26 neighbours). Coordinates are the
 * model's tree coordinates (what set_voxels takes). An island's name is its key: x << 16 | y << 8 | z of its voxel with the smallest
 * such value. DUST_HIP_NO_ISLAND (no voxel has that key) stands for "empty".
 *
 * dust_hip_model_find_islands labels the model and describes the islands. *n_islands is the total number of islands, whatever the
 * capacity; the first min(total, capacity) records are written in ascending key order and the slots past them are left untouched;
 * capacity == 0 (islands may then be NULL) only counts. Per record: key; voxels, the number of voxels; lo / hi, the inclusive bounds
 * of its voxels; flags, DUST_HIP_ISLAND_ANCHORED when at least one of its voxels lies in the query's anchor box and 0 otherwise;
 * reserved, 0; sum, the sums of x, of y and of z over its voxels (centre of mass = sum / voxels + 0.5). The anchor box is inclusive,
 * in voxels, and clipped to the tree; anchor_lo > anchor_hi on any axis anchors nothing. An empty model has 0 islands. Everything is
 * integer arithmetic: two runs give the same bytes.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything changes: a null model, query or n_islands; a struct_size below
 * sizeof(DustHipIslandQuery); a connectivity other than the two above; null islands with capacity > 0. DUST_ERR_UNSUPPORTED exactly
 * where set_voxels returns it (4096^3 trees, models that hold material byte 255) -- from all three calls, before they look at
 * coordinates, keys or the model's state.
 * Synchronous, like edit_shapes. A model that is not yet editable is moved into its editable form first, exactly as an n == 0 edit
 * does (scenes that instance it must then be committed again); on an editable model the call changes nothing a scene reads, and
 * committed scenes stay valid. The labelling stays on the device with the model -- per voxel, the key of its island: 64 MiB on top of
 * the editable form, allocated by the first call, released with the model -- and replaces the previous one, whatever its connectivity.
 * It is invalidated by every set_voxels or edit_shapes with n > 0 (whether or not a voxel changed), and by a find_islands that fails.
 * While it stands, a further find_islands with the same connectivity keeps it and only counts and describes the islands again (other
 * anchor box, other capacity): counting with capacity == 0 and then asking for every record labels once.
 *
 * dust_hip_model_island_of answers, per coordinate triple, the key of the voxel's island under the last labelling; an empty voxel
 * answers DUST_HIP_NO_ISLAND (a picking ray's hit.xyz names the island that was hit). Refused with DUST_ERR_INVALID_ARGUMENT: a null
 * model; null arrays with n > 0; a coordinate >= 256 (nothing is written then). DUST_ERR_NOT_READY when the model was never labelled
 * or its labelling was invalidated, also with n == 0.
 *
 * dust_hip_model_detach_islands moves the union of the named islands out of the model. keys are keys of the CURRENT labelling;
 * duplicates are allowed. Checked in this order, before anything changes: DUST_ERR_INVALID_ARGUMENT for a null model, null keys with
 * n > 0, flags other than DUST_HIP_DETACH_KEEP_SOURCE, or DUST_HIP_DETACH_KEEP_SOURCE with out == NULL; n == 0 is a no-op in every
 * state (*out, if given, is set to NULL); DUST_ERR_NOT_READY without a valid labelling; DUST_ERR_INVALID_ARGUMENT when some key does
 * not name an island (the key of an empty voxel, of a voxel that is not its island's smallest, of an island detached earlier, or a
 * value >= 1 << 24). On any refusal or failure *out is left as it was. The new model is built before the source is carved, so a
 * failure up to there leaves the source as it was too; a device failure while the carved source is rebuilt leaves the source as a
 * failed edit does (not to be used further) and invalidates its labelling, and the new model is not delivered.
 * out != NULL: *out is a new model on the same context holding exactly the named islands' voxels, at the same tree coordinates, with
 * the source's palette and their materials -- an instance added with the source's transform shows the pieces where they were. Its
 * arrays are byte for byte what dust_hip_model_create builds from those voxels. It is born in editable form, at the editable form's
 * memory cost (~44 MB, as a model after its first edit), unlabelled, and is the caller's to destroy.
 * Without DUST_HIP_DETACH_KEEP_SOURCE the voxels are carved from the source: it is rebuilt as after an edit, and scenes that instance
 * it must be committed again. With out == NULL that simply deletes the islands (debris clean-up). With DUST_HIP_DETACH_KEEP_SOURCE
 * the source is not touched at all: committed scenes stay valid.
 * Removing whole islands leaves every other island as it was, so the source's labelling STAYS VALID: the removed voxels answer
 * DUST_HIP_NO_ISLAND, the removed keys are refused from then on, and the remaining keys can be detached by later calls without
 * labelling again (every floating piece into a model of its own after one find_islands). Synchronous. */
#define DUST_HIP_ISLANDS_FACES   0u   /* 6-connectivity: voxels sharing a face */
#define DUST_HIP_ISLANDS_CORNERS 1u   /* 26-connectivity: sharing a face, an edge or a corner */
#define DUST_HIP_ISLAND_ANCHORED 1u   /* DustHipIsland.flags */
#define DUST_HIP_NO_ISLAND 0xFFFFFFFFu
typedef struct DustHipIslandQuery {   /* 32 bytes */
  uint32_t struct_size, connectivity;
  uint32_t anchor_lo[3], anchor_hi[3]; /* inclusive voxel box in tree coordinates, clipped to the tree; lo > hi on any axis: nothing is anchored */
} DustHipIslandQuery;
typedef struct DustHipIsland {        /* 40 bytes */
  uint32_t key;                       /* x << 16 | y << 8 | z of the island's voxel with the smallest such value: its name */
  uint32_t voxels;
  uint8_t lo[3], flags;               /* inclusive bounds; DUST_HIP_ISLAND_ANCHORED: some voxel lies in the anchor box */
  uint8_t hi[3], reserved;            /* 0 */
  uint64_t sum[3];                    /* sum of x, of y, of z over its voxels: centre of mass = sum / voxels + 0.5 */
} DustHipIsland;
DustStatus dust_hip_model_find_islands(DustHipModel*, const DustHipIslandQuery*, uint32_t* n_islands,
                                       DustHipIsland* islands, uint32_t capacity);
DustStatus dust_hip_model_island_of(DustHipModel*, const uint32_t* xyz, uint32_t* keys, uint32_t n);
#define DUST_HIP_DETACH_KEEP_SOURCE 1u /* copy the islands into *out and leave the source as it is */
DustStatus dust_hip_model_detach_islands(DustHipModel*, const uint32_t* keys, uint32_t n, uint32_t flags,
                                         DustHipModel** out /* may be NULL */);
/* Model stamps: the constructive edit, and the inverse of detach_islands -- the voxels of one model pasted into another, rotated or
 * mirrored, materials and all: a prefab (a tree, a wall segment, a door frame), a detached island that has come to rest, a copy of a
 * region of the same model. edit_shapes writes one palette index per shape; a stamp carries a textured piece.
 *
 * Geometry: everything is integer, in the two models' tree coordinates (what set_voxels takes). A stamp names an inclusive sub-box
 * [src_lo, src_hi] of the source, a signed axis permutation and where the image lands. p[r] = (orient >> 2r) & 3 is the source axis
 * that destination axis r reads, g[r] = (orient >> (6 + r)) & 1 whether it runs backwards, for r = 0, 1, 2: {p[0], p[1], p[2]} must be
 * a permutation of {0, 1, 2} and bits 9 and above must be 0 -- 48 orientations, the 24 mirrored ones included; orient == 0x24 is the
 * identity. With e[k] = src_hi[k] - src_lo[k], the image box is offset[r] .. offset[r] + e[p[r]] on destination axis r. A destination
 * voxel d that lies in the image box and inside the tree reads source voxel s: with u[r] = d[r] - offset[r],
 *   s[p[r]] = src_lo[p[r]] + u[r]   when g[r] == 0,        s[p[r]] = src_hi[p[r]] - u[r]   when g[r] == 1.
 * Any int32 offset is legal (nothing overflows); the image is clipped to the tree, and an image entirely outside it changes nothing.
 * src_lo > src_hi on any axis covers nothing (changed[i] = 0, not an error, as the shapes' degenerate inputs).
 * Values: v is the source voxel's value -- None, or palette_map[index] when a map is given (255 entries, one per palette index 0..254),
 * otherwise the index itself; w is the destination voxel's. PLACE: v solid and w None -> v. OVERWRITE: v solid -> v. REPLACE: every
 * voxel of the image box -> v, None included. CARVE: v solid -> None (the boolean difference). PAINT: v solid and w solid -> v. Every
 * other voxel keeps w. The destination's palette is not touched: indices are copied (or mapped), colours are not.
 * Order: the stamps of a call apply in array order, as n successive calls would. The source is read as it stood when the call began,
 * also when src == dst: a model may be stamped onto itself, with overlapping images, without any memmove hazard. changed[i] is the
 * number of voxels whose value after stamp i differs from their value before it; `changed` may be NULL. Deterministic: two runs give the
 * same bytes and the same counts.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything changes: a null dst or src; null stamps with n > 0; n > DUST_HIP_MAX_STAMPS;
 * models of different contexts; an invalid orient; an unknown op; a palette_map entry above 254. n == 0 is a no-op in the set_voxels
 * sense (it may move dst into its editable form). DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that
 * hold material byte 255), for dst and for src alike, before the stamps are looked at.
 * Synchronous, like edit_shapes: the call returns with dst rebuilt -- the device arrays byte for byte what dust_hip_model_create builds
 * from the resulting voxels -- and changed written. Scenes that instance dst must be committed again; dst's island labelling is
 * invalidated when n > 0. The SOURCE is not modified in any way unless it is dst: it is not moved into editable form, its generation
 * stays, and committed scenes that instance it stay valid (a source that is not editable is expanded into a 16 MiB scratch grid the
 * context owns, allocated by the first call that needs it; nothing is cached from one call to the next). */
#define DUST_HIP_STAMP_PLACE     0u  /* source solid, destination empty -> source's material              */
#define DUST_HIP_STAMP_OVERWRITE 1u  /* source solid -> source's material, whatever was there              */
#define DUST_HIP_STAMP_REPLACE   2u  /* every voxel of the image box takes the source's value, None too    */
#define DUST_HIP_STAMP_CARVE     3u  /* source solid -> None (boolean difference)                          */
#define DUST_HIP_STAMP_PAINT     4u  /* source solid and destination solid -> source's material            */
#define DUST_HIP_MAX_STAMPS 65536u
typedef struct DustHipStamp {        /* 32 bytes */
  int32_t  offset[3];                /* where the lowest corner of the image box lands, destination tree coordinates */
  uint32_t orient;                   /* signed axis permutation, above */
  uint32_t op;
  uint8_t  src_lo[3], pad0;          /* inclusive sub-box of the source, tree coordinates */
  uint8_t  src_hi[3], pad1;
  uint32_t reserved;                 /* ignored */
} DustHipStamp;
DustStatus dust_hip_model_stamp(DustHipModel* dst, const DustHipModel* src, const DustHipStamp* stamps, uint32_t n,
                                const uint8_t* palette_map /* 255 entries, or NULL = identity */, uint32_t* changed /* n, may be NULL */);
/* Model casts: where a voxel piece comes to rest, and whether a prefab fits -- the voxel-against-voxel query between detach_islands
 * ("debris that falls") and stamp ("a detached island that has come to rest"). sweep_boxes moves a box; a detached arch or a wall segment
 * is not one. A cast takes a sub-box of a source model under one of the stamp's 48 orientations, puts it at an integer offset in the
 * destination and moves it in integer steps along a direction: how many steps are free, and what does it touch first?
 *
 * Geometry: the stamp's definitions, word for word -- orient, p[r], g[r], e[k] and the image box offset[r] .. offset[r] + e[p[r]] as
 * above. The piece is the set of solid source voxels s inside [src_lo, src_hi]. With u[r] = s[p[r]] - src_lo[p[r]] when g[r] == 0 and
 * src_hi[p[r]] - s[p[r]] when g[r] == 1, voxel s stands at placement k = 0, 1, ... at
 *   d_k(s)[r] = offset[r] + k * step[r] + u[r].
 * A piece voxel is blocked at k when d_k lies inside the tree (0..255 on every axis) and the destination is solid there, or when d_k
 * lies outside the tree and DUST_HIP_CAST_WALLS is set; without WALLS, voxels outside the tree touch nothing. Placement k is blocked
 * when some piece voxel is.
 * Result: let k* be the smallest blocked placement in 0..max_steps. If there is none: steps = max_steps, flags = 0, contacts = 0,
 * contact = {0, 0, 0}, src_key = DUST_HIP_CAST_NO_KEY. Otherwise flags has HIT; steps = k* - 1, or 0 with OVERLAP when k* == 0; contacts
 * is the number of piece voxels blocked at k*; HIT_WALL is set when one of them stands outside the tree; src_key = x << 16 | y << 8 | z
 * of the blocked source voxel with the smallest such key, and contact = d_k*(that voxel) -- under WALLS it may lie outside 0..255 (it is
 * computed in 64 bits and stored as its low 32: it can only wrap for an offset within 65 790 of the int32 limits). `voxels` is always the
 * number of solid voxels in the source sub-box, whatever the clipping. The piece's resting place is offset + steps * step, ready to go
 * into a DustHipStamp. A zero step is legal: every placement is then placement 0. src_lo > src_hi on any axis, or a piece with no solid
 * voxel, gives no hit and voxels = 0. Any int32 offset is legal: nothing overflows, and the work does not grow with
 * the offset or with max_steps -- no more placements are examined than the piece's image can spend inside the tree.
 * State: both models are only read. dst is moved into its editable form first if it is not there yet, exactly as find_islands does
 * (scenes that instance it must then be committed again); on an editable dst nothing a scene reads changes, and the island labelling
 * and the flood field stay valid. src is treated as a stamp's source: not modified, not made editable, its generation stays. src == dst
 * is allowed and not special: the piece meets its own voxels.
 * The casts of a call are independent: hits[i] is what a call with casts[i] alone returns. Deterministic and exact: everything is integer.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything is written: a null dst or src; null casts or hits with n > 0;
 * n > DUST_HIP_MAX_CASTS; models of different contexts; an invalid orient; a step component outside -1..1;
 * max_steps > DUST_HIP_CAST_MAX_STEPS; flag bits other than WALLS. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees,
 * models that hold material byte 255), for either model, before the records are looked at. n == 0 is a no-op in the find_islands sense
 * (it may move dst into its editable form). Synchronous: the call returns with hits written.
 * Out of scope: motion that is not an integer translation (rotation while moving, float offsets); casts against a scene's
 * instances in world space; excluding an undetached island's own voxels (detach it first, or cast it from a KEEP_SOURCE copy
 * against a carved destination); 4096^3 trees; an asynchronous form. */
#define DUST_HIP_CAST_WALLS     1u   /* DustHipCast.flags: positions outside the tree block, as solid voxels do */
#define DUST_HIP_CAST_HIT       1u   /* DustHipCastHit.flags: some placement 0..max_steps is blocked */
#define DUST_HIP_CAST_OVERLAP   2u   /* ... and it is placement 0 */
#define DUST_HIP_CAST_HIT_WALL  4u   /* ... and at least one contact lies outside the tree */
#define DUST_HIP_CAST_MAX_STEPS 65535u
#define DUST_HIP_MAX_CASTS      65536u
#define DUST_HIP_CAST_NO_KEY    0xFFFFFFFFu
typedef struct DustHipCast {        /* 48 bytes */
  int32_t  offset[3];               /* where the image box's lowest corner is at placement 0 (stamp's offset) */
  uint32_t orient;                  /* stamp's signed axis permutation */
  int32_t  step[3];                 /* each -1, 0 or 1 */
  uint32_t max_steps;               /* 0: a fit test */
  uint32_t flags;
  uint8_t  src_lo[3], pad0, src_hi[3], pad1;
  uint32_t reserved;                /* ignored */
} DustHipCast;
typedef struct DustHipCastHit {     /* 32 bytes */
  uint32_t steps, flags, contacts, voxels;
  int32_t  contact[3];
  uint32_t src_key;
} DustHipCastHit;
DustStatus dust_hip_model_cast(DustHipModel* dst, const DustHipModel* src, const DustHipCast* casts, uint32_t n,
                               DustHipCastHit* hits /* n */);
/* Model floods: questions about the space BETWEEN the solid voxels, and about connectivity with a distance attached -- where an agent can
 * go after an edit and what its next step toward a goal is, whether a room is sealed, how far a gas or a fire gets in k steps, filling
 * what a flood reaches with a material (water in a crater, a paint bucket, a vein of ore), the voxels within k steps of a blast through
 * the structure itself. Coordinates are the model's tree coordinates (what set_voxels takes), on 256^3 models.
 *
 * A flood has a medium, which decides the voxels that are passable: DUST_HIP_FLOOD_EMPTY the voxels holding None, DUST_HIP_FLOOD_SOLID the
 * solid voxels of any material, DUST_HIP_FLOOD_MATERIAL the solid voxels whose palette index equals query.palette. A voxel outside the
 * query's inclusive region box [lo, hi] is never passable; the box is clipped to the tree, and lo > hi on any axis means nothing is
 * passable. A step goes from a passable voxel to a passable voxel sharing a face (6 neighbours). steps(v) is the smallest number of steps
 * from any seed to v; it is DUST_HIP_FLOOD_UNREACHED when v is not passable, not connected to a seed, or farther than query.max_steps
 * (at most DUST_HIP_FLOOD_MAX_STEPS). Seeds that are not passable or lie outside the region are ignored (not an error); duplicates are
 * harmless; n_seeds == 0 is legal and gives an all-unreached, valid field. Everything is integer and the field is a unique fixed point:
 * two runs give the same bytes whatever the scheduling.
 *
 * dust_hip_model_flood computes the field and leaves it on the device with the model -- one uint16 per voxel, 32 MiB on top of the editable
 * form, allocated by the first call and released with the model -- replacing the previous field. A model that is not yet editable is moved
 * into its editable form first, exactly as find_islands does (scenes that instance it must then be committed again); on an editable model
 * the call changes nothing a scene reads. The result record: reached, the voxels with steps != UNREACHED; farthest, the largest steps
 * value; seeds_used, the voxels with steps == 0; boundary, the reached voxels that lie on a face of the clipped region (0: the flood is
 * enclosed); lo / hi, the inclusive bounds of the reached voxels. With reached == 0 every member is 0.
 * dust_hip_model_flood_at reads the field at coordinates, as island_of reads labels.
 * dust_hip_model_flood_paths descends the field: for a reached start s with d = steps(s) the path is p_0 = s, ..., p_d, where p_(i+1) is
 * the neighbour of p_i with steps == steps(p_i) - 1, the first such in the order -x, +x, -y, +y, -z, +z; p_d is a seed. lengths[i] = d + 1
 * whatever the capacity; the first min(d + 1, capacity) voxels are written to keys[i * capacity ..] as x << 16 | y << 8 | z (the island key
 * format) and the slots past them are left untouched. An unreached start has lengths[i] = 0 and writes nothing. capacity == 2 is "my
 * next step toward the goal".
 * dust_hip_model_flood_apply gives every voxel with steps != UNREACHED && steps <= max_steps the value `value` (a palette index 0..254, or
 * negative for None; any uint32 is a legal max_steps). *changed is the number of voxels whose value differs afterwards. The model is
 * rebuilt as after an edit -- its arrays byte for byte what dust_hip_model_create builds from the resulting voxels -- and its generation
 * bumped: scenes must commit again.
 * Validity: the field is invalidated by every set_voxels, edit_shapes, stamp (as destination) and carving detach_islands with n > 0, by
 * flood_apply itself, and by a flood that fails. find_islands, island_of, KEEP_SOURCE detaches and being a stamp's source leave it
 * standing. flood and flood_apply treat the island labelling as any edit would: flood leaves it, flood_apply invalidates it.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything changes: a null model, query or lengths; a struct_size below
 * sizeof(DustHipFloodQuery); an unknown medium; palette outside 0..254 under MATERIAL; max_steps > DUST_HIP_FLOOD_MAX_STEPS in a query;
 * null arrays with n > 0; n_seeds > DUST_HIP_MAX_FLOOD_SEEDS; a seed, start or lookup coordinate >= 256; null keys with capacity > 0 and
 * n > 0; value > 254. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material byte 255), before
 * anything but the model pointer is looked at. DUST_ERR_NOT_READY from flood_at, flood_paths and flood_apply without a standing field,
 * also with n == 0. All four calls are synchronous.
 * Out of scope: ground-walking agents (clearance, step height); 26-neighbour or weighted steps; floods across the instances of a scene,
 * in world space; 4096^3 trees; an asynchronous form. */
#define DUST_HIP_FLOOD_EMPTY    0u   /* passable: voxels holding None */
#define DUST_HIP_FLOOD_SOLID    1u   /* passable: solid voxels of any material */
#define DUST_HIP_FLOOD_MATERIAL 2u   /* passable: solid voxels whose palette index equals query.palette */
#define DUST_HIP_FLOOD_UNREACHED 0xFFFFu
#define DUST_HIP_FLOOD_MAX_STEPS 65534u
#define DUST_HIP_MAX_FLOOD_SEEDS 65536u
typedef struct DustHipFloodQuery {   /* 40 bytes */
  uint32_t struct_size, medium;
  int32_t  palette;                  /* read by DUST_HIP_FLOOD_MATERIAL only: 0..254 */
  uint32_t max_steps;                /* 0..65534; larger values are refused */
  uint32_t lo[3], hi[3];             /* inclusive region, clipped to the tree */
} DustHipFloodQuery;
typedef struct DustHipFloodResult {  /* 32 bytes */
  uint32_t reached;                  /* voxels with steps != UNREACHED */
  uint32_t farthest;                 /* the largest steps value (0 when reached == 0) */
  uint32_t seeds_used;               /* voxels with steps == 0 */
  uint32_t boundary;                 /* reached voxels on a face of the clipped region: 0 = the flood is enclosed */
  uint8_t lo[3], pad0, hi[3], pad1;  /* inclusive bounds of the reached voxels; all 0 when reached == 0 */
  uint32_t reserved[2];              /* 0 */
} DustHipFloodResult;
DustStatus dust_hip_model_flood(DustHipModel*, const DustHipFloodQuery*, const uint32_t* seeds_xyz, uint32_t n_seeds,
                                DustHipFloodResult* out /* may be NULL */);
DustStatus dust_hip_model_flood_at(DustHipModel*, const uint32_t* xyz, uint16_t* steps, uint32_t n);
DustStatus dust_hip_model_flood_paths(DustHipModel*, const uint32_t* starts_xyz, uint32_t n, uint32_t capacity,
                                      uint32_t* keys /* n * capacity, may be NULL when capacity == 0 */, uint32_t* lengths /* n */);
DustStatus dust_hip_model_flood_apply(DustHipModel*, uint32_t max_steps, int32_t value, uint32_t* changed /* may be NULL */);
/* Model distances: how much ROOM there is. Rays, boxes, islands, floods and casts answer which voxels are solid, or count unit steps
 * through faces; a distance field answers whether a sphere of radius r fits at a voxel, how thick a wall is here, where the roomiest
 * spot is, and which voxels lie within r of the surface -- growing terrain by r (snow, moss, armour), eroding it by r (melt,
 * weathering), painting the outer k voxels of a solid (scorch, rust). Coordinates are the model's tree coordinates, on 256^3 models.
 *
 * A query has a target set: DUST_HIP_DISTANCE_TO_SOLID the solid voxels, DUST_HIP_DISTANCE_TO_EMPTY the voxels holding None,
 * DUST_HIP_DISTANCE_TO_MATERIAL the solid voxels whose palette index equals query.palette. value(v) is the minimum over all targets t of
 * the metric between the voxel coordinates of v and t: under DUST_HIP_DISTANCE_EUCLIDEAN dx^2 + dy^2 + dz^2, the SQUARED distance (an
 * integer; take the root on the host if you need it), under DUST_HIP_DISTANCE_CHEBYSHEV max(|dx|, |dy|, |dz|), the clearance of a cube.
 * A target itself holds 0. With R = query.max_radius (1..DUST_HIP_DISTANCE_MAX_RADIUS) the limit is R^2 under EUCLIDEAN and R under
 * CHEBYSHEV: a value above the limit, or no target at all, is reported as DUST_HIP_DISTANCE_FAR; a value at or below it is exact.
 * With R = 255 and one target at (0, 0, 0), voxel (255, 0, 0) holds 65025 and voxel (255, 1, 0) holds FAR. Under the flag
 * DUST_HIP_DISTANCE_WALLS every voxel outside the tree (coordinate -1 or 256 on an axis, and beyond) is a target too; the nearest of
 * them lies straight across the nearest face, so the value is min(value, w^2) under EUCLIDEAN and min(value, w) under CHEBYSHEV with
 * w = min over the axes of min(c + 1, 256 - c), under the same limit. Everything is integer: two runs give the same bytes.
 * Three identities: a ball of radius r around a voxel's centre holds no target centre iff the EUCLIDEAN value is above r^2; a cube of
 * half-width k (2 k + 1 voxels wide) around a voxel holds no target iff the CHEBYSHEV value is above k; TO_EMPTY with WALLS is "how deep
 * inside the solid" (wall thickness on the solid side), and the maximum of a TO_SOLID field is the roomiest spot on the empty side.
 *
 * dust_hip_model_distance computes the field and leaves it on the device with the model -- one uint16 per voxel, brick-major like the
 * editable grid, 32 MiB of its own next to the flood field and the island labelling, allocated by the first call and released with the
 * model -- replacing the previous distance field. A model that is not yet editable is moved into its editable form first, exactly as
 * flood does (scenes that instance it must then be committed again); on an editable model the call changes nothing a scene reads. The
 * result record: targets, the voxels with value 0; near, the voxels with 0 < value != FAR; far, the voxels with value FAR (the three sum
 * to 2^24); largest, the largest value != FAR (0 when there is none); largest_key, x << 16 | y << 8 | z of the LOWEST-keyed voxel that
 * holds it, DUST_HIP_DISTANCE_NO_KEY when targets + near == 0.
 * dust_hip_model_distance_at reads the field at coordinates, as flood_at reads steps.
 * dust_hip_model_distance_apply gives every voxel with value != FAR && lo <= value <= hi the value `value` (a palette index 0..254, or
 * negative for None). lo and hi are in the field's own units -- squared under EUCLIDEAN --, any uint32 is legal and lo > hi matches
 * nothing. *changed is the number of voxels whose value differs afterwards. The model is rebuilt as after flood_apply -- its arrays
 * byte for byte what dust_hip_model_create builds from the resulting voxels -- and its generation bumped: scenes must commit again.
 * With r = 2 under EUCLIDEAN (r^2 = 4): a TO_SOLID field, range 1..4 and a palette index grow the solid by 2; a TO_EMPTY field, range
 * 1..4 and None erode it by 2; a TO_EMPTY field, range 1..4 and a palette index paint its two-voxel skin.
 * Validity: the distance field stands under exactly the rules of the flood field. It is invalidated by every set_voxels, edit_shapes,
 * stamp (as destination) and carving detach_islands with n > 0, by flood_apply, by distance_apply itself, and by a distance call that
 * fails. find_islands, island_of, flood, flood_at, flood_paths, KEEP_SOURCE detaches and being a stamp's or a cast's source leave it
 * standing. distance leaves the flood field and the island labelling standing; distance_apply invalidates all three, as any edit does.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything changes: a null model or query; a struct_size below
 * sizeof(DustHipDistanceQuery); an unknown target, metric or flag bit; palette outside 0..254 under TO_MATERIAL; max_radius of 0 or above
 * DUST_HIP_DISTANCE_MAX_RADIUS; null arrays with n > 0; a coordinate >= 256; value > 254. DUST_ERR_UNSUPPORTED exactly where set_voxels
 * returns it (4096^3 trees, models that hold material byte 255), before anything but the model pointer is looked at.
 * DUST_ERR_NOT_READY from distance_at and distance_apply without a standing field, also with n == 0. All three calls are synchronous.
 * Out of scope: a flood restricted by clearance (what agent-sized paths need: an entry point of its own, DustHipFloodQuery stays as it
 * is); listing the voxels above a value; Manhattan distance; distances across the instances of a scene, in world space; 4096^3 trees; an
 * asynchronous form. */
#define DUST_HIP_DISTANCE_TO_SOLID    0u  /* targets: the solid voxels */
#define DUST_HIP_DISTANCE_TO_EMPTY    1u  /* targets: the voxels holding None */
#define DUST_HIP_DISTANCE_TO_MATERIAL 2u  /* targets: the solid voxels whose palette index equals query.palette */
#define DUST_HIP_DISTANCE_EUCLIDEAN   0u  /* value = dx^2 + dy^2 + dz^2 between voxel coordinates (the SQUARED distance) */
#define DUST_HIP_DISTANCE_CHEBYSHEV   1u  /* value = max(|dx|, |dy|, |dz|): the clearance of a cube */
#define DUST_HIP_DISTANCE_WALLS       1u  /* flags: every voxel outside the tree is a target too */
#define DUST_HIP_DISTANCE_FAR         0xFFFFu
#define DUST_HIP_DISTANCE_MAX_RADIUS  255u
#define DUST_HIP_DISTANCE_NO_KEY      0xFFFFFFFFu
typedef struct DustHipDistanceQuery {   /* 32 bytes */
  uint32_t struct_size, target, metric, flags;
  int32_t  palette;                     /* read under TO_MATERIAL only: 0..254 */
  uint32_t max_radius;                  /* 1..255 */
  uint32_t reserved[2];                 /* 0 */
} DustHipDistanceQuery;
typedef struct DustHipDistanceResult {  /* 32 bytes */
  uint32_t targets;                     /* voxels with value 0 */
  uint32_t near;                        /* voxels with 0 < value != FAR */
  uint32_t far;                         /* voxels with value FAR; targets + near + far == 2^24 */
  uint32_t largest;                     /* the largest value != FAR (0 when there is none) */
  uint32_t largest_key;                 /* x << 16 | y << 8 | z of the LOWEST-keyed voxel holding it; NO_KEY when targets + near == 0 */
  uint32_t reserved[3];                 /* 0 */
} DustHipDistanceResult;
DustStatus dust_hip_model_distance(DustHipModel*, const DustHipDistanceQuery*, DustHipDistanceResult* out /* may be NULL */);
DustStatus dust_hip_model_distance_at(DustHipModel*, const uint32_t* xyz, uint16_t* values, uint32_t n);
DustStatus dust_hip_model_distance_apply(DustHipModel*, uint32_t lo, uint32_t hi, int32_t value, uint32_t* changed /* may be NULL */);
/* Model reductions: coarser copies of a model, level by level -- a level of detail for the instances that are far away, a cheap
 * collision or line-of-sight proxy for the scene queries, a minimap, a half-resolution grid for flood and distance at an eighth of
 * the cost. The copy is made from the model as it stands NOW on the device, edits included, without a round trip over the host.
 *
 * One level: values are a palette index (0..254) or None. Coarse voxel (X, Y, Z), X, Y, Z < 128, has the eight children
 * (2X + i, 2Y + j, 2Z + k), i, j, k in {0, 1}. With s the number of solid children, the coarse voxel is solid iff s >= min_solid
 * (1..8); its palette index is the one most of its solid children carry, and among indices with the same highest count the lowest
 * index wins. Coarse voxels with a coordinate >= 128 are empty. min_solid = 1 never opens a hole (a render LOD, a collision proxy),
 * min_solid = 4 keeps the volume roughly, min_solid = 8 keeps only the cells that are solid throughout (a safe interior for navigation).
 * levels = n is that rule applied n times with the same min_solid -- the vote of votes, NOT one vote over 8^n voxels -- so a reduction
 * by 2 levels holds exactly what the reduction by 1 level of a reduction by 1 level holds; levels = 8 is a single voxel at the origin.
 * Everything is integer: two runs give the same bytes.
 *
 * The new model: *out is on the source's context and has the source's palette. It is a hierarchy (4,2,2) model (256^3 tree) whose
 * voxels occupy [0, 256 >> levels)^3, born editable exactly as detach_islands' output is (about 44 MB, unlabelled, no fields, the
 * caller's to destroy), its arrays byte for byte what dust_hip_model_create builds from those voxels. An instance whose obj_to_world
 * is the source's times a uniform scale of 2^levels shows the reduction where the source stands. An empty result is a valid empty
 * model, not an error. The result record: src_voxels, the solid voxels of the source; voxels, those of the new model; extent,
 * 256 >> levels.
 * The source is only read: one that is not editable stays not editable (it is expanded into the context's 16 MiB scratch grid, as a
 * stamp's source is), its generation does not move -- committed scenes that instance it stay valid --, and its island labelling and
 * fields stay valid. With levels >= 2 the levels take turns between the new model's grid and a second 16 MiB grid the context owns,
 * allocated by the first such call.
 * Refused, in this order, with *out and *result left as they were (as on any device failure): DUST_ERR_INVALID_ARGUMENT for a null
 * src, query or out, or a struct_size below sizeof(DustHipReduce); DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3
 * trees, models that hold material byte 255), before the query's values are looked at; DUST_ERR_INVALID_ARGUMENT for levels outside
 * 1..DUST_HIP_REDUCE_MAX_LEVELS, min_solid outside 1..8, or nonzero flags. Synchronous, like every model call.
 * Out of scope: reducing a sub-box of the source; an asynchronous form; 4096^3 trees; choosing between levels while rendering -- the
 * renderer traces the model an instance names, level selection is the host's. */
#define DUST_HIP_REDUCE_MAX_LEVELS 8u
typedef struct DustHipReduce {        /* 16 bytes */
  uint32_t struct_size;
  uint32_t levels;                    /* 1..8: the result spans (256 >> levels)^3 voxels from the origin */
  uint32_t min_solid;                 /* 1..8: a coarse voxel is solid when at least this many of its 8 children are */
  uint32_t flags;                     /* 0 */
} DustHipReduce;
typedef struct DustHipReduceResult {  /* 16 bytes */
  uint32_t src_voxels;                /* solid voxels of the source */
  uint32_t voxels;                    /* solid voxels of the new model */
  uint32_t extent;                    /* 256 >> levels */
  uint32_t reserved;                  /* 0 */
} DustHipReduceResult;
DustStatus dust_hip_model_reduce(const DustHipModel* src, const DustHipReduce*, DustHipModel** out,
                                 DustHipReduceResult* result /* may be NULL */);
/* Model censuses: what a region holds, counted on the device without changing anything -- what a blast will remove and of which
 * materials (loot, debris colour, damage, score), how much ore a chunk has, what a piece weighs given a density per material, whether
 * a box is empty enough to build in. The read-only sibling of edit_shapes: ask first, carve after.
 *
 * Shapes: they are edit_shapes' shapes, DustHipEditShape records in the model's tree coordinates. A shape covers the voxels whose centre
 * it contains, under the float32 contract stated at edit_shapes, operation for operation (the device runs one text for both calls),
 * clipped to the tree. op, palette and reserved are ignored and not validated: an array built for edit_shapes can be passed unchanged.
 * Independence: every shape is counted on its own against the model as it stands. Unlike edits, order does not matter and overlapping
 * shapes each see every voxel.
 * Records: covered, the voxels of the tree whose centre the shape contains; solid, those of them that are solid; lo / hi, the inclusive
 * bounds of the solid covered voxels (255, 255, 255 / 0, 0, 0 when solid == 0); sum, the sums of x, of y and of z over the solid
 * covered voxels (centre of mass = sum / solid + 0.5); the reserved bytes are 0. An edit_shapes CARVE of the same shape changes exactly
 * `solid` voxels, a PLACE exactly covered - solid.
 * Tables: counts[i * 256 + 0] is the number of covered voxels that hold None, counts[i * 256 + 1 + p] the number that hold palette
 * index p (0..254). A row sums to covered, and its entries 1..255 sum to solid.
 * Shapes that cover nothing get the zero record (bounds 255 / 0, as for solid == 0) and a zero row. The cases are exactly those of
 * edit_shapes: a non-finite value in a field the kind reads; a[r] > b[r] on a box; radius < 0 on a sphere or capsule; for spheres and
 * capsules any |coordinate| or radius above 65 536; and a shape wholly outside the tree.
 * The model is only read. One that is not editable stays not editable (it is expanded into the context's 16 MiB scratch grid, as a
 * stamp's or a reduction's source is); an editable one is read in place, edits included. The generation does not move -- committed
 * scenes that instance the model stay valid --, and the island labelling and both fields stay valid.
 * Everything is integer arithmetic: two runs give the same bytes.
 * Refused with DUST_ERR_INVALID_ARGUMENT, the outputs untouched: a null model; null shapes with n > 0; n > DUST_HIP_MAX_CENSUS_SHAPES;
 * counts != NULL with n > DUST_HIP_MAX_CENSUS_TABLES (a row is 1 KiB); a kind above CAPSULE. DUST_ERR_UNSUPPORTED exactly where
 * set_voxels returns it (4096^3 trees, models that hold material byte 255), before the shapes are looked at. n == 0 is a no-op; records
 * and counts may each be NULL, and with both NULL the call validates and returns. Synchronous, like every model call.
 * Out of scope: an asynchronous form; world-space shapes over a scene's instances; regions named by an island key or by a
 * field's range; second moments (an inertia tensor). */
#define DUST_HIP_MAX_CENSUS_SHAPES 65536u   /* records only */
#define DUST_HIP_MAX_CENSUS_TABLES 4096u    /* with per-material tables (1 KiB each) */
#define DUST_HIP_CENSUS_BINS 256u
typedef struct DustHipCensus {   /* 40 bytes, laid out like DustHipIsland */
  uint32_t covered;              /* voxels of the tree whose centre the shape contains */
  uint32_t solid;                /* ... of them solid */
  uint8_t lo[3], reserved0;      /* inclusive bounds of the solid covered voxels; 255,255,255 when solid == 0 */
  uint8_t hi[3], reserved1;      /* 0,0,0 when solid == 0; reserved bytes 0 */
  uint64_t sum[3];               /* sums of x, of y, of z over the solid covered voxels */
} DustHipCensus;
DustStatus dust_hip_model_census(const DustHipModel*, const DustHipEditShape* shapes, uint32_t n,
                                 DustHipCensus* records /* n, may be NULL */,
                                 uint32_t* counts /* n * 256, may be NULL */);
/* Model surfaces: where the solid meets the air, and facing which way -- grass or snow on every voxel whose top face is open, soot on
 * the faces a blast opened, the surface area of a piece per material (drag, burn rate, paint needed), the surface voxels as a list
 * with their open faces (spawn points for particles and decals, the input of a host-side mesher or a physics engine, the only voxels
 * worth sending over a network), and peeling exactly one layer off a solid (weathering) without a cascade.
 *
 * Exposed: face d of a solid voxel is exposed when the voxel across d is empty. Across a face of the tree the neighbour is empty, or
 * solid under DUST_HIP_SURFACE_WALLS. The directions are the DUST_HIP_FACE_* bits: bit 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z.
 * Region: lo / hi is an inclusive voxel box, clipped to the tree (as DustHipFloodQuery's). It selects which voxels are looked at;
 * neighbours outside the region, but inside the tree, are consulted as they are. lo > hi on an axis is legal and empty: the zero
 * result (bounds 255 / 0), changed 0.
 * Listed: a voxel is listed when it is solid, lies inside the clipped region, passes the palette filter (palette -1: every solid
 * voxel; 0..254: only voxels of that palette index) and has at least one exposed face among query.faces.
 * Order and capacity: the listed voxels come in the order of the model's Blocks (Tree::iter_leaf, the order dust_hip_model_read
 * uses), then ascending voxel bit (x&3)<<4 | (y&3)<<2 | (z&3). The first min(result.voxels, capacity) entries are written; the slots
 * past them are left untouched. result.voxels is the full count whatever the capacity (the convention of find_islands); capacity 0
 * counts only. A record's faces are its exposed faces among query.faces, never 0; its palette is the voxel's, 0..254.
 * Tables: counts[d * 256 + 1 + p] is the number of exposed faces of direction d, among query.faces, on listed voxels of palette index
 * p. Bin 0 of every row is 0, rows of directions not in query.faces are 0, and the table sums to result.faces.
 * Result: voxels, the listed voxels; faces, their exposed faces among query.faces; by_face, the same per direction (sums to faces);
 * solid, the solid voxels in the region that pass the palette filter, listed or hidden; lo / hi, the inclusive bounds of the listed
 * voxels (255, 255, 255 / 0, 0, 0 when there is none, as in DustHipCensus); the reserved words are 0.
 * dust_hip_model_surface only reads the model, with census's guarantees: one that is not editable stays not editable (its blocks'
 * masks are scattered into the context's 2 MiB scratch as for a cast's source, and it is expanded into the 16 MiB scratch grid only
 * when a material is needed: a palette filter, tables, a list); the generation does not move; the island labelling and both fields
 * stand.
 * dust_hip_model_surface_apply gives every listed voxel `value`: a palette index 0..254, or negative for None. What is listed is
 * decided on the model as it stood when the call began: a None peels exactly one layer, the voxels behind do not follow. *changed is
 * the number of voxels whose value differs afterwards. The model is rebuilt as after flood_apply, byte for byte a host build; the
 * generation is bumped, the island labelling and both fields are invalid afterwards.
 * Refused with DUST_ERR_INVALID_ARGUMENT, the outputs untouched: a null model or query; a struct_size below the struct's size; faces
 * of 0 or above 63; an unknown flag bit; a palette below -1 or above 254; a region coordinate >= 256; null voxels with capacity > 0;
 * a value > 254. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material byte 255),
 * before the query is looked at. Both calls are synchronous, like every model call. Everything is integer arithmetic: two runs give
 * the same bytes.
 * Out of scope: merged quads (greedy meshing); seams between different materials as faces; faces across the instances of a scene in
 * world space; 4096^3 trees; an asynchronous form. */
#define DUST_HIP_FACE_NEG_X 1u
#define DUST_HIP_FACE_POS_X 2u
#define DUST_HIP_FACE_NEG_Y 4u
#define DUST_HIP_FACE_POS_Y 8u
#define DUST_HIP_FACE_NEG_Z 16u
#define DUST_HIP_FACE_POS_Z 32u
#define DUST_HIP_FACES_ALL 63u
#define DUST_HIP_SURFACE_WALLS 1u  /* flags: the outside of the tree counts as solid (as DUST_HIP_CAST_WALLS, DUST_HIP_DISTANCE_WALLS) */
#define DUST_HIP_SURFACE_BINS 256u
typedef struct DustHipSurfaceQuery {   /* 48 bytes */
  uint32_t struct_size;
  uint32_t faces;                /* 1..63: the directions that count */
  uint32_t flags;                /* DUST_HIP_SURFACE_WALLS or 0 */
  int32_t palette;               /* -1: every solid voxel; 0..254: only voxels of this palette index */
  uint32_t lo[3], hi[3];         /* inclusive region, clipped to the tree */
  uint32_t reserved[2];          /* 0 */
} DustHipSurfaceQuery;
typedef struct DustHipSurfaceResult {  /* 64 bytes */
  uint32_t voxels;               /* listed voxels */
  uint32_t faces;                /* their exposed faces among query.faces */
  uint32_t by_face[6];           /* ... per direction; sums to faces */
  uint32_t solid;                /* solid voxels in the region that pass the palette filter (listed + hidden) */
  uint8_t lo[3], pad0;           /* inclusive bounds of the listed voxels; 255,255,255 when there is none */
  uint8_t hi[3], pad1;           /* 0,0,0 when there is none; pad bytes 0 */
  uint32_t reserved[5];          /* 0 */
} DustHipSurfaceResult;
typedef struct DustHipSurfaceVoxel {   /* 8 bytes */
  uint32_t key;                  /* x << 16 | y << 8 | z */
  uint8_t faces;                 /* exposed & query.faces, never 0 */
  uint8_t palette;               /* 0..254 */
  uint16_t reserved;             /* 0 */
} DustHipSurfaceVoxel;
DustStatus dust_hip_model_surface(const DustHipModel*, const DustHipSurfaceQuery*, DustHipSurfaceResult* result /* may be NULL */,
                                  DustHipSurfaceVoxel* voxels /* capacity; may be NULL when capacity == 0 */, uint32_t capacity,
                                  uint32_t* counts /* 6 * 256, may be NULL */);
DustStatus dust_hip_model_surface_apply(DustHipModel*, const DustHipSurfaceQuery*, int32_t value, uint32_t* changed /* may be NULL */);
/* Model meshes: a model in the form everything outside a ray tracer wants, a short list of rectangles -- flat colliders for a
 * physics engine, quads for a rasterised fallback, a shadow proxy, an editor gizmo, an export or a network snapshot.
 * dust_hip_model_mesh returns the exposed faces of the solid voxels, per direction, merged into axis-aligned rectangles under one
 * canonical rule: the output is a function of the model and the query alone, two runs or two implementations give the same bytes.
 *
 * Face set: for direction d, F_d is exactly what dust_hip_model_surface counts in by_face[d] for the same faces, palette, region and
 * WALLS: the voxels that are solid, lie inside the clipped inclusive region, pass the palette filter and whose face d is exposed (the
 * neighbour across d is empty, or lies off the tree without DUST_HIP_MESH_WALLS), for the d among query.faces.
 * Axes: the normal axis n is that of d. In the plane, u is the higher-numbered remaining axis and v the other one: faces -x / +x have
 * u = z, v = y; faces -y / +y have u = z, v = x; faces -z / +z have u = y, v = x. A slice is one value of the n coordinate, a row one
 * value of v within a slice.
 * Run: a maximal set of consecutive u in one row whose voxels are all in F_d and all hold the same palette index (under
 * DUST_HIP_MESH_ANY_PALETTE the palette condition is dropped).
 * Quad: a maximal set of consecutive rows v0..v1 of one slice that each contain the identical run: the same u0, the same u1 and the
 * same palette index (unless ANY_PALETTE). Rows v0 - 1 and v1 + 1 do not contain that run; a longer or shorter run in a neighbouring
 * row does not merge. The quads partition F_d into rectangles. This is NOT the minimum-count greedy mesh: a greedy mesher may split a
 * long run to grow a taller rectangle, this rule never does. In exchange the answer depends on no processing order.
 * Order and capacity: the quads come in ascending order of face index d (0..5, the bit order of DUST_HIP_FACE_*), then slice, then
 * v0, then u0. The first min(result.quads, capacity) records are written; the slots past them are left untouched. result.quads is
 * the full count whatever the capacity; capacity 0 counts only.
 * Record: key is x << 16 | y << 8 | z of the voxel at (u0, v0), the quad's lowest corner; face the direction index 0..5 (not the
 * bit); palette 0..254, under ANY_PALETTE that of the key voxel; du and dv the extents along u and v minus 1 (extents run 1..256).
 * The device writes a record as one 64-bit word.
 * Result: quads; faces, the sum of the quads' areas, which equals dust_hip_model_surface's faces for the same query;
 * quads_by_face; faces_by_face, which equals its by_face; largest, the area of the largest quad (0 when there is none); reserved 0.
 * lo > hi on an axis is legal and gives the zero result.
 * The model is only read, with dust_hip_model_surface's guarantees: one that is not editable stays not editable (its blocks' masks
 * are scattered into the context's 2 MiB scratch, and it is expanded into the 16 MiB scratch grid only when a material is needed:
 * a palette filter, runs that stop at a change of material, a list); the generation does not move; the island labelling and both
 * fields stand.
 * Refused with DUST_ERR_INVALID_ARGUMENT, every output untouched: a null model or query; a struct_size below the struct's size;
 * faces of 0 or above 63; a flag bit above 3; a palette below -1 or above 254; a region coordinate >= 256; null quads with
 * capacity > 0. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material byte 255), before
 * the query is looked at. The call is synchronous, like every model call. Everything is integer arithmetic.
 * Out of scope: the minimum-count greedy mesh; T-junction-free output; seams between different materials as faces; vertex or index
 * buffers on the device; faces across the instances of a scene; 4096^3 trees; an asynchronous form. */
#define DUST_HIP_MESH_WALLS 1u        /* flags: the outside of the tree counts as solid (DUST_HIP_SURFACE_WALLS) */
#define DUST_HIP_MESH_ANY_PALETTE 2u  /* flags: runs and quads merge across palette indices */
typedef struct DustHipMeshQuery {      /* 48 bytes, field for field DustHipSurfaceQuery */
  uint32_t struct_size;
  uint32_t faces;                /* 1..63: the directions that count (DUST_HIP_FACE_*) */
  uint32_t flags;                /* DUST_HIP_MESH_WALLS | DUST_HIP_MESH_ANY_PALETTE */
  int32_t palette;               /* -1: every solid voxel; 0..254: only voxels of this palette index */
  uint32_t lo[3], hi[3];         /* inclusive region, clipped to the tree */
  uint32_t reserved[2];          /* 0 */
} DustHipMeshQuery;
typedef struct DustHipMeshQuad {       /* 8 bytes */
  uint32_t key;                  /* x << 16 | y << 8 | z of the voxel at (u0, v0) */
  uint8_t face;                  /* direction index 0..5 */
  uint8_t palette;               /* 0..254; under ANY_PALETTE that of the key voxel */
  uint8_t du;                    /* extent along u minus 1 */
  uint8_t dv;                    /* extent along v minus 1 */
} DustHipMeshQuad;
typedef struct DustHipMeshResult {     /* 64 bytes */
  uint32_t quads;                /* number of quads */
  uint32_t faces;                /* the sum of their areas */
  uint32_t quads_by_face[6];     /* quads per direction; sums to quads */
  uint32_t faces_by_face[6];     /* area per direction; sums to faces */
  uint32_t largest;              /* area of the largest quad; 0 when there is none */
  uint32_t reserved;             /* 0 */
} DustHipMeshResult;
DustStatus dust_hip_model_mesh(const DustHipModel*, const DustHipMeshQuery*, DustHipMeshResult* result /* may be NULL */,
                               DustHipMeshQuad* quads /* capacity; may be NULL when capacity == 0 */, uint32_t capacity);
/* Model boxes: a solid as a short list of axis-aligned boxes -- the convex pieces of a compound collider for a rigid-body solver (a
 * detached island, a fractured piece), the smallest exact snapshot of a model the library hands out, a replayable description (every
 * box is a DUST_HIP_SHAPE_BOX record of dust_hip_model_edit_shapes), and the volume counterpart of dust_hip_model_mesh for editors and
 * exports. dust_hip_model_boxes merges the solid voxels under one canonical rule: the output is a function of the model and the
 * query alone, two runs or two implementations give the same bytes.
 *
 * Query: DustHipSurfaceQuery's layout with `axis` where `faces` stands: the stacking axis n (0 x, 1 y, 2 z), the last one merged.
 * Set S: the voxels that are solid, lie inside the clipped inclusive region and pass the palette filter (palette -1: every solid
 * voxel; 0..254: only voxels of that palette index) -- what dust_hip_model_surface counts in `solid` for the same palette and region.
 * Nothing outside the region exists for the call: runs, rects and boxes are cut at the region's faces.
 * Axes: dust_hip_model_mesh's. n = x: u = z, v = y; n = y: u = z, v = x; n = z: u = y, v = x. A slice is one value of the n
 * coordinate, a row one value of v within a slice.
 * Run: a maximal set of consecutive u in one row whose voxels are all in S and all hold the same palette index (under
 * DUST_HIP_BOXES_ANY_PALETTE the palette condition is dropped).
 * Rect: a maximal set of consecutive rows v0..v1 of one slice that each contain the identical run: the same u0, the same u1 and the
 * same palette index (unless ANY_PALETTE) -- dust_hip_model_mesh's quad over S instead of the exposed faces.
 * Box: a maximal set of consecutive slices s0..s1 that each contain the identical rect: the same u0, u1, v0, v1 and palette index
 * (unless ANY_PALETTE). Slices s0 - 1 and s1 + 1 do not contain that rect; a larger or smaller rect at the same corner does not
 * merge. The boxes partition S. This is NOT the minimum-count decomposition: in exchange the answer depends on no processing order.
 * Record: key is x << 16 | y << 8 | z of the box's lowest corner voxel; palette 0..254, under ANY_PALETTE that of the key voxel; dx,
 * dy, dz the extents along the world axes minus 1 (extents run 1..256). The device writes a record as one 64-bit word.
 * Order and capacity: the boxes come in ascending (s0, v0, u0); for axis 0 that is ascending key. The first min(result.boxes,
 * capacity) records are written; the slots past them are left untouched. result.boxes is the full count whatever the capacity;
 * capacity 0 counts only.
 * Result: boxes; rects, the rects of all slices (the boxes there would be without stacking); voxels, |S|, which equals the sum of the
 * boxes' volumes; lo / hi, the inclusive bounds of S (255, 255, 255 / 0, 0, 0 when S is empty); the pad and reserved words are 0.
 * There is no "largest volume": a count-only call needs the depth of no box and stays one launch.
 * lo > hi on an axis is legal and gives the zero result (bounds 255 / 0).
 * The model is only read, with dust_hip_model_surface's guarantees: one that is not editable stays not editable (its blocks' masks
 * are scattered into the context's 2 MiB scratch, and it is expanded into the 16 MiB scratch grid only when a byte is needed: a
 * palette filter, runs that stop at a change of material, a list); the generation does not move; the island labelling and all
 * fields stand.
 * Refused with DUST_ERR_INVALID_ARGUMENT, every output untouched: a null model or query; a struct_size below the struct's size; an
 * axis above 2; a flag bit other than DUST_HIP_BOXES_ANY_PALETTE; a palette below -1 or above 254; a region coordinate >= 256; null
 * boxes with capacity > 0. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material byte
 * 255), before the query is looked at. The call is synchronous, like every model call. Everything is integer arithmetic: two runs
 * give the same bytes.
 * Out of scope: the minimum-count decomposition; boxes across materials other than by ANY_PALETTE; convex pieces other than boxes;
 * 4096^3 trees; an asynchronous form; boxes across the instances of a scene. */
#define DUST_HIP_BOXES_ANY_PALETTE 1u  /* flags: runs, rects and boxes merge across palette indices */
typedef struct DustHipBoxesQuery {     /* 48 bytes, DustHipSurfaceQuery's layout with `axis` where `faces` stands */
  uint32_t struct_size;
  uint32_t axis;                 /* 0..2: the stacking axis n, the last one merged */
  uint32_t flags;                /* DUST_HIP_BOXES_ANY_PALETTE or 0 */
  int32_t palette;               /* -1: every solid voxel; 0..254: only voxels of this palette index */
  uint32_t lo[3], hi[3];         /* inclusive region, clipped to the tree */
  uint32_t reserved[2];          /* 0 */
} DustHipBoxesQuery;
typedef struct DustHipBox {            /* 8 bytes */
  uint32_t key;                  /* x << 16 | y << 8 | z of the box's lowest corner voxel */
  uint8_t palette;               /* 0..254; under ANY_PALETTE that of the key voxel */
  uint8_t dx, dy, dz;            /* extents along x, y, z minus 1 */
} DustHipBox;
typedef struct DustHipBoxesResult {    /* 64 bytes */
  uint32_t boxes;                /* number of boxes */
  uint32_t rects;                /* rects of all slices: the boxes there would be without stacking */
  uint32_t voxels;               /* |S|: the sum of the boxes' volumes */
  uint8_t lo[3], pad0;           /* inclusive bounds of S; 255,255,255 when S is empty */
  uint8_t hi[3], pad1;           /* 0,0,0 when S is empty; pad bytes 0 */
  uint32_t reserved[11];         /* 0 */
} DustHipBoxesResult;
DustStatus dust_hip_model_boxes(const DustHipModel*, const DustHipBoxesQuery*, DustHipBoxesResult* result /* may be NULL */,
                                DustHipBox* boxes /* capacity; may be NULL when capacity == 0 */, uint32_t capacity);
/* Model deltas: what changed between two states of a model, as a list -- an edit replicated to clients without sending the model, an
 * undo / redo stack, an incremental save, the voxels a blast removed as particles of the right materials -- and the list handed back:
 * dust_hip_model_delta_apply plays it onto a model in either direction and says how many voxels were not in the state it assumes.
 *
 * Kinds: a voxel differs when its value differs between the two models at the same tree coordinates; a value is None or a palette
 * index 0..254. DUST_HIP_DELTA_ADDED: None before, solid after. DUST_HIP_DELTA_REMOVED: solid before, None after.
 * DUST_HIP_DELTA_REPAINTED: solid in both, the palette index differs. The two palettes' colours are not compared, only indices.
 * Query: DustHipSurfaceQuery's layout with `kinds` where `faces` stands. palette -1: every change; 0..254: only voxels whose value
 * before or after is that index. lo / hi is an inclusive voxel box under the surface query's rules: clipped to the tree, lo > hi on
 * an axis legal and empty -- the zero result (bounds 255 / 0), nothing written.
 * Listed: a voxel is listed when it lies inside the clipped region, differs, its kind is among query.kinds and it passes the palette
 * filter.
 * Record: key is x << 16 | y << 8 | z; kind the one DUST_HIP_DELTA_* bit; before and after a palette index 0..254 or
 * DUST_HIP_DELTA_NONE (255, free because models that hold material byte 255 are unsupported); reserved 0. The device writes a record
 * as one 64-bit word.
 * Order and capacity: the records come in ascending brick code (leaf_code: Tree::iter_leaf, the order in which dust_hip_model_read
 * lists any model's blocks), then ascending voxel bit (x&3)<<4 | (y&3)<<2 | (z&3). The first min(result.voxels, capacity) records are
 * written; the slots past them are left untouched. result.voxels is the full count whatever the capacity; capacity 0 counts only
 * (dust_hip_model_surface's convention).
 * Result: voxels, the listed voxels; added, removed, repainted, which sum to voxels; solid_before and solid_after, the solid voxels
 * of each model inside the clipped region, whatever the kinds and the filter; lo / hi, the inclusive bounds of the listed voxels
 * (255, 255, 255 / 0, 0, 0 when there is none); pad and reserved bytes 0.
 * Tables: counts[0 * 256 + b] is the number of listed voxels whose value before has bin b, counts[1 * 256 + b] the same for the value
 * after; bin 0 is None and bin 1 + p palette index p (dust_hip_model_census's convention). Each row sums to result.voxels; row 0 bin 0
 * equals added, row 1 bin 0 equals removed.
 * dust_hip_model_delta only reads both models, with dust_hip_model_surface's guarantees: one that is not editable stays not editable
 * (its blocks' masks are scattered into a 2 MiB scratch of the context, and it is expanded into a 16 MiB scratch grid only when a
 * byte is needed: REPAINTED among the kinds, a palette filter, tables, a list; the context has one pair of each, and a second one from
 * the first call in which neither model is editable); generations do not move, so committed scenes stay valid; island labellings and
 * both fields stand. before == after, the same handle, is legal and gives the zero result.
 * dust_hip_model_delta_apply walks records[0..n) and reads key, before and after; kind and reserved are ignored. With flags 0 a voxel
 * takes `after` and is expected to hold `before`; with DUST_HIP_DELTA_BACKWARD it takes `before` and is expected to hold `after`. A
 * key named more than once keeps its last record (set_voxels' rule). *conflicts is the number of surviving records whose voxel did not
 * hold the expected value, judged on the model as it stood when the call began; those records are applied all the same. *changed is
 * the number of voxels whose value differs afterwards. The model is rebuilt as after surface_apply, byte for byte a host build; the
 * generation is bumped, the island labelling and both fields are invalid afterwards. n == 0 is a no-op that may make the model
 * editable, as with set_voxels.
 * Refused with DUST_ERR_INVALID_ARGUMENT, every output untouched: a null model or query; models of two contexts; a struct_size below
 * the struct's size; kinds of 0 or above 7; any flag bit for delta, a bit above 0 for delta_apply; a palette below -1 or above 254; a
 * region coordinate >= 256; null voxels with capacity > 0; null records with n > 0; n above 16 777 216; a record key >= 2^24.
 * DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material byte 255), for either model,
 * before the query is looked at. Both calls are synchronous, like every model call. Everything is integer arithmetic: two runs give
 * the same bytes.
 * Out of scope: an offset or orientation between the two models (stamp's job); a device-side copy of a model (a snapshot today is an
 * empty model with one OVERWRITE stamp of the whole tree); run-length or otherwise packed deltas; 4096^3 trees; an asynchronous
 * form; a strict apply that changes nothing on a conflict. */
#define DUST_HIP_DELTA_ADDED 1u
#define DUST_HIP_DELTA_REMOVED 2u
#define DUST_HIP_DELTA_REPAINTED 4u
#define DUST_HIP_DELTA_ALL 7u
#define DUST_HIP_DELTA_NONE 255u      /* a record's before / after: no voxel */
#define DUST_HIP_DELTA_BACKWARD 1u    /* delta_apply flags: voxels take `before` and are expected to hold `after` */
#define DUST_HIP_DELTA_BINS 256u
#define DUST_HIP_MAX_DELTA_RECORDS 16777216u
typedef struct DustHipDeltaQuery {     /* 48 bytes, DustHipSurfaceQuery's layout */
  uint32_t struct_size;
  uint32_t kinds;                /* 1..7: the DUST_HIP_DELTA_* kinds that count */
  uint32_t flags;                /* 0 */
  int32_t palette;               /* -1: every change; 0..254: only voxels whose value before or after is this palette index */
  uint32_t lo[3], hi[3];         /* inclusive region, clipped to the tree */
  uint32_t reserved[2];          /* 0 */
} DustHipDeltaQuery;
typedef struct DustHipDeltaResult {    /* 64 bytes */
  uint32_t voxels;               /* listed voxels */
  uint32_t added, removed, repainted;  /* ... per kind; they sum to voxels */
  uint32_t solid_before;         /* solid voxels of `before` in the clipped region, whatever the kinds and the filter */
  uint32_t solid_after;          /* ... of `after` */
  uint8_t lo[3], pad0;           /* inclusive bounds of the listed voxels; 255,255,255 when there is none */
  uint8_t hi[3], pad1;           /* 0,0,0 when there is none; pad bytes 0 */
  uint32_t reserved[8];          /* 0 */
} DustHipDeltaResult;
typedef struct DustHipDeltaVoxel {     /* 8 bytes */
  uint32_t key;                  /* x << 16 | y << 8 | z */
  uint8_t kind;                  /* the one DUST_HIP_DELTA_* bit */
  uint8_t before;                /* palette index 0..254, or DUST_HIP_DELTA_NONE */
  uint8_t after;                 /* palette index 0..254, or DUST_HIP_DELTA_NONE */
  uint8_t reserved;              /* 0 */
} DustHipDeltaVoxel;
DustStatus dust_hip_model_delta(const DustHipModel* before, const DustHipModel* after, const DustHipDeltaQuery*,
                                DustHipDeltaResult* result /* may be NULL */,
                                DustHipDeltaVoxel* voxels /* capacity; may be NULL when capacity == 0 */, uint32_t capacity,
                                uint32_t* counts /* 2 * 256, may be NULL */);
DustStatus dust_hip_model_delta_apply(DustHipModel*, const DustHipDeltaVoxel* records, uint32_t n, uint32_t flags,
                                      uint32_t* changed /* may be NULL */, uint32_t* conflicts /* may be NULL */);
/* Model columns: the 2.5-D view of a model -- for every voxel column along an axis, where the solid starts, how thick it is and what
 * lies behind it: the height of the ground at (x, z) for spawning and placing, a heightfield collider, a minimap or an orthographic
 * thumbnail (height plus the palette of the top voxel), sky exposure (snow, rain and sunlight reach a voxel only when nothing is above
 * it), the ceiling and the floor of the cave under an overhang (the second layer), and the oldest terrain edit there is: the top
 * voxel becomes grass, the three below it dirt.
 *
 * Side and axis: query.face names exactly one DUST_HIP_FACE_* bit, the side the columns are looked at FROM. DUST_HIP_FACE_POS_Y looks
 * down from above: a column is walked from hi[1] down to lo[1]; DUST_HIP_FACE_NEG_Y looks up from below, from lo[1] up to hi[1]; the
 * other axes work alike. "Near" is the end the walk starts at.
 * Region: lo / hi is an inclusive voxel box, clipped to the tree (a coordinate above 255 is cut back to 255); lo > hi on an axis is
 * legal and empty. Unlike dust_hip_model_surface, voxels outside the region do not exist for this call: a run is cut at the region's
 * faces, and nothing outside is consulted.
 * Counted voxel: with palette -1 every solid voxel; with palette 0..254 only voxels of that index -- every other voxel, solid or
 * not, is see-through.
 * Run: a maximal stretch of consecutive counted voxels in a column, numbered 0, 1, 2, ... from the near end; a column of 256 voxels
 * has at most 128. Gap of run k: the stretch of not-counted voxels between run k - 1 (or the near region face) and run k; it may be
 * empty. Layer: query.layer (0..255) selects run `layer` of every column; a column with fewer runs is a miss.
 * Map: one DustHipColumnCell per column of the clipped region, row-major [v][u] with u fastest; u / v are dust_hip_model_mesh's axes:
 * u = z and v = y for the x sides, u = z and v = x for the y sides, u = y and v = x for the z sides. at is the coordinate, on the
 * axis, of the run's nearest voxel; palette that voxel's index 0..254, or 255 for a miss (then at = length_minus_1 = 0);
 * length_minus_1 the run length 1..256 minus one; runs the number of runs of the whole column, valid for a miss too. The device writes
 * a cell as one 32-bit word.
 * Result, all of it defined for the empty region as well: columns, the columns of the clipped region; hit, those that have the layer;
 * voxels, the sum of the listed runs' lengths; runs, the sum of every column's run count; depth_sum, the sum over the hit columns of
 * the number of voxels between the near region face and `at` (the mean height is depth_sum / hit); nearest_key and farthest_key, the
 * key x << 16 | y << 8 | z of the hit voxel (a listed run's nearest voxel) with the smallest and with the largest depth, among equals
 * the lowest key, DUST_HIP_COLUMNS_NO_KEY without a hit; lo / hi, the inclusive bounds of the hit voxels (255, 255, 255 / 0, 0, 0
 * when there is none, as in DustHipSurfaceResult); pad and reserved 0.
 * cells may be NULL: counts only. Otherwise capacity, counted in cells, must be at least result.columns; a smaller one is refused and
 * nothing is written. counts may be NULL; otherwise DUST_HIP_COLUMNS_BINS words: bin 0 the missed columns, bin 1 + p the hit columns
 * whose nearest voxel has palette index p (dust_hip_model_census's bins); the table sums to columns.
 * dust_hip_model_columns only reads the model, with dust_hip_model_surface's guarantees: one that is not editable stays not editable
 * (its blocks' masks are scattered into the context's 2 MiB scratch as for a cast's source, and it is expanded into the 16 MiB
 * scratch grid only when a grid byte is needed: a palette filter, a map, the table); the generation does not move; the island
 * labelling and both fields stand.
 * dust_hip_model_columns_apply, decided on the model as it stood when the call began, in every column that has the layer: with
 * DUST_HIP_COLUMNS_RUN the nearest min(depth, length) voxels of the run take `value`; with DUST_HIP_COLUMNS_GAP the min(depth, gap
 * length) voxels of the gap that lie directly in front of the run take `value`, whatever they hold. depth is 1..256; value -1 for
 * None or a palette index 0..254; *changed the number of voxels whose value changed. The model is then made editable and rebuilt
 * exactly as after dust_hip_model_surface_apply, byte for byte a host build; the generation is bumped, the island labelling and both
 * fields are invalid afterwards. With DUST_HIP_FACE_POS_Y and layer 0: RUN 1 grass, then RUN 4 under a stone filter, is grass over
 * dirt; GAP 1 snow is snow only under open sky; RUN 256 None peels the top layer off; GAP 256 water with the region's hi[1] at sea
 * level fills to sea level from above and stops at the first roof.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything happens, every output untouched: a null model or query; a struct_size below
 * the struct's size; a face that is not a single bit below 64; a non-zero flag or reserved word; a palette below -1 or above 254; a
 * layer above 255; a capacity below result.columns with cells given; a where above DUST_HIP_COLUMNS_GAP; a depth of 0 or above 256; a
 * value below -1 or above 254. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material
 * byte 255), before the query is looked at. Both calls are synchronous, like every model call. Everything is integer arithmetic: two
 * runs give the same bytes.
 * Out of scope: columns across the instances of a scene in world space; walls (the outside of the tree as solid); arbitrary
 * directions; 4096^3 trees; an asynchronous form; more than one layer per call. */
#define DUST_HIP_COLUMNS_RUN 0u        /* columns_apply where: the nearest voxels of the run */
#define DUST_HIP_COLUMNS_GAP 1u        /* ... the voxels of the gap directly in front of the run */
#define DUST_HIP_COLUMNS_BINS 256u
#define DUST_HIP_COLUMNS_NO_KEY 0xFFFFFFFFu
typedef struct DustHipColumnsQuery {   /* 48 bytes, DustHipSurfaceQuery's layout */
  uint32_t struct_size;
  uint32_t face;                 /* exactly one DUST_HIP_FACE_* bit: the side the columns are looked at from */
  uint32_t flags;                /* 0 */
  int32_t palette;               /* -1: every solid voxel counts; 0..254: only voxels of this palette index */
  uint32_t lo[3], hi[3];         /* inclusive region, clipped to the tree */
  uint32_t layer;                /* 0..255: the run of every column that is asked for */
  uint32_t reserved;             /* 0 */
} DustHipColumnsQuery;
typedef struct DustHipColumnsResult {  /* 64 bytes */
  uint32_t columns;              /* columns of the clipped region */
  uint32_t hit;                  /* ... that have the layer */
  uint32_t voxels;               /* the sum of the listed runs' lengths */
  uint32_t runs;                 /* the sum of every column's run count */
  uint32_t depth_sum;            /* the sum over hit columns of the voxels between the near region face and `at` */
  uint32_t nearest_key;          /* x << 16 | y << 8 | z of the hit voxel with the smallest depth; DUST_HIP_COLUMNS_NO_KEY without a hit */
  uint32_t farthest_key;         /* ... with the largest depth */
  uint8_t lo[3], pad0;           /* inclusive bounds of the hit voxels; 255,255,255 when there is none */
  uint8_t hi[3], pad1;           /* 0,0,0 when there is none; pad bytes 0 */
  uint32_t reserved[7];          /* 0 */
} DustHipColumnsResult;
typedef struct DustHipColumnCell {     /* 4 bytes */
  uint8_t at;                    /* the coordinate on the axis of the run's nearest voxel; 0 for a miss */
  uint8_t palette;               /* that voxel's palette index 0..254; 255 for a miss */
  uint8_t length_minus_1;        /* the run's length 1..256, minus one; 0 for a miss */
  uint8_t runs;                  /* the runs of the whole column, 0..128 */
} DustHipColumnCell;
DustStatus dust_hip_model_columns(const DustHipModel*, const DustHipColumnsQuery*, DustHipColumnsResult* result /* may be NULL */,
                                  DustHipColumnCell* cells /* capacity >= result.columns; may be NULL: counts only */, uint32_t capacity,
                                  uint32_t* counts /* 256, may be NULL */);
DustStatus dust_hip_model_columns_apply(DustHipModel*, const DustHipColumnsQuery*, uint32_t where, uint32_t depth, int32_t value,
                                        uint32_t* changed /* may be NULL */);
/* Model neighbourhoods: a voxel decided from how many of its neighbours are solid -- the one-voxel spikes taken off and the one-voxel
 * pits filled round a crater, specks removed and pinholes closed, caves and rough terrain from a random fill (the "4-5 rule" family,
 * run for a handful of generations), moss, fire, rot or crystal spreading by contact, one ring per generation, in the material most
 * neighbours carry.
 *
 * Neighbourhood: query.neighbourhood is DUST_HIP_NEIGHBOURS_FACES (6: the offsets with |d|1 == 1), DUST_HIP_NEIGHBOURS_EDGES (18:
 * |d|1 <= 2 within the 3^3 box) or DUST_HIP_NEIGHBOURS_CORNERS (26: the 3^3 box without its centre). A voxel's count n is the number
 * of solid voxels at those offsets. A neighbour outside the tree is empty, or solid under DUST_HIP_NEIGHBOURS_WALLS (the convention
 * of DUST_HIP_SURFACE_WALLS).
 * Birth and survival: query.birth and query.survive are bit masks over n. An empty voxel with bit n of birth set becomes solid; a
 * solid voxel with bit n of survive clear becomes empty; every other voxel keeps its value, and survivors keep their material. All
 * voxels of a generation are decided on the model as it stood before that generation: a synchronous update.
 * Material of a born voxel: query.palette (0..254). Under DUST_HIP_NEIGHBOURS_MAJORITY it takes the palette index that most of its
 * solid neighbours in the same neighbourhood carry, the lowest index among equals (dust_hip_model_reduce's tie rule). Walls carry no
 * material and do not vote; where no neighbour votes (bit 0 of birth, or only walls were counted) the fallback is query.palette.
 * Region: lo / hi is an inclusive voxel box under dust_hip_model_surface's rules. Only voxels inside it are counted or changed;
 * neighbours outside it, but inside the tree, are consulted as they are, in every generation. lo > hi on an axis is legal and empty:
 * the zero result (bounds 255 / 0), and an apply that changes nothing.
 * Result (dust_hip_model_neighbours): voxels, the voxels of the clipped region; solid, the solid ones; born and died, what ONE
 * generation of the query's rule would do -- ask first, apply after; lo / hi, the inclusive bounds of the voxels that would change
 * (255, 255, 255 / 0, 0, 0 when there is none); pad and reserved 0.
 * Table: counts[n] is the number of empty voxels of the region with n neighbours, counts[27 + n] the same for the solid ones; bins
 * above the neighbourhood's size are 0; the two rows sum to voxels - solid and to solid.
 * Applied (dust_hip_model_neighbours_apply): generations, 1 + the index of the last generation that changed a voxel, 0 when none did;
 * solid_before and solid_after, the region's solid voxels; born and died, the sums over all generations (64 bits: 256 generations of
 * 16.7 M voxels do not fit 32); lo / hi, the bounds of every voxel born or killed in any generation; pad and reserved 0.
 * per_generation[2 g] and per_generation[2 g + 1] are the born and the died of generation g; the rows after a fixed point are 0.
 * Generations: 1..256. The library may stop launching once a generation changed nothing; how often it looks does not show in any
 * output. A rule that oscillates simply runs all its generations.
 * dust_hip_model_neighbours only reads the model, with dust_hip_model_surface's guarantees and a stronger one: it needs no grid byte at
 * all. One that is not editable stays not editable (its blocks' masks are scattered into the context's 2 MiB scratch as for a cast's
 * source) and is never expanded; the generation does not move; the island labelling and both fields stand.
 * dust_hip_model_neighbours_apply makes the model editable as every apply does, runs the generations on the device between the
 * model's grid and the context's scratch grid, and then rebuilds ONCE as after dust_hip_model_surface_apply, byte for byte a host
 * build. The generation is bumped and the island labelling and both fields are invalid afterwards, even when nothing changed (as
 * after dust_hip_model_columns_apply).
 * Refused with DUST_ERR_INVALID_ARGUMENT, the outputs untouched: a null model or query; a struct_size below the struct's size; a
 * neighbourhood other than 6, 18 or 26; an unknown flag bit; a palette outside 0..254; a birth or survive bit above the
 * neighbourhood's size; a region coordinate >= 256; generations of 0 or above 256. A null per_generation is fine.
 * DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material byte 255), before the query is
 * looked at. Both calls are synchronous, like every model call. Everything is integer arithmetic: two runs give the same bytes.
 * Out of scope: a list of the voxels that would change; radius above 1, weighted or asymmetric neighbourhoods; rules that count only
 * one material; asynchronous (sequential-sweep) updates; neighbourhoods across the instances of a scene; 4096^3 trees; an
 * asynchronous form; a brick worklist between generations. */
#define DUST_HIP_NEIGHBOURS_FACES 6u
#define DUST_HIP_NEIGHBOURS_EDGES 18u
#define DUST_HIP_NEIGHBOURS_CORNERS 26u
#define DUST_HIP_NEIGHBOURS_WALLS 1u     /* flags: the outside of the tree counts as solid (DUST_HIP_SURFACE_WALLS) */
#define DUST_HIP_NEIGHBOURS_MAJORITY 2u  /* flags: a born voxel takes the palette index most of its solid neighbours carry */
#define DUST_HIP_NEIGHBOURS_BINS 27u
#define DUST_HIP_NEIGHBOURS_MAX_GENERATIONS 256u
typedef struct DustHipNeighboursQuery {   /* 48 bytes, DustHipSurfaceQuery's layout */
  uint32_t struct_size;
  uint32_t neighbourhood;        /* DUST_HIP_NEIGHBOURS_FACES, _EDGES or _CORNERS */
  uint32_t flags;                /* DUST_HIP_NEIGHBOURS_WALLS | DUST_HIP_NEIGHBOURS_MAJORITY or 0 */
  int32_t palette;               /* 0..254: what a born voxel takes (under MAJORITY: where nobody votes) */
  uint32_t lo[3], hi[3];         /* inclusive region, clipped to the tree */
  uint32_t birth;                /* bit n: an empty voxel with n solid neighbours becomes solid */
  uint32_t survive;              /* bit n: a solid voxel with n solid neighbours stays */
} DustHipNeighboursQuery;
typedef struct DustHipNeighboursResult {  /* 64 bytes */
  uint32_t voxels;               /* voxels of the clipped region */
  uint32_t solid;                /* ... that are solid */
  uint32_t born, died;           /* what one generation of the query's rule would do */
  uint8_t lo[3], pad0;           /* inclusive bounds of the voxels that would change; 255,255,255 when there is none */
  uint8_t hi[3], pad1;           /* 0,0,0 when there is none; pad bytes 0 */
  uint32_t reserved[10];         /* 0 */
} DustHipNeighboursResult;
typedef struct DustHipNeighboursApplied { /* 64 bytes */
  uint32_t generations;          /* 1 + the index of the last generation that changed a voxel; 0 when none did */
  uint32_t solid_before;         /* the region's solid voxels before the first generation */
  uint32_t solid_after;          /* ... after the last */
  uint32_t reserved0;            /* 0 */
  uint64_t born, died;           /* sums over all generations */
  uint8_t lo[3], pad0;           /* inclusive bounds of every voxel born or killed; 255,255,255 when there is none */
  uint8_t hi[3], pad1;           /* 0,0,0 when there is none; pad bytes 0 */
  uint32_t reserved[6];          /* 0 */
} DustHipNeighboursApplied;
DustStatus dust_hip_model_neighbours(const DustHipModel*, const DustHipNeighboursQuery*, DustHipNeighboursResult* result /* may be NULL */,
                                     uint32_t* counts /* 2 * 27, may be NULL */);
DustStatus dust_hip_model_neighbours_apply(DustHipModel*, const DustHipNeighboursQuery*, uint32_t generations,
                                           DustHipNeighboursApplied* applied /* may be NULL */,
                                           uint32_t* per_generation /* 2 * generations, may be NULL */);
/* Model settling: granular material obeys gravity -- sand, gravel, snow and rubble stop hanging in the air after a crater is carved
 * under them, fall until they rest and slide down slopes steeper than 45 degrees.
 *
 * Direction: query.toward is exactly one DUST_HIP_FACE_* bit, the side things fall toward (DUST_HIP_FACE_NEG_Y: ordinary gravity). g
 * is the unit step toward that side, "above p" is p - g, and u / v are the plane axes of dust_hip_model_columns.
 * Region: lo / hi is an inclusive voxel box under dust_hip_model_neighbours' rules (a coordinate >= 256 is refused; lo > hi on an
 * axis is legal and empty). As for dust_hip_model_columns, voxels outside the region do not exist for the call: they are neither
 * consulted nor changed. The region's face on the toward side is a floor, and nothing falls in from above the region.
 * Loose and fixed: query.loose is a bit mask over the palette indices 0..254 (bit p of the 256: word p / 32, bit p % 32). A solid
 * voxel whose index has its bit set is loose; every other solid voxel is fixed. All 255 bits set: everything is loose.
 * Fall: in every voxel column of the region along the axis, with positions counted from the toward end, a loose voxel at position i
 * has a floor f, one past the highest fixed position below i (0 when there is none), and moves to f + the number of loose voxels in
 * [f, i): a stable compaction per stretch between fixed voxels. Loose voxels keep their order and their palette indices, fixed
 * voxels do not move; the voxel's fall is i - its new position.
 * Slide in a lateral direction d, decided on the model as it stood before the slide: a loose voxel at p moves to p + d + g when the
 * voxel above p is empty or outside the region and p + d and p + d + g are both inside the region and empty. A destination has one
 * possible source, and sources and destinations are disjoint: no voxel is lost or doubled and no order shows.
 * Generation k (0, 1, ...): a slide with d = +u, -u, +v, -v for k mod 4 = 0, 1, 2, 3, then a fall.
 * Result (dust_hip_model_settle): what ONE fall would do -- ask first, apply after. columns, the voxel columns of the region; loose
 * and fixed, its loose and its fixed voxels; moved, the loose voxels whose position would change; changed, the voxels that would turn
 * from solid to empty or from empty to solid (a loose voxel that takes the place of another loose voxel is not counted, whatever
 * their materials: the record is decided from the two occupancies alone, which is why an all-ones mask needs no grid byte);
 * fall_max and fall_sum over the falls; lo / hi, the inclusive bounds of the changed voxels (255, 255, 255 / 0, 0, 0 when there is
 * none); changed_columns, the columns with a moved voxel; pad and reserved 0.
 * Applied (dust_hip_model_settle_apply): one initial fall, then `generations` (0..256) generations; 0 is a plain vertical settle.
 * generations, 1 + the index of the last generation that moved a voxel, 0 when none did; first_moved, the voxels the initial fall
 * moved; loose, the region's loose voxels; slid and fell, the voxels moved by the slides and by the falls of the generations (the
 * initial fall is not in fell); fall_sum, the sum of every fall's distance, the initial fall included, the slides not; lo / hi, the
 * bounds of every voxel that turned solid or empty in any step. per_generation[2 k] and [2 k + 1] are the slid and the fell of
 * generation k; the rows after a fixed point are 0. With s(M) the sum over the loose voxels of their position along the fall
 * (counted from the toward end), s(before) - s(after) == fall_sum + slid: every fall of n takes n off, every slide takes 1.
 * The library may stop launching once four consecutive generations (one per direction) moved nothing; how often it looks does not
 * show in any output.
 * dust_hip_model_settle only reads the model, with dust_hip_model_surface's guarantees: one that is not editable stays not editable
 * and is expanded into the context's scratch grid only when a grid byte is needed, that is when loose is not all-ones; the
 * generation does not move; the island labelling and both fields stand.
 * dust_hip_model_settle_apply makes the model editable as every apply does, runs the steps on the device -- falls in place, slides
 * between the model's grid and the context's scratch grid -- and then rebuilds ONCE as after dust_hip_model_neighbours_apply, byte
 * for byte a host build. The generation is bumped and the island labelling and both fields are invalid afterwards, even when nothing
 * moved.
 * Refused with DUST_ERR_INVALID_ARGUMENT, the outputs untouched: a null model or query; a struct_size below the struct's size; a
 * toward that is not exactly one face bit; a flags or reserved word that is not 0; a region coordinate >= 256; loose bit 255;
 * generations above 256. A null result, applied or per_generation is fine. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it
 * (4096^3 trees, models that hold material byte 255), before the query is looked at. Both calls are synchronous, like every model
 * call. Everything is integer arithmetic and every step is synchronous: two runs give the same bytes.
 * Out of scope: angles of repose other than 45 degrees; liquids; settling across the instances of a scene; 4096^3 trees; an
 * asynchronous form; a brick worklist between generations. */
#define DUST_HIP_SETTLE_MAX_GENERATIONS 256u
typedef struct DustHipSettleQuery {    /* 72 bytes */
  uint32_t struct_size;
  uint32_t toward;               /* exactly one DUST_HIP_FACE_* bit: the side loose voxels fall toward */
  uint32_t flags;                /* 0 */
  uint32_t reserved;             /* 0 */
  uint32_t lo[3], hi[3];         /* inclusive region */
  uint32_t loose[8];             /* bit p: palette index p is loose; bit 255 must be 0 */
} DustHipSettleQuery;
typedef struct DustHipSettleResult {   /* 64 bytes: what ONE fall would do -- ask first, apply after */
  uint32_t columns, loose, fixed;      /* columns of the region; its loose and its fixed voxels */
  uint32_t moved;                /* loose voxels whose position would change */
  uint32_t changed;              /* voxels that would turn solid or empty */
  uint32_t fall_max;             /* the longest fall, 0..255 */
  uint64_t fall_sum;             /* the sum of all falls */
  uint8_t lo[3], pad0, hi[3], pad1;    /* bounds of the changed voxels; 255,255,255 / 0,0,0 when none */
  uint32_t changed_columns;      /* columns with at least one moved voxel */
  uint32_t reserved[5];          /* 0 */
} DustHipSettleResult;
typedef struct DustHipSettleApplied {  /* 64 bytes */
  uint32_t generations;          /* 1 + the index of the last generation that moved a voxel; 0 when none did */
  uint32_t first_moved;          /* voxels moved by the initial fall */
  uint32_t loose, reserved0;     /* the region's loose voxels; 0 */
  uint64_t slid, fell;           /* sums over the generations (the initial fall is not in fell) */
  uint64_t fall_sum;             /* the sum of every fall's distance, the initial fall included; slides are not */
  uint8_t lo[3], pad0, hi[3], pad1;    /* bounds of every voxel that turned solid or empty in any step */
  uint32_t reserved[4];          /* 0 */
} DustHipSettleApplied;
DustStatus dust_hip_model_settle(const DustHipModel*, const DustHipSettleQuery*, DustHipSettleResult* result /* may be NULL */);
DustStatus dust_hip_model_settle_apply(DustHipModel*, const DustHipSettleQuery*, uint32_t generations /* 0..256 */,
                                       DustHipSettleApplied* applied /* may be NULL */,
                                       uint32_t* per_generation /* 2 * generations: slid, fell; may be NULL; rows after a fixed point 0 */);
/* Model voxelisation: triangles to voxels on the device -- an imported prop, a CSG result, a physics hull, the quads dust_hip_model_mesh
 * itself handed out. The siblings of dust_hip_model_edit_shapes, and the inverse of dust_hip_model_mesh. Two calls:
 *   dust_hip_model_edit_triangles  SURFACE: the voxels each triangle touches, triangle by triangle, in order, an op and a palette index
 *                                  per triangle;
 *   dust_hip_model_fill_mesh       SOLID: the voxels whose centres lie inside a closed triangle mesh, one op and palette index for all.
 *
 * Coordinates: INTEGERS, in units of 1 / DUST_HIP_TRIANGLE_UNIT = 1/256 voxel of the model's tree coordinates. Voxel (x, y, z) is the
 * cube [256 x, 256 x + 256]^3, its centre (256 x + 128, 256 y + 128, 256 z + 128). Both rules are EXACT: every predicate below is a
 * sign test on 64-bit integers that cannot overflow (every intermediate stays below 2^60), so the device, a host and a witness agree
 * on every voxel, not within a voxel. Float vertices are not taken: the caller rounds (the Python binding: rint(v * 256)).
 * Common to both calls. With e1 = v1 - v0 and e2 = v2 - v0 the normal is n = e1 x e2. A triangle with n == 0, or with any |coordinate|
 * above DUST_HIP_TRIANGLE_MAX_COORD = 2^18 (+-1024 voxels), covers nothing: changed[i] = 0, it is not live, and that is not an error.
 * Triangles are clipped to the tree; vertices may lie outside it, negative coordinates included. reserved is ignored.
 *
 * Surface rule (edit_triangles). Triangle i covers voxel (x, y, z) iff the closed triangle and the closed cube share a point, decided by
 * the 13-axis separating-axis test on integers: the axes (1,0,0), (0,1,0), (0,0,1), n, and e x u for the three edges e (v0->v1, v1->v2,
 * v2->v0) and the three unit axes u. An axis a separates the pair iff max over k of dot(a, v_k) < min over the cube's corners c of
 * dot(a, c), or min over k of dot(a, v_k) > max over the corners of dot(a, c). The inequalities are strict, so touching covers: a
 * triangle lying exactly on a voxel face covers the voxels on both sides, one that meets a cube at only a corner or an edge covers it.
 * The voxel is covered iff no axis separates. Thin (6-separating) surfaces are not offered.
 * Operations on a covered voxel are edit_shapes' (DUST_HIP_EDIT_CARVE, _FILL, _PAINT, _PLACE), per triangle. Order: the triangles of a
 * call apply in array order, as n successive calls would. changed[i] is counted as edit_shapes counts it: the voxels whose value after
 * triangle i differs from their value before it. Deterministic: two runs give the same bytes and the same counts. `changed` may be NULL.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything changes: a null model; null triangles with n > 0; n >
 * DUST_HIP_MAX_EDIT_TRIANGLES; an unknown op; a palette outside 0..254 on an op that uses it. n == 0 is a no-op, whatever the arrays (it
 * may move the model into its editable form). DUST_ERR_UNSUPPORTED exactly where edit_shapes returns it: 4096^3 trees, and models that
 * hold material byte 255.
 *
 * Solid rule (fill_mesh). A voxel of the region is inside iff an odd number of triangles is CROSSED above its centre c = (px, py, cz).
 * For one triangle let s = sign(n.z). If s == 0 the triangle crosses nothing. Otherwise it is crossed above c iff both hold:
 *   Column test: for each edge a -> b in the order v0->v1, v1->v2, v2->v0, with d = s * (b - a) in xy and
 *     E = d.x * (py - a.y) - d.y * (px - a.x): E > 0, or E == 0 and (d.y > 0, or d.y == 0 and d.x < 0), for every edge.
 *   Height test: s * dot(n, c - v0) < 0. A centre exactly on the plane is not crossed.
 * The rule does not depend on the winding or on the order of the triangles, and a column centre on an edge or a vertex shared by several
 * triangles is counted for exactly the right ones: a closed mesh fills its inside, whatever passes through column centres. A triangle's
 * own op and palette are ignored and not validated; query.op and query.palette apply to the inside voxels of the region (edit_shapes'
 * operations). An OPEN mesh still gives a deterministic answer, the parity above, and nothing more is promised for it; open meshes are
 * not repaired. The ray axis is z; there is no choice of axis. Two runs give the same bytes.
 * Region: query.lo .. query.hi, inclusive, clipped to the tree as dust_hip_model_columns clips it (a coordinate past 255 is cut back to
 * 255); lo > hi on an axis is the empty region: nothing is looked at, the triangles included, and the result is the zero result with
 * bounds 255 / 0. Voxels outside the region are neither consulted nor changed.
 * Result: covered, the voxels of the region inside the mesh; changed, those whose value changed; live, the triangles in range and not
 * degenerate; crossing, those of them with n.z != 0 (vertical triangles cross nothing); lo / hi, the bounds of the covered voxels,
 * 255 / 0 when there are none. `result` may be NULL.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything changes, in this order: a null model; (DUST_ERR_UNSUPPORTED for the model's
 * kind, as above, before the query is looked at); a null query; a struct_size below this library's; null triangles with n > 0; n >
 * DUST_HIP_MAX_MESH_TRIANGLES; an unknown query.op; a query.palette outside 0..254 on an op that uses it; a flag; a reserved word not 0.
 * n == 0 is a no-op that may make the model editable; the result is the zero result. The empty region is the same no-op: the model
 * is not rebuilt, and its island labelling and its fields stand.
 *
 * Both calls are synchronous, like edit_shapes: they return with the model rebuilt -- the device arrays byte for byte what
 * dust_hip_model_create builds from the same voxels -- and the outputs written; whatever edit_shapes invalidates (the island labelling,
 * the flood and distance fields) they invalidate. Scenes that instance the model must be committed again; until then frames and queries
 * answer DUST_ERR_NOT_READY.
 * Out of scope: thin (6-separating) surfaces; float vertices in the ABI; count-only dry runs; a choice of ray axis; repairing open
 * meshes; 4096^3 trees; asynchronous forms; texture or colour sampling. */
#define DUST_HIP_TRIANGLE_UNIT 256            /* vertex units per voxel; voxel (x,y,z) is [256x, 256x+256]^3, centre 256x+128 */
#define DUST_HIP_TRIANGLE_MAX_COORD 262144    /* |coordinate| <= 2^18 units (+-1024 voxels); beyond: the triangle covers nothing */
#define DUST_HIP_MAX_EDIT_TRIANGLES 65536u
#define DUST_HIP_MAX_MESH_TRIANGLES 1048576u
typedef struct DustHipTriangle {      /* 48 bytes */
  int32_t v[3][3];                    /* three vertices, x y z, in 1/256 voxel of the model's tree coordinates */
  uint32_t op; int32_t palette;       /* DUST_HIP_EDIT_*; palette 0..254 where the op uses it (fill_mesh ignores both) */
  uint32_t reserved;                  /* ignored */
} DustHipTriangle;
DustStatus dust_hip_model_edit_triangles(DustHipModel*, const DustHipTriangle* triangles, uint32_t n,
                                         uint32_t* changed /* n entries, may be NULL */);
typedef struct DustHipFillMeshQuery {  /* 48 bytes */
  uint32_t struct_size, op;           /* sizeof(DustHipFillMeshQuery); DUST_HIP_EDIT_* */
  int32_t palette;                    /* 0..254 where the op uses it */
  uint32_t flags;                     /* 0 */
  uint32_t lo[3], hi[3];              /* inclusive region, clipped to the tree as dust_hip_model_columns clips it; lo > hi: nothing */
  uint32_t reserved[2];               /* 0 */
} DustHipFillMeshQuery;
typedef struct DustHipFillMeshResult { /* 48 bytes */
  uint32_t covered, changed;          /* voxels of the region inside the mesh; those whose value changed */
  uint32_t live, crossing;            /* triangles in range and not degenerate; of those, with n.z != 0 */
  uint32_t lo[3], hi[3];              /* bounds of the covered voxels, 255 / 0 when none */
  uint32_t reserved[2];               /* 0 */
} DustHipFillMeshResult;
DustStatus dust_hip_model_fill_mesh(DustHipModel*, const DustHipTriangle* triangles, uint32_t n, const DustHipFillMeshQuery*,
                                    DustHipFillMeshResult* result /* may be NULL */);
/* Model fracture: BREAKING A SOLID INTO PIECES. edit_shapes carves a crater, find_islands and detach_islands lift out what it cut
 * loose, settle drops it, cast and stamp land it, delta replicates it -- but a wall that is hit stays one island. Fracture scatters seed
 * points and gives every solid voxel to its nearest seed: a Voronoi partition, exact on integers, kept on the device with the model.
 * Four calls:
 *   dust_hip_model_fracture         labels the model's voxels with the index of their nearest seed and describes the cells;
 *   dust_hip_model_fracture_at      reads labels at coordinates, as flood_at reads steps;
 *   dust_hip_model_fracture_detach  moves the union of named cells into a model of its own, under detach_islands' contract;
 *   dust_hip_model_fracture_apply   gives the seam voxels, or every labelled voxel, a value.
 *
 * Seeds: integer voxel coordinates, int32 per axis, each in DUST_HIP_FRACTURE_SEED_MIN .. DUST_HIP_FRACTURE_SEED_MAX = -1024 .. 1279;
 * seeds may lie outside the tree. A voxel is the integer point (x, y, z). At most DUST_HIP_MAX_FRACTURE_SEEDS = 4096 seeds; n_seeds == 0
 * is legal: nothing is labelled and `solid` is still counted.
 * Metric: with scale = (sx, sy, sz), each in 1..16, d2(v, s) = sx (x - s.x)^2 + sy (y - s.y)^2 + sz (z - s.z)^2. d2 stays below 2^27 and
 * every coordinate difference below 2^11, so the device, a host and a witness agree on every voxel. Unequal scales give splinters.
 * Labelled voxels: a voxel is COUNTED when it is solid, lies inside the inclusive region lo..hi, clipped to the tree as
 * dust_hip_model_columns clips it (a coordinate past 255 is cut back to 255; lo > hi on an axis is the empty region), and query.palette
 * is -1 or the voxel holds that palette index. A counted voxel is labelled with the seed index i that minimises (d2, i)
 * lexicographically: ties go to the lowest index; duplicate seeds are legal, the later one gets nothing. With max_distance2 !=
 * DUST_HIP_FRACTURE_NO_LIMIT a counted voxel whose minimum d2 exceeds max_distance2 stays unlabelled: local damage, only the
 * neighbourhood of the impact breaks. Every other voxel holds DUST_HIP_NO_CELL.
 * A CELL is the set of voxels labelled i; it need not be connected (after a detach, find_islands on the piece splits it). A CUT FACE is
 * a face shared by two face-neighbours that are both labelled, with different cells. A SEAM voxel is a labelled voxel with a
 * face-neighbour labelled with a higher cell index: seams are one voxel thick.
 *
 * dust_hip_model_fracture makes the model editable first, exactly as flood does (scenes that instance it must then be committed again;
 * on an editable model the call changes nothing a scene reads), and leaves the labels on the device with the model -- one uint16 per
 * voxel, 32 MiB next to the flood and distance fields, allocated by the first call -- together with n_seeds. result: solid, the counted
 * voxels; labelled; cells, the seeds with at least one voxel; largest_cell and largest_voxels, the lowest index among equals, 0xFFFFFFFF
 * and 0 when cells == 0; cut_faces, each face once; max_d2, the largest d2 of a labelled voxel to its seed; lo / hi, the inclusive bounds
 * of the labelled voxels, 255 / 0 when there are none. cells[i] for every seed: voxels; cut_faces, the faces this cell shares with other
 * cells; lo / hi, 255,255,255 / 0,0,0 when empty; sum, the sums of x, y, z. The sum of cells[i].voxels equals labelled and the sum of
 * cells[i].cut_faces equals 2 * cut_faces. `result` and `cells` may be NULL; with both NULL only the labels are made. Two runs give the
 * same bytes.
 * dust_hip_model_fracture_detach: *out is a new editable model of the same context and palette that holds the voxels of the named cells
 * at the same tree coordinates, byte for byte a host build. DUST_HIP_DETACH_KEEP_SOURCE copies only; out == NULL deletes. The copy is
 * made before the carve, so a failure leaves the source intact. Duplicates and empty cells are legal; n == 0 is detach_islands' no-op
 * (*out = NULL). After a carving detach the removed voxels answer DUST_HIP_NO_CELL and the rest of the labelling STANDS. The recipe for
 * chunks: one fracture, then one KEEP_SOURCE detach per piece, then one deleting detach of all of them -- the source is rebuilt once.
 * dust_hip_model_fracture_apply: where = DUST_HIP_FRACTURE_SEAMS or DUST_HIP_FRACTURE_LABELLED; value a palette index 0..254, or -1 for
 * None. Every decision is made on the labelling as it stands; *changed is the number of voxels whose value differs afterwards; the
 * model is rebuilt as after surface_apply. Crack lines painted before the break; a one-voxel gap after which find_islands sees the
 * pieces; scorch within max_distance2.
 *
 * Validity: the cell field is invalidated by exactly what invalidates the flood field (every set_voxels, edit_shapes, stamp as
 * destination, carving detach_islands with n > 0, flood_apply, distance_apply and every other call that may change a voxel), by
 * fracture_apply, and by a fracture that fails; a second fracture replaces it. fracture leaves the island labelling and both other
 * fields standing. A carving fracture_detach invalidates the flood and distance fields as a carving detach_islands does, and the island
 * labelling too (it cuts islands apart); the cell field itself stands. fracture_apply invalidates all of them.
 * Refused with DUST_ERR_INVALID_ARGUMENT, nothing changed: a null model or query; a struct_size below sizeof(DustHipFractureQuery); null
 * seeds with n_seeds > 0; n_seeds > DUST_HIP_MAX_FRACTURE_SEEDS; a seed coordinate out of range or a seed's reserved word not 0; a scale
 * outside 1..16; a palette outside -1..254; flags or reserved words not 0; null arrays with n > 0; a lookup coordinate >= 256; a cell
 * index >= n_seeds; unknown detach flags, or KEEP_SOURCE without `out`; an unknown `where`; a value outside -1..254.
 * DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material byte 255), before anything but the
 * model pointer is looked at. DUST_ERR_NOT_READY from fracture_at, fracture_detach (n > 0) and fracture_apply without a standing
 * labelling, as flood_at answers without a field.
 * Out of scope: weighted (power) diagrams and non-integer seeds; seeds chosen by the library (a Poisson scatter); splitting a cell into
 * its connected pieces inside the call (find_islands does it); world-space or scene-level fracture; an asynchronous form; 4096^3
 * trees. */
#define DUST_HIP_MAX_FRACTURE_SEEDS 4096u
#define DUST_HIP_FRACTURE_SEED_MIN (-1024)
#define DUST_HIP_FRACTURE_SEED_MAX 1279
#define DUST_HIP_FRACTURE_MAX_SCALE 16u
#define DUST_HIP_FRACTURE_NO_LIMIT 0xFFFFFFFFu
#define DUST_HIP_NO_CELL 0xFFFFu
#define DUST_HIP_FRACTURE_SEAMS    0u   /* fracture_apply: the labelled voxels with a face-neighbour of a higher cell index */
#define DUST_HIP_FRACTURE_LABELLED 1u   /* fracture_apply: every labelled voxel */
typedef struct DustHipFractureSeed {   /* 16 bytes */
  int32_t x, y, z;                     /* voxel coordinates, -1024..1279 */
  uint32_t reserved;                   /* 0 */
} DustHipFractureSeed;
typedef struct DustHipFractureQuery {  /* 48 bytes */
  uint32_t struct_size, flags;         /* sizeof(DustHipFractureQuery); 0 */
  int32_t palette;                     /* -1: every solid voxel; 0..254: the voxels of that palette index */
  uint32_t max_distance2;              /* DUST_HIP_FRACTURE_NO_LIMIT, or the largest d2 at which a voxel is still labelled */
  uint8_t scale[3], reserved0;         /* 1..16 per axis; 0 */
  uint32_t lo[3], hi[3];               /* inclusive region, clipped to the tree; lo > hi: nothing */
  uint32_t reserved;                   /* 0 */
} DustHipFractureQuery;
typedef struct DustHipFractureResult { /* 64 bytes */
  uint32_t solid, labelled;            /* counted voxels; those that hold a cell index */
  uint32_t cells;                      /* seeds with at least one voxel */
  uint32_t largest_cell, largest_voxels; /* the lowest index among equals; 0xFFFFFFFF, 0 when cells == 0 */
  uint32_t cut_faces;                  /* each face once */
  uint32_t max_d2;                     /* the largest d2 of a labelled voxel to its seed */
  uint8_t lo[3], reserved0;            /* inclusive bounds of the labelled voxels; 255,255,255 when there are none */
  uint8_t hi[3], reserved1;            /* 0,0,0 when there are none; reserved bytes 0 */
  uint32_t reserved[7];                /* 0 */
} DustHipFractureResult;
typedef struct DustHipFractureCell {   /* 40 bytes, laid out like DustHipCensus */
  uint32_t voxels;                     /* voxels labelled with this cell */
  uint32_t cut_faces;                  /* faces this cell shares with other cells */
  uint8_t lo[3], reserved0;            /* inclusive bounds; 255,255,255 when voxels == 0 */
  uint8_t hi[3], reserved1;            /* 0,0,0 when voxels == 0; reserved bytes 0 */
  uint64_t sum[3];                     /* sums of x, of y, of z over the cell's voxels */
} DustHipFractureCell;
DustStatus dust_hip_model_fracture(DustHipModel*, const DustHipFractureQuery*, const DustHipFractureSeed* seeds, uint32_t n_seeds,
                                   DustHipFractureResult* result /* may be NULL */, DustHipFractureCell* cells /* n_seeds, may be NULL */);
DustStatus dust_hip_model_fracture_at(DustHipModel*, const uint32_t* xyz, uint16_t* cells, uint32_t n);
DustStatus dust_hip_model_fracture_detach(DustHipModel*, const uint32_t* cells, uint32_t n, uint32_t flags, DustHipModel** out /* may be NULL */);
DustStatus dust_hip_model_fracture_apply(DustHipModel*, uint32_t where, int32_t value, uint32_t* changed /* may be NULL */);
/* Model bodies: WHAT A RIGID-BODY SOLVER NEEDS OF A PIECE. find_islands and fracture say which voxels form a piece, detach lifts pieces
 * out, boxes and mesh give the colliders; a solver also needs mass, centre of mass and inertia tensor per body. One read-only call sums
 * them per GROUP of voxels, with a weight per material: a piece that is half stone and half wood has its centre where it belongs.
 *
 * Counted: a voxel COUNTS when it is solid, lies inside the inclusive region lo..hi (DustHipSurfaceQuery's rules: a coordinate >= 256
 * is refused; lo > hi on an axis is the empty region), passes the palette filter (palette -1: every solid voxel; 0..254: only voxels
 * of that palette index) and belongs to a group of the chosen kind.
 * Groups: query.group is one of
 *   DUST_HIP_BODIES_ALL        one record, key 0: every counted voxel;
 *   DUST_HIP_BODIES_MATERIALS  255 records, record p with key p: the counted voxels of palette index p;
 *   DUST_HIP_BODIES_ISLANDS    one record per island of the STANDING labelling (dust_hip_model_find_islands), in ascending key order:
 *                              number and order are exactly what a find_islands on the standing labelling would report now, islands
 *                              detached earlier excluded. An island without a counted voxel still gets its record: the zero record
 *                              with its key;
 *   DUST_HIP_BODIES_CELLS      one record per seed of the STANDING fracture (dust_hip_model_fracture), n_seeds records, key i. Voxels
 *                              that answer DUST_HIP_NO_CELL belong to no group.
 * Weights: w = weights[palette index], 255 uint16 entries, 0..65535; weights == NULL: every voxel weighs 1. A weight of 0 is legal: the
 * voxel still counts in `voxels` and the bounds.
 * Records: key; voxels, the counted voxels of the group; lo / hi, their inclusive bounds (255, 255, 255 / 0, 0, 0 when there are none);
 * mass, the sum of w; m1, the sums of w x, w y, w z; m2, the sums of w xx, w yy, w zz, w xy, w yz, w zx -- x, y, z the voxel's integer
 * coordinates, as `sum` in DustHipIsland (centre of mass = m1 / mass + 0.5). All integer and exact. Overflow bound: a sum is at most
 * 65535 * 255^2 * 2^24 < 2^56, below 2^63. With weights == NULL, voxels, lo, hi and m1 are byte for byte those of find_islands, of
 * fracture or of a whole-tree census over the same voxels. The tensor about the centre of mass with every voxel a solid unit cube:
 * C_ab = m2_ab - m1_a m1_b / mass, I_xx = C_yy + C_zz + mass / 6, I_xy = -C_xy.
 * Capacity: *n_bodies is the number of groups whatever the capacity; the first min(*n_bodies, capacity) records are written and the
 * slots past them are left untouched; capacity 0 only counts (the conventions of find_islands).
 * The model is only read: the generation does not move, the island labelling and all three fields stand. ALL and MATERIALS work on a
 * model that is not editable and leave it so, under census's guarantees (its blocks' masks are scattered into the context's 2 MiB
 * scratch, and it is expanded into the 16 MiB scratch grid only when a material is needed: weights, a palette filter, MATERIALS).
 * Synchronous, like every model call. Everything is integer arithmetic: two runs give the same bytes.
 * Refused with DUST_ERR_INVALID_ARGUMENT, the outputs untouched: a null model, query or n_bodies; a struct_size below the struct's
 * size; an unknown group; flags or reserved words not 0; a palette outside -1..254; a region coordinate >= 256; null bodies with
 * capacity > 0. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it (4096^3 trees, models that hold material byte 255), before the
 * query is looked at. DUST_ERR_NOT_READY from ISLANDS without a standing labelling and from CELLS without a standing cell field, as
 * island_of and fracture_at answer -- also on a model that is not editable, which cannot hold either.
 * Out of scope: world-space bodies over a scene's instances; float densities; groups named by a field's range; an asynchronous form;
 * 4096^3 trees. */
#define DUST_HIP_BODIES_ALL       0u
#define DUST_HIP_BODIES_MATERIALS 1u
#define DUST_HIP_BODIES_ISLANDS   2u
#define DUST_HIP_BODIES_CELLS     3u
#define DUST_HIP_BODY_WEIGHTS     255u   /* entries of a weight table, and records of a MATERIALS call */
typedef struct DustHipBodyQuery {      /* 48 bytes, DustHipSurfaceQuery's layout with `group` where `faces` stands */
  uint32_t struct_size;
  uint32_t group;                      /* DUST_HIP_BODIES_* */
  uint32_t flags;                      /* 0 */
  int32_t palette;                     /* -1: every solid voxel; 0..254: only voxels of this palette index */
  uint32_t lo[3], hi[3];               /* inclusive region; lo > hi: nothing */
  uint32_t reserved[2];                /* 0 */
} DustHipBodyQuery;
typedef struct DustHipBody {           /* 96 bytes */
  uint32_t key, voxels;                /* the group's key; its counted voxels */
  uint8_t lo[3], reserved0;            /* inclusive bounds of the counted voxels; 255,255,255 when there are none */
  uint8_t hi[3], reserved1;            /* 0,0,0 when there are none; reserved bytes 0 */
  uint64_t mass;                       /* sum of w */
  uint64_t m1[3];                      /* sums of w x, w y, w z */
  uint64_t m2[6];                      /* sums of w xx, w yy, w zz, w xy, w yz, w zx */
} DustHipBody;
DustStatus dust_hip_model_bodies(const DustHipModel*, const DustHipBodyQuery*,
                                 const uint16_t* weights /* 255, by palette index; NULL: every voxel weighs 1 */,
                                 uint32_t* n_bodies, DustHipBody* bodies /* capacity; may be NULL when capacity == 0 */,
                                 uint32_t capacity);
/* Model joints: THE CONTACT FACES BETWEEN NEIGHBOURING PIECES. fracture breaks a solid into cells, fracture_detach lifts pieces out,
 * boxes gives each piece its colliders, bodies its mass, centre and inertia; what holds the pieces together is missing: fracture's
 * cut_faces are scalars. One read-only call returns, for every pair of distinct GROUPS that share at least one voxel face, a record of
 * that contact -- the area stands for strength, the centroid is the anchor, the direction counts give the normal -- in canonical order
 * and exact. The same call answers it per material: how much stone touches wood, and where.
 *
 * Voxels: a voxel EXISTS for the call when it is solid and lies inside the inclusive region lo..hi, clipped to the tree as
 * dust_hip_model_columns clips it (a coordinate past 255 is cut back to it; lo > hi on an axis is the empty region). Nothing outside the
 * region exists, as in boxes and columns.
 * Groups: query.group is one of
 *   DUST_HIP_JOINTS_MATERIALS  the voxel's group is its palette index, 0..254;
 *   DUST_HIP_JOINTS_CELLS      the group is the cell index of the STANDING fracture (dust_hip_model_fracture), 0..4095; a solid voxel
 *                              that answers DUST_HIP_NO_CELL -- beyond max_distance2, outside the fracture's region or filter -- has
 *                              group DUST_HIP_JOINT_REST: the unbroken rest of the piece.
 * Island groups are deliberately absent: under the labelling's own connectivity two islands never share a face.
 * Faces: a face is a pair of voxels p and p + e_r, r one of x, y, z, that both exist and whose groups differ. Each face is counted once
 * and belongs to the pair (a, b) of its two groups with a < b; REST is always b. There is no neighbour across a face of the tree.
 * Records: a, b, the two group keys; faces, the faces they share; by_face, the faces by the direction FROM the a voxel TO the b voxel in
 * the order of the DUST_HIP_FACE_* bits (-x, +x, -y, +y, -z, +z), summing to faces; lo2 / hi2, the inclusive bounds of the face centres
 * in HALF voxels on the lattice 0..512; sum2, the sums of the face centres in half voxels. The centre of face (p, r) is 2 p + 1 + e_r:
 * 2 p_r + 2 along r, 2 p + 1 on the other two axes. A sum needs 64 bits: one pair can hold about 5 * 10^7 faces of coordinates up to
 * 511. A pair without faces has no record. All integer and exact. Area = faces, anchor = sum2 / (2 faces), the unnormalised normal from
 * a to b = (by_face[+x] - by_face[-x], ...). Under CELLS with the fracture's own region the faces of the records with b != REST sum to
 * the fracture result's cut_faces, and those of the records that name cell c to that cell's cut_faces.
 * Capacity: *n_joints is the number of pairs whatever the capacity; the first min(*n_joints, capacity) records in ascending (a, b) are
 * written and the bytes past them are left untouched; capacity 0 only counts. The empty region: *n_joints = 0, DUST_OK.
 * The model is only read: the generation does not move, committed scenes keep answering, the island labelling and all three fields
 * stand. MATERIALS works on a model that is not editable and leaves it so, under census's guarantees (its blocks' masks are scattered
 * into the context's 2 MiB scratch and it is expanded into the 16 MiB scratch grid). Synchronous, like every model call. Integer adds
 * and maxima, the output sorted by key: two runs give the same bytes.
 * Memory: the pairs are collected in a hash table of 80-byte slots in the context's scratch: sixteen slots per root cell of the region,
 * between 1024 and 65 536 (5 MiB for the whole tree: MATERIALS' 32 385 possible pairs at a load below one half); a table that turns
 * out too small is doubled and the pass repeated, up to 2^24 slots (1.25 GiB), which the 8 390 656 pairs of 4096 cells and REST cannot
 * fill. The sort takes 16 bytes per pair more. DUST_ERR_OUT_OF_MEMORY when the device cannot hold them.
 * Refused with DUST_ERR_INVALID_ARGUMENT, the outputs untouched: a null model, query or n_joints; a struct_size below the struct's
 * size; an unknown group; flags or reserved words not 0; a palette other than -1 (reserved for a later filter); null joints with
 * capacity > 0. DUST_ERR_UNSUPPORTED exactly where set_voxels returns it, before the query is looked at. DUST_ERR_NOT_READY from CELLS
 * without a standing cell field, as fracture_at answers -- also on a model that is not editable, which cannot hold one.
 * Out of scope: contacts with the tree's faces (find_islands' `anchored` covers the common case); edge and corner contacts; a palette
 * filter; breaking joints or solving anything on the device -- the host owns the graph. */
#define DUST_HIP_JOINTS_MATERIALS 0u
#define DUST_HIP_JOINTS_CELLS     1u
#define DUST_HIP_JOINT_REST       0xFFFFu /* the group of a solid voxel that answers DUST_HIP_NO_CELL */
typedef struct DustHipJointQuery {     /* 48 bytes, DustHipSurfaceQuery's layout with `group` where `faces` stands */
  uint32_t struct_size;
  uint32_t group;                      /* DUST_HIP_JOINTS_* */
  uint32_t flags;                      /* 0 */
  int32_t palette;                     /* -1 (reserved for a later filter) */
  uint32_t lo[3], hi[3];               /* inclusive region, clipped to the tree; lo > hi: nothing */
  uint32_t reserved[2];                /* 0 */
} DustHipJointQuery;
typedef struct DustHipJoint {          /* 80 bytes */
  uint32_t a, b;                       /* the two group keys, a < b; b may be DUST_HIP_JOINT_REST */
  uint32_t faces;                      /* shared faces */
  uint32_t reserved0;                  /* 0 */
  uint32_t by_face[6];                 /* by the direction from the a voxel to the b voxel: -x, +x, -y, +y, -z, +z */
  uint16_t lo2[3], hi2[3];             /* inclusive bounds of the face centres in half voxels */
  uint32_t reserved1;                  /* 0 */
  uint64_t sum2[3];                    /* sums of the face centres in half voxels */
} DustHipJoint;
DustStatus dust_hip_model_joints(const DustHipModel*, const DustHipJointQuery*,
                                 uint32_t* n_joints, DustHipJoint* joints /* capacity; may be NULL when capacity == 0 */,
                                 uint32_t capacity);
/* Model resampling: A STAMP UNDER ANY ROTATION, SCALE OR SHEAR. stamp, cast and delta place a piece under the 48 signed axis
 * permutations: a fallen wall segment lands at 0 or 90 degrees, never at 30; a prefab cannot be pasted at 1.5 times its size. A resample
 * is a stamp whose geometry is a fixed-point affine map from the destination to the source -- the voxels of one model pasted into
 * another, materials and all, with the stamp's five ops, its palette map, its order and its snapshot rule.
 *
 * Geometry: everything is integer. A record names an inclusive sub-box [src_lo, src_hi] of the source, an inclusive destination box
 * [dst_lo, dst_hi] and the INVERSE map: a matrix m and a translation t that take a destination position to a source position, in units
 * of 1 / DUST_HIP_RESAMPLE_ONE = 1 / 65536 voxel (16 fraction bits; m[k][r] = 65536 is 1.0). Sampling is point sampling at the
 * destination voxel's centre: for destination voxel d = (x, y, z) and each source axis k,
 *   Q[k] = m[k][0] * (2x + 1) + m[k][1] * (2y + 1) + m[k][2] * (2z + 1) + 2 * t[k],        s[k] = floor(Q[k] / 131072),
 * the division rounding toward minus infinity: Q[k] = -1 gives s[k] = -1, not 0. Limits: |m[k][r]| <= 8 * 65536 and |t[k]| <= 2^28;
 * with them |Q| <= 3 * 2^19 * 511 + 2^29 = 1 340 604 416 < 2^31, so the device computes in 32 bits. Any int32 dst_lo and dst_hi are
 * legal; the box is clipped to the tree. The image box is the set of voxels d of the clipped destination box whose s lies inside
 * [src_lo, src_hi] on all three axes. A voxel whose s lies outside is not part of the image: it keeps its value under every op,
 * REPLACE included. A singular m is legal: every destination voxel then reads one plane, line or voxel of the source. A record covers
 * nothing (all four counts 0, not an error, as a stamp's degenerate inputs) when dst_lo > dst_hi on some axis, when src_lo > src_hi on
 * some axis, or when its destination box lies wholly outside the tree.
 * Values: v is the source voxel's value at s -- None, or palette_map[index] when a map is given (255 entries, one per palette index
 * 0..254), otherwise the index itself; w is the destination voxel's. The ops are the stamp's, DUST_HIP_STAMP_PLACE .. _PAINT with the
 * same values and the same table, "image box" read as above. PLACE: v solid and w None -> v. OVERWRITE: v solid -> v. REPLACE: every
 * voxel of the image box -> v, None included. CARVE: v solid -> None. PAINT: v solid and w solid -> v. Every other voxel keeps w.
 * Counts: counts[i] (may be NULL) describes record i -- changed: voxels whose value after the record differs from their value before
 * it (the stamp's changed); covered: voxels of the image box; solid: those whose v is solid; blocked: those where v and w are both
 * solid, w the destination's value before the record.
 * With flags == 0 the call behaves as a stamp does: the records apply in array order, as n successive calls would; the source is read
 * as it stood when the call began, also when src == dst; the call is synchronous and returns with dst rebuilt -- the device arrays
 * byte for byte what dust_hip_model_create builds from the resulting voxels -- its generation bumped and, when n > 0, its island
 * labelling and every derived field (flood, distance, cells) invalidated exactly as by a stamp. The SOURCE is not modified unless it is
 * dst and is not made editable; its generation stays. Deterministic: two runs give the same bytes and the same counts.
 * DUST_HIP_RESAMPLE_DRY_RUN is the fit test for a rotated prefab: nothing is written. Every record is counted against dst as it stands,
 * independently of the others: counts[i] is what a call with records[i] alone would return, changed included; blocked == 0 means the
 * piece fits. Under a dry run dst is moved into its editable form first if it is not there yet, exactly as cast does (scenes that
 * instance it must then be committed again); otherwise its generation, its island labelling and all its fields stay.
 * Refused with DUST_ERR_INVALID_ARGUMENT before anything changes: a null dst or src; null records with n > 0;
 * n > DUST_HIP_MAX_RESAMPLES; models of different contexts; an unknown op; flag bits other than DRY_RUN; an m or t beyond its limit; a
 * palette_map entry above 254. n == 0 is a no-op in the set_voxels sense (it may move dst into its editable form).
 * DUST_ERR_UNSUPPORTED exactly where stamp returns it (4096^3 trees, models that hold material byte 255), for dst and for src alike,
 * before the records are looked at.
 * The result is defined by the integer record, not by whatever float matrix it was rounded from.
 * Out of scope: filtered sampling (shrinking drops thin features; dust_hip_model_reduce is the tool for whole levels); float matrices
 * in the ABI; perspective maps; 4096^3 trees; an asynchronous form; a rotating cast. */
#define DUST_HIP_RESAMPLE_ONE     65536   /* 1.0 in DustHipResample.m and .t */
#define DUST_HIP_RESAMPLE_MAX_M   (8 * 65536)
#define DUST_HIP_RESAMPLE_MAX_T   (1 << 28)
#define DUST_HIP_RESAMPLE_DRY_RUN 1u      /* flags: count, write nothing */
#define DUST_HIP_MAX_RESAMPLES    65536u
typedef struct DustHipResample {     /* 96 bytes */
  int32_t  m[3][3];                  /* the inverse map's matrix: destination -> source, 1 / 65536 per unit */
  int32_t  t[3];                     /* its translation, in 1 / 65536 voxel */
  int32_t  dst_lo[3], dst_hi[3];     /* inclusive destination box, clipped to the tree */
  uint8_t  src_lo[3], pad0;          /* inclusive sub-box of the source, tree coordinates */
  uint8_t  src_hi[3], pad1;
  uint32_t op;                       /* DUST_HIP_STAMP_* */
  uint32_t reserved[3];              /* ignored */
} DustHipResample;
typedef struct DustHipResampleCount { /* 16 bytes */
  uint32_t changed, covered, solid, blocked;
} DustHipResampleCount;
DustStatus dust_hip_model_resample(DustHipModel* dst, const DustHipModel* src, const DustHipResample* records, uint32_t n,
                                   const uint8_t* palette_map /* 255 entries, or NULL = identity */, uint32_t flags,
                                   DustHipResampleCount* counts /* n, may be NULL */);
/* current size of a model's Block array and material stream, and a synchronous copy of both to the host */
DustStatus dust_hip_model_info(const DustHipModel*, uint32_t* n_blocks, uint64_t* n_materials);
DustStatus dust_hip_model_read(const DustHipModel*, DustHipBlock* blocks, uint32_t block_capacity, uint8_t* materials, uint64_t material_capacity);
/* The upper levels of a model as they stand on the device -- what the traversal descends through before it reaches a Block --, and a
 * synchronous copy of them to the host: a check of the device-side rebuild (set_voxels and every later edit call) against
 * dust_hip_model_create, array for array. Layouts:
 *   N16 node (root; l2 nodes of 4096^3 trees), DUST_HIP_N16_BYTES: 64 x u64 child mask, bit (x << 8 | y << 4 | z) of the node's 16^3
 *     cells; 64 x u16 rank prefix, the number of children in the mask words before this one; u32 child_base; 12 bytes of zero. A child's
 *     index is child_base + prefix[word] + popcount(mask[word] below the bit): into the l2 nodes from a 4096^3 tree's root, into the
 *     mid nodes otherwise.
 *   DustHipMidNode: the 64-bit mask of a 16^3 cell's 4^3 bricks (bit x << 4 | y << 2 | z), and the Block index of its first brick;
 *     brick `bit` is Block first_block + popcount(mask below the bit).
 *   dense_mask: 64 x u64 per mid node, the occupancy mask of brick `bit` at [mid * 64 + bit], 0 where there is none.
 *   DustHipL2Cell (4096^3 trees): per l2 node and 16^3 cell, [l2 * 4096 + cell]: its mid node, or 0xFFFFFFFF with bounds and
 *     child_mask 0 for an empty cell; the mid node's mask; the box of its occupied bricks, lo.x | lo.y << 2 | lo.z << 4 | hi.x << 6 |
 *     hi.y << 8 | hi.z << 10.
 * info (struct_size set by the caller) receives extent_log2 (8 or 12), n_mid, n_l2 (0 for 256^3 trees) and the tight bounds bmin /
 * bmax of the bricks (all 0 for an empty model). Every array is optional (NULL: not copied): mid takes n_mid records, dense_mask
 * n_mid * 64 words, root DUST_HIP_N16_BYTES, l2 n_l2 * DUST_HIP_N16_BYTES, l2_cells n_l2 * 4096 records; host_root takes the
 * DUST_HIP_N16_ROOT_BYTES (masks and prefixes) the library keeps on the host, the copy dust_hip_scene_commit puts into the scene image.
 * The capacities are counted in records (mid, l2, l2_cells) and words (dense_mask); a call with info alone reports the sizes. What lies
 * past n_mid in an editable model's buffers is not part of any contract and is not copied.
 * DUST_ERR_INVALID_ARGUMENT, before anything is written: a null model or info; a struct_size below sizeof(DustHipHierarchyInfo); a
 * capacity below what its array takes. Synchronous, like dust_hip_model_read: it waits for the context's stream. */
#define DUST_HIP_N16_BYTES      656u
#define DUST_HIP_N16_ROOT_BYTES 640u
typedef struct DustHipHierarchyInfo {   /* 48 bytes */
  uint32_t struct_size;
  uint32_t extent_log2;                 /* 8 or 12 */
  uint32_t n_mid, n_l2;
  float bmin[3], bmax[3];
  uint32_t reserved[2];                 /* 0 */
} DustHipHierarchyInfo;
typedef struct DustHipMidNode {         /* 16 bytes */
  uint32_t mask_lo, mask_hi;
  uint32_t first_block;
  uint32_t pad;                         /* 0 */
} DustHipMidNode;
typedef struct DustHipL2Cell {          /* 16 bytes */
  uint32_t mid;
  uint32_t bounds;
  uint64_t child_mask;
} DustHipL2Cell;
DustStatus dust_hip_model_read_hierarchy(const DustHipModel*, DustHipHierarchyInfo* info, DustHipMidNode* mid, uint32_t mid_capacity,
                                         uint64_t* dense_mask, uint64_t dense_mask_capacity, uint8_t* root, uint8_t* host_root,
                                         uint8_t* l2, uint32_t l2_capacity, DustHipL2Cell* l2_cells, uint64_t l2_cell_capacity);
/* Lifetimes: a scene keeps the models it instances alive, every model / scene / pipeline its context; destroying a scene or
 * pipeline first waits for the frames in flight on the context's stream. After *_destroy the CALLER must not use the handle
 * again, whatever else still holds the object. Calls on one context are not thread-safe against each other;
 * dust_hip_last_error() is per thread. */

/* TLASStore (render/src/accel_struct/tlas.rs:28-180) + the prev-frame transform vec (standard.rs:845-878) */
DustStatus dust_hip_scene_create(DustHipContext*, DustHipScene** out);
void dust_hip_scene_destroy(DustHipScene*);
/* tlas_system push (tlas.rs:79-128): returns gl_InstanceID == push order */
DustStatus dust_hip_scene_add_instance(DustHipScene*, const DustHipModel*, const float obj_to_world[12],
                                       const float prev_obj_to_world_mat4[16], uint32_t* instance_id);
DustStatus dust_hip_scene_set_transform(DustHipScene*, uint32_t instance_id, const float obj_to_world[12],
                                        const float prev_obj_to_world_mat4[16]);
/* TLAS build (tlas.rs:43-64, rebuilt inside the frame's command stream whenever an instance moved): must be called after
 * add / set_transform (and after editing an instanced model) before rendering. Asynchronous: the records of the instances
 * that changed are re-derived on the host and one stream-ordered copy from pinned memory carries them to the device behind
 * the frame in flight -- no allocation and no wait unless instances were added since the last commit. */
DustStatus dust_hip_scene_commit(DustHipScene*);
/* Host only (no device, no context): the two top-level structures dust_hip_scene_commit builds over the instances' world boxes --
 * what the reference hands to the driver as a TLAS (accel_struct/tlas.rs:37-117). boxes: n x {lo[3], hi[3]}.
 *   grid:  info->dim cells of info->cell from info->lo; cells[c] = first item | items << 20 for cell c = (z * dim[1] + y) * dim[0] + x;
 *          items: instance ids; ranges[2 i], ranges[2 i + 1]: the block of cells instance i is listed in, x | y << 9 | z << 18;
 *   slot_order: the instances along a Morton curve (the packet cull groups 64 consecutive ones when n > 256: info->n_groups).
 * Any output pointer may be NULL (info alone gives the sizes). For tests and tools. */
typedef struct DustTopLevelInfo {
  uint32_t struct_size;
  uint32_t dim[3];
  float lo[3], cell[3];
  uint32_t n_cells, n_items, n_groups;
} DustTopLevelInfo;
DustStatus dust_hip_top_level_build(const float* boxes, uint32_t n, DustTopLevelInfo* info, uint32_t* cells, size_t cells_capacity, uint16_t* items,
                                size_t items_capacity, uint32_t* ranges, uint32_t* slot_order);

/* Scene ray queries: what a game's own ray-tracing pipeline traces against the TLAS (render/src/pipeline/mod.rs:64-98) -- picking,
 * where an edit lands, line of sight, probes. Every ray is a primary-type ray: hit.rint's exact voxel DDA over the instances, with
 * the frame's tie rule (equal t: the lower instance, then the lower block wins). */
typedef struct DustHipRay {      /* 32 bytes */
  float origin[3]; float tmin;   /* world space; t is measured in units of |direction| (it need not be normalised) */
  float direction[3]; float tmax;
} DustHipRay;
typedef struct DustHipRayHit {   /* 32 bytes */
  float t;                       /* tmax on a miss */
  uint32_t instance;             /* gl_InstanceID; DUST_HIP_NO_HIT on a miss */
  uint32_t block;                /* gl_PrimitiveID: index into the model's Block array */
  uint32_t voxel;                /* voxel in the 4^3 brick, hit.rint's numbering: x << 4 | y << 2 | z */
  uint32_t xyz[3];               /* that voxel in the model's tree coordinates: what the model's set_voxels / get_voxels take */
  uint8_t face;                  /* normal2FaceID (normal.glsl:39-43) of the model-space normal hit.rchit computes */
  uint8_t palette;               /* palette index (hit.rchit's material lookup) */
  uint16_t reserved;             /* 0 */
} DustHipRayHit;
#define DUST_HIP_NO_HIT 0xFFFFFFFFu
#define DUST_HIP_QUERY_ANY_HIT 1u   /* stop at the first accepted hit (gl_RayFlagsTerminateOnFirstHitEXT): some hit in [tmin, tmax],
                                       not necessarily the closest; every field describes that one hit */
/* A query reads the scene as last committed: DUST_ERR_NOT_READY with uncommitted changes or a model edited since the commit (as a
 * frame). Degenerate rays -- a zero direction, any non-finite component, a non-finite tmin or tmax, tmin > tmax -- report a miss.
 * A null scene is refused; n == 0 is a no-op, whatever the arrays. Synchronous: host arrays, returns with the hits written (device staging is the context's, grown on demand). */
DustStatus dust_hip_scene_trace_rays(DustHipScene*, const DustHipRay* rays, DustHipRayHit* hits, uint32_t n, uint32_t flags);
/* The same on device arrays (16-byte aligned), enqueued on the context's stream behind the frames already submitted; returns at once.
 * The hits are valid after dust_hip_sync, or after an event recorded on the caller's stream when the context was given that stream. */
DustStatus dust_hip_scene_trace_rays_async(DustHipScene*, const DustHipRay* d_rays, DustHipRayHit* d_hits, uint32_t n, uint32_t flags);

/* Scene box queries: the region counterpart of the ray queries -- every solid voxel of the committed scene inside a world-space box
 * (collision, placement, area edits, trigger volumes).
 *
 * Voxel (x, y, z) of an instance is the model-space unit cube [x, x+1] x [y, y+1] x [z, z+1], mapped into world space by the instance's
 * obj_to_world m (3 x 4, row-major).
 * - Axis-aligned instances (the 3 x 3 part has exactly one nonzero entry per row and per column: 90-degree rotations, mirrors, any
 *   scale) are EXACT on float32: a world corner coordinate is w_r = ((m[r][0]*px + m[r][1]*py) + m[r][2]*pz) + m[r][3], every operation
 *   rounded to nearest, no fused multiply-add; the voxel's world box is the per-axis min and max of its corners. Per axis the voxel
 *   overlaps the query when v_lo < hi && lo < v_hi; on an axis where lo == hi, when v_lo <= lo < v_hi (a point or a flat box names
 *   exactly one voxel per axis). Touching faces do not count: a box standing on a floor does not report the floor.
 * - Other instances (arbitrary rotations, shears) within tau = 1e-5 * (1 + M), M the largest magnitude of any coordinate of the box or
 *   of the voxel's world corners: every voxel whose world cube overlaps the box shrunk by tau on every side is reported, none that does
 *   not overlap the box grown by tau.
 * counts[i]: the overlapping voxels over all instances (saturating at UINT32_MAX). Query i writes min(counts[i], capacity) records into
 * records[first .. first + capacity); slots past counts[i] are left untouched. Nothing is ever written at an index >= n_records, whatever
 * first and capacity say (the synchronous form refuses a slice that runs past n_records with DUST_ERR_INVALID_ARGUMENT before anything
 * is launched). Overlapping slices of two queries have unspecified contents.
 * Order (deterministic): ascending instance, then ascending block, then ascending voxel bit; a truncated query keeps the first capacity
 * records in that order, and two runs give the same bytes. DUST_HIP_QUERY_ANY_HIT: counts[i] is 0 or 1, and the record (capacity >= 1)
 * is one overlapping voxel, not necessarily the first in order ("is this space free"). Degenerate boxes -- a non-finite coordinate, or
 * lo > hi on any axis -- report 0.
 * As the ray queries: the scene as last committed (DUST_ERR_NOT_READY otherwise); a null scene is refused; n == 0 is a no-op, whatever
 * the arrays; null arrays with n > 0 are refused; flags other than DUST_HIP_QUERY_ANY_HIT are refused. */
typedef struct DustHipBoxQuery {   /* 32 bytes */
  float lo[3]; uint32_t first;     /* world-space box; first: index of this query's first slot in `records` */
  float hi[3]; uint32_t capacity;  /* slots this query may fill (0 = count only) */
} DustHipBoxQuery;
typedef struct DustHipVoxelRef {   /* 16 bytes */
  uint32_t instance;               /* gl_InstanceID */
  uint32_t block;                  /* gl_PrimitiveID: index into the model's Block array */
  uint16_t xyz[3];                 /* the voxel in the model's tree coordinates: what the model's set_voxels / get_voxels take */
  uint8_t palette;                 /* palette index (the material stream, as in DustHipRayHit) */
  uint8_t voxel;                   /* voxel in the 4^3 brick, x << 4 | y << 2 | z (as DustHipRayHit.voxel) */
} DustHipVoxelRef;
/* Synchronous: host arrays, returns with counts and records written (device staging is the context's, grown on demand). */
DustStatus dust_hip_scene_overlap_boxes(DustHipScene*, const DustHipBoxQuery* boxes, uint32_t n, uint32_t* counts,
                                        DustHipVoxelRef* records, uint32_t n_records, uint32_t flags);
/* The same on device arrays (16-byte aligned), enqueued on the context's stream; valid after dust_hip_sync (as trace_rays_async). */
DustStatus dust_hip_scene_overlap_boxes_async(DustHipScene*, const DustHipBoxQuery* d_boxes, uint32_t n, uint32_t* d_counts,
                                              DustHipVoxelRef* d_records, uint32_t n_records, uint32_t flags);

/* Scene box sweeps (shape casts): how far a world-space box can move along a straight path before it touches a solid voxel of the
 * committed scene, and which face stops it -- a character controller's move-and-slide, a thrown prop, a camera spring arm.
 *
 * At t in [0, 1] the box is [lo + t delta, hi + t delta]. The voxels are the box queries' (above): the unit cube of voxel (x, y, z)
 * through the instance's obj_to_world.
 * - Axis-aligned instances are EXACT on float32. The voxel's world slab [a_r, b_r] on world axis r is the box queries' corner formula;
 *   each - and / below is one float32 operation, rounded to nearest (IEEE division, no contraction). Per world axis r, d = delta[r]:
 *     d > 0:  e_r = (a_r - hi_r) / d,  x_r = (b_r - lo_r) / d;
 *     d < 0:  e_r = (b_r - lo_r) / d,  x_r = (a_r - hi_r) / d;
 *     d == +-0 (a resting axis): in contact at every t when the box queries' per-axis rule holds (a < hi && lo < b; on lo == hi:
 *     a <= lo < b), never otherwise.
 *   T_in = the max of e_r over the moving axes (-inf if there are none), T_out = the min of x_r (+inf if there are none). The voxel is
 *   HIT when every resting axis is in contact, T_in < T_out, T_in < 1 and T_out > 0 -- and, with DUST_HIP_SWEEP_IGNORE_START, T_in >= 0
 *   (-0 passes). Its time is t = T_in if T_in > 0, else +0. Its normal is 0 if T_in < 0 (the box started inside it); otherwise
 *   -sign(delta[r*]) on axis r*, the lowest moving axis with e_r == T_in (IEEE equality: -0 == +0).
 *   So: touching faces do not count; a grazing edge (T_in == T_out) is not a hit; touching at t = 1 is not a hit; a box standing on a
 *   floor slides along it freely, but moving down it reports t = 0 with normal +y. delta = 0 hits exactly when overlap_boxes counts
 *   at least one voxel inside the box.
 * - Other instances (rotations, shears) within the box queries' tau = 1e-5 * (1 + M), M the largest magnitude of the box's coordinates
 *   at t = 0 and t = 1 and of the voxel's world corners. With t_v(s) the exact first contact time of voxel v against the box grown by s
 *   on every side: a hit on v* at t satisfies t_v*(+tau) <= t <= min over v of t_v(-tau); a miss means that no voxel has contact with
 *   the shrunk box; the normal is a unit vector with normal . delta <= 0. (There, delta = 0 agrees with overlap_boxes only within tau.)
 * The answer is the hit voxel that minimises (t, instance, block, voxel bit): deterministic, two runs give the same bytes.
 * DUST_HIP_QUERY_ANY_HIT: some hit voxel, with its own t and normal. A miss writes t = 1, instance = DUST_HIP_NO_HIT and zeros in every
 * other field. Degenerate sweeps -- a non-finite coordinate or delta component, or lo > hi on any axis -- report a miss.
 * As the box queries: the scene as last committed (DUST_ERR_NOT_READY otherwise); a null scene is refused; n == 0 is a no-op, whatever
 * the arrays; null arrays with n > 0 are refused; flags other than DUST_HIP_QUERY_ANY_HIT | DUST_HIP_SWEEP_IGNORE_START are refused. */
typedef struct DustHipBoxSweep {   /* 48 bytes */
  float lo[3];    uint32_t reserved0;  /* world-space box at t = 0 */
  float hi[3];    uint32_t reserved1;
  float delta[3]; uint32_t reserved2;  /* displacement: at t in [0, 1] the box is [lo + t delta, hi + t delta]; reserved words ignored */
} DustHipBoxSweep;
typedef struct DustHipSweepHit {   /* 32 bytes */
  float t;                         /* first contact in [0, 1); 1 on a miss */
  uint32_t instance;               /* gl_InstanceID; DUST_HIP_NO_HIT on a miss */
  uint32_t block;                  /* index into the model's Block array */
  uint16_t xyz[3];                 /* the voxel in the model's tree coordinates (what set_voxels / get_voxels take) */
  uint8_t palette;                 /* palette index */
  uint8_t voxel;                   /* x << 4 | y << 2 | z in the brick */
  float normal[3];                 /* world-space unit contact normal, pointing from the voxel toward the box (normal . delta < 0);
                                      0 when the box starts inside the voxel, and on a miss */
} DustHipSweepHit;                 /* bytes 4..19 have the layout of a DustHipVoxelRef */
#define DUST_HIP_SWEEP_IGNORE_START 2u /* voxels the box is already inside at t = 0 do not stop it (a controller unsticking itself) */
/* Synchronous: host arrays, returns with the hits written (device staging is the context's, grown on demand). */
DustStatus dust_hip_scene_sweep_boxes(DustHipScene*, const DustHipBoxSweep* sweeps, DustHipSweepHit* hits, uint32_t n, uint32_t flags);
/* The same on device arrays (16-byte aligned), enqueued on the context's stream; valid after dust_hip_sync (as trace_rays_async). */
DustStatus dust_hip_scene_sweep_boxes_async(DustHipScene*, const DustHipBoxSweep* d_sweeps, DustHipSweepHit* d_hits, uint32_t n, uint32_t flags);

/* the members of CameraSettings the shaders read (standard.rs:277-302,813-827; layout.playout:20-33) */
typedef struct DustHipCamera {
  float view_col0[3], view_col1[3], view_col2[3]; /* camera_view_col0..2 */
  float position[3];
  float tan_half_fov, far_, near_;
} DustHipCamera;


/* GBuffer planes (standard.rs:881-917; formats :974-1050) */
typedef enum DustHipPlane {
  DUST_PLANE_ILLUMINANCE = 0, /* RGBA16F, 8 B/px  (img_illuminance) */
  DUST_PLANE_DENOISED = 1,    /* RGBA16F, 8 B/px  (img_illuminance_denoised) */
  DUST_PLANE_ALBEDO = 2,      /* A2B10G10R10, 4 B/px */
  DUST_PLANE_NORMAL = 3,      /* A2B10G10R10, 4 B/px */
  DUST_PLANE_DEPTH = 4,       /* R32F, 4 B/px */
  DUST_PLANE_MOTION = 5,      /* RGBA16F, 8 B/px */
  DUST_PLANE_VOXEL_ID = 6,    /* R32UI, 4 B/px */
  DUST_PLANE_ACCUM = 7,       /* RGBA32F, 16 B/px: accumulated unpacked illuminance + frame count (DUST_PASS_ACCUMULATE: plain
                                 N-frame mean; DUST_PASS_DENOISE: the reprojected temporal accumulation, which IS the filter's history:
                                 the plane's device pointer then alternates between two buffers from frame to frame -- query it
                                 per frame, or bind the plane -- and a frame may ask for one of the two passes, not both) */
  DUST_PLANE_OUTPUT = 8,      /* RGBA16F, 8 B/px: tone-mapped display image (ToneMappingPipeline's dst) */
  DUST_PLANE_COUNT = 9
} DustHipPlane;

/* ray types (StandardPipeline::*_RAYTYPE, standard.rs:223-226) double as pass bits */
#define DUST_PASS_PRIMARY (1u << 0)            /* standard.rs:477-490 */
#define DUST_PASS_AMBIENT_OCCLUSION (1u << 1)  /* standard.rs:564-577 (sun shadow + AO ray) */
#define DUST_PASS_FINAL_GATHER (1u << 2)       /* standard.rs:627-640 */
#define DUST_PASS_SURFEL (1u << 3)             /* standard.rs:712-725 */
#define DUST_PASS_ACCUMULATE (1u << 4)         /* stands in for NRDPipeline::render (nrd.rs:272-617) */
#define DUST_PASS_DENOISE (1u << 5)            /* NRDPipeline::render (nrd.rs:272-617) as a native spatiotemporal filter: temporal
                                                  reprojection through the motion plane with disocclusion tests and antilag, then an
                                                  edge-aware blur; writes img_illuminance_denoised (and DUST_PLANE_ACCUM: the temporal
                                                  accumulation + frame count). Whole frames only. Settings: dust_hip_pipeline_set_denoiser */
#define DUST_PASS_COUNT_STATS (1u << 16)       /* run the counting build of the kernels (slower) */
#define DUST_PASS_GI_ORDERED (1u << 17)        /* apply the surfel pass's hash inserts in surfel-index order (bitwise
                                                  repeatable, serial); default: concurrently, as the reference's racy
                                                  shaders do (spatial_hash.glsl:147-195), statistically repeatable.
                                                  Of one frame's inserts of ONE hash key only the last 8 in surfel order
                                                  are applied (the reference applies all): on a scene whose surfels pile
                                                  onto hot keys that costs a third of their samples, and after 12 frames
                                                  the mean illuminance differs by 1.3 %, a key's radiance by 5 % at the
                                                  95th percentile (tests/parity_util.py DRIFT_BOUNDS: bounds of 3 % and 10 %) */
#define DUST_PASS_GI_SHARDED (1u << 18)        /* multi-GPU GI (see dust_hip_pipeline_gi_exchange): the final gather may
                                                  run on a row band; it records which hash entries it stamped and
                                                  leaves the surfel enqueues uncommitted for the exchange */

typedef struct DustHipFrameParams {
  uint32_t struct_size;
  uint32_t passes;       /* DUST_PASS_* */
  uint32_t frame_index;  /* push constant frame_index (standard.rs:252,457-463) */
  uint32_t rand;         /* push constant rand (standard.rs:449-456) */
  uint32_t row_begin, row_end; /* rows of the frame this call renders (multi-GPU bands); 0,0 = all */
  /* ---- appended in round 6 (a caller whose struct_size ends at row_end gets zeroes: the whole pool on this device) */
  uint32_t surfel_rank, surfel_world; /* DUST_PASS_SURFEL | DUST_PASS_GI_SHARDED with surfel_world >= 1: this call runs the pool's ordering and
                                  TRACES only rank surfel_rank's share of the position-ordered pool (see dust_hip_gi_surfel_exchange_run,
                                  which completes the pass); surfel_world == 0: the whole pass, as before */
} DustHipFrameParams;

typedef struct DustHipPassStats {
  float ms;                 /* kernel time from HIP events on the launch stream (needs DUST_HIP_CONTEXT_TIMING) */
  uint64_t rays;            /* rays issued (needs DUST_PASS_COUNT_STATS, else 0) */
  uint64_t instances_tested;
  uint64_t upper_descents;
  uint64_t mid_descents;
  uint64_t bricks_tested;
  uint64_t hits;
} DustHipPassStats;

/* StandardPipeline::new + use_gbuffer (standard.rs:90-173, :940-1065): persistent buffers and G-buffer */
DustStatus dust_hip_pipeline_create(DustHipContext*, uint32_t width, uint32_t height, DustHipPipeline** out);
void dust_hip_pipeline_destroy(DustHipPipeline*);
/* BlueNoise (noise.rs:7-56): texture 0 (scalar, R8) or 5 (unitvec3_cosine, RGBA8), 128 x 128 x layers */
DustStatus dust_hip_pipeline_set_noise(DustHipPipeline*, uint32_t texture, const uint8_t* texels, uint32_t layers);
/* StandardPipeline::render (standard.rs:228-810). Asynchronous on the context's stream.
 * DUST_ERR_NOT_READY while a noise texture a requested pass samples has not been set.
 * Every pass of the frame is enqueued before the call returns (nothing is kept back for a later call). The surfel pass
 * (DUST_PASS_SURFEL) only has to be complete before the NEXT frame's final gather reads the spatial hash, and it is latency-bound:
 * it is enqueued on a second stream the context owns, behind this frame's final gather, so that the next frame's primary / AO
 * kernels run beside it. It reads the scene and writes only the library-owned GI buffers; every library call that conflicts with
 * it (the next final gather, dust_hip_scene_commit, model edits, the GI state accessors) waits for it on the device, and
 * dust_hip_sync and every synchronous read-back wait for both streams -- a caller that orders its own work on the context's
 * stream (e.g. a collective that reads a bound plane) needs nothing more. DustHipPipelineConfig.side_stream = DUST_SIDE_STREAM_OFF keeps
 * the pass in place. */
DustStatus dust_hip_render_frame(DustHipPipeline*, const DustHipScene*, const DustHipCamera*, const DustHipSky*,
                                 const DustHipFrameParams*);
/* What the host does to the scene before a frame of dust_hip_render_frames: the transforms of the entities that moved since the previous frame
 * (tlas_system pushes them every frame, accel_struct/tlas.rs:79-128; castle.rs:287-291 moves the teapot). n == 0: the scene as the previous
 * frame left it. */
typedef struct DustHipFrameMoves {
  uint32_t n;                      /* instances moved before this frame */
  const uint32_t* instance_ids;    /* n ids (dust_hip_scene_add_instance) */
  const float* obj_to_world;       /* n x 12, as dust_hip_scene_set_transform takes them */
  const float* prev_obj_to_world;  /* n x 16 (the previous frame's transforms, for the motion vectors), or NULL */
} DustHipFrameMoves;
/* Frames in flight (rhyolite_bevy/src/lib.rs:58 `max_frame_in_flight: 3`; StandardPipeline::render is called once per frame and the frames
 * overlap on the device): n_frames frames in one call -- frame i with cameras[i], skies[i], params[i] into pipelines[i], after moves[i] (if
 * moves != NULL) have been applied to the scene and committed -- with exactly the results of, for every i in order,
 * dust_hip_scene_set_transform x moves[i].n + dust_hip_scene_commit + dust_hip_render_frame. Frames that qualify share ONE persistent launch
 * (up to 8 per launch, more are split): a wavefront that finds frame i without tiles goes straight on to frame i + 1, so the launch's tail,
 * the staging of the roots and the gap between launches are paid once for all of its frames (1080p primary + AO: 0.22 ms per frame alone,
 * 0.209 at four per launch, 0.2065 at eight). Qualifying: passes == DUST_PASS_PRIMARY | DUST_PASS_AMBIENT_OCCLUSION for every frame, distinct pipelines of
 * the scene's context with one frame size, one row band and the same DustHipPipelineConfig, no surfel pass outstanding. Every frame reads the
 * scene as ITS moves left it (the scene's ring of device images holds as many states as a launch has frames). Anything else (GI passes: a
 * frame's gather reads the hash its predecessor's surfel pass wrote) is enqueued frame after frame as dust_hip_render_frame would. Every
 * frame's arguments are checked before the scene is touched and the first frame is enqueued; params[i].struct_size must be
 * sizeof(DustHipFrameParams). With DUST_HIP_CONTEXT_TIMING the launch's time is reported by pipelines[0] (pass 0), once for all frames of
 * the launch. After the call the scene is as the last frame saw it.
 * Same-view frames: consecutive frames of a launch whose cameras[i] and skies[i] are byte-identical and between which no moves were committed
 * (N samples per pixel of one view, a viewer whose camera rests) differ only in their AO rays -- frame_index and rand feed nothing else. Their
 * camera rays, the shading and their sun shadow rays are traced ONCE per launch; every frame's pipeline still gets all of its planes, with the
 * bits dust_hip_render_frame writes, and each frame's AO ray is its own. A frame whose camera, sky or scene differs starts a new run of its own. */
DustStatus dust_hip_render_frames(uint32_t n_frames, DustHipPipeline* const* pipelines, DustHipScene*, const DustHipCamera* cameras,
                                  const DustHipSky* skies, const DustHipFrameParams* params, const DustHipFrameMoves* moves);
/* pass: 0 primary, 1 AO-pass sun-shadow rays, 2 AO rays, 3 final gather, 4 surfel sun rays, 5 surfel cosine rays.
 * When primary and AO passes are requested together they run as ONE fused kernel: its time is reported under
 * pass 0 and passes 1-2 report ms = 0 (set DUST_HIP_NO_FUSE=1 to launch them separately). */
DustStatus dust_hip_pipeline_pass_stats(DustHipPipeline*, uint32_t pass, DustHipPassStats* out);
/* Kernel time over a run of frames (DUST_HIP_CONTEXT_TIMING): per pass kind -- 0 primary (or the fused primary + AO kernel), 1 AO,
 * 2 final gather (+ commit; not the regrouping pre-pass), 3 surfel pass (keys, sort, trace, apply) -- the summed HIP-event durations of its launches
 * since the last call with mark != 0 (at most the 256 most recent ones), and how many launches that was. Waits for the stream.
 * Nothing is synchronised per frame: the pairs are recorded into a ring on the launch stream and read here. */
DustStatus dust_hip_pipeline_kernel_times(DustHipPipeline*, int mark, float ms_sum[4], uint32_t launches[4]);
/* Work distribution feedback. The traversal kernels are persistent launches whose tiles (8 x 8 pixel packets; 64-entry chunks of
 * the regrouped gather and surfel lists) cost very different amounts; a launch records the shader-clock cycles each tile took,
 * and the next launch of the same pass hands its tiles out most expensive first (per XCD band), so that the launch does not end on a
 * few late, slow tiles. While camera, scene, sun and row band stay as they were the order is kept and re-measured every 8th launch at first, then every 16th, 32nd, 64th
 * only. The order never changes a result. This reads the map of the pass's last MEASURED launch (a profiling heat map):
 * pass_kind 0 primary (or fused primary + AO), 1 AO, 2 final gather, 3 surfel trace; cycles may be NULL to query the grid only
 * (tiles_x x tiles_y, 0 x 0 before the first launch). DUST_HIP_NO_TILE_ORDER=1 switches the feedback off. */
DustStatus dust_hip_pipeline_tile_costs(DustHipPipeline*, uint32_t pass_kind, uint32_t* cycles, uint32_t capacity, uint32_t* tiles_x,
                                        uint32_t* tiles_y);
DustStatus dust_hip_pipeline_plane_device_ptr(DustHipPipeline*, DustHipPlane, void** ptr, size_t* bytes);
/* Render target binding (the reference binds its G-buffer images per frame, standard.rs:974-1050): redirects one plane to
 * caller-owned device memory of at least the plane's size (16-byte aligned), or back to the pipeline's own storage with a
 * null pointer. Frames enqueued afterwards read and write the plane there -- e.g. alternate two illuminance buffers so that
 * frame k can be sent to another GPU while frame k+1 renders, without a copy. The memory must stay valid until those frames
 * have completed; ordering against the caller's own use is the caller's (same stream, or events). */
DustStatus dust_hip_pipeline_bind_plane(DustHipPipeline*, DustHipPlane, void* device_ptr, size_t bytes);
/* synchronous device-to-host copy of one plane */
DustStatus dust_hip_pipeline_read_plane(DustHipPipeline*, DustHipPlane, void* dst, size_t dst_bytes);
/* Persistent GI buffers (standard.rs:334-358): (re)allocates and resets the spatial hash (SpatialHashCapacity,
 * spatial_hash.glsl:1, default 32 Mi entries) and the surfel pool (SurfelPoolSize, surfel.glsl:2, default 345600).
 * Called implicitly with the defaults by the first frame that runs a GI pass. Cancels a pending sharded surfel trace (step 6a of the
 * multi-GPU protocol below): its completion, dust_hip_gi_surfel_exchange_run, then fails with DUST_ERR_NOT_READY. */
DustStatus dust_hip_pipeline_configure_gi(DustHipPipeline*, uint32_t hash_capacity, uint32_t surfel_pool_size);
/* synchronous copy of GI state to the host: which = 0 spatial hash ((capacity+2) x 12 B), 1 surfel pool (16 B each);
 * and its inverse, which restores a saved state into a pipeline configured with the same capacity and pool size (checkpoint /
 * resume of a converged hash: the reference keeps its hash for the life of the process, standard.rs:334-358). The write is refused
 * with DUST_ERR_NOT_READY while a sharded surfel trace is pending (its completion would overwrite what it restores); the read is not. */
DustStatus dust_hip_pipeline_read_gi(DustHipPipeline*, uint32_t which, void* dst, size_t dst_bytes);
DustStatus dust_hip_pipeline_write_gi(DustHipPipeline*, uint32_t which, const void* src, size_t src_bytes);
/* Multi-GPU GI: every GPU keeps an identical spatial hash and surfel pool, the pixel passes run on row bands and the
 * (small) surfel pass is replicated. The reference has no multi-device path; the merge rule is this library's defined
 * order (final_gather.rchit:52-63 leaves the winner among the pixels aliasing a slot to a race): the highest pixel
 * index wins a surfel slot, as on one GPU. Per frame, on every rank:
 *   1. dust_hip_render_frame(PRIMARY | AMBIENT_OCCLUSION | FINAL_GATHER | DUST_PASS_GI_SHARDED, own row band)
 *   2. all-reduce MAX  of slot_owner (u32 x pool_size)                       -- the caller's collective (RCCL)
 *      all-gather      of the bands of `touched` (u32 per pixel, band r at row r * band_rows)
 *   3. dust_hip_gi_export(own band): merged[s] = the enqueued surfel if the winning pixel of slot s is in this band, else 0
 *   4. all-reduce SUM  of merged as i32 (16 B x pool_size; exactly one rank contributes per slot)
 *   5. dust_hip_gi_import(own band, frame_index): stamps last_accessed_frame of the entries the OTHER bands' final
 *      gather read, commits the winning surfels to the pool, clears slot_owner
 *   6. dust_hip_render_frame(SURFEL [| ACCUMULATE] | DUST_PASS_GI_SHARDED, rows as in 1 for ACCUMULATE)
 * With DUST_PASS_GI_ORDERED in step 6 every rank's hash and pool stay bit-identical to the single-GPU run.
 * Step 6 replicates the whole surfel pass on every rank -- 0.23 ms of the castle's 0.65 ms GI frame, which caps 8 ranks at 1.3-1.7 x.
 * Round 6 shards its TRACE (85 % of the pass) as well; the trace only reads the hash (identical on every rank after step 5):
 *   6a. dust_hip_render_frame(SURFEL | GI_ORDERED | GI_SHARDED [| ACCUMULATE], surfel_rank = r, surfel_world = N): orders the pool by
 *       position (replicated: 50 us) and traces the slots [r S, (r + 1) S) of that order, S = ceil(groups / N) x 64 -- the records
 *       {request 32 B, replacement 16 B, sun payload 16 B} go to staging arrays in SLOT order, a rank's share one contiguous run
 *   6b. dust_hip_gi_surfel_exchange_run: all-gather of the three arrays (64 B per slot: 22 MB for 345 600 slots), then on every rank
 *       the records move to their surfels, the trace's hash stamps are repeated, and the ordered apply runs (replicated: 30 us)
 *   Between 6a and 6b the pipeline refuses every GI pass (a second trace included) and dust_hip_pipeline_write_gi with
 *   DUST_ERR_NOT_READY; a refused 6b (DUST_ERR_INVALID_ARGUMENT: wrong rank, world or frame) leaves the trace pending for a correct one.
 *   dust_hip_pipeline_configure_gi and dust_hip_pipeline_clear cancel it. 6a without DUST_PASS_GI_ORDERED is DUST_ERR_INVALID_ARGUMENT.
 * -- bit-identical to the single-device ordered run again (tests/test_gpu_comm.py, test_gpu_gi_sharded.py).
 * dust_hip_pipeline_gi_exchange allocates (once) and returns the three device buffers the collectives run on;
 * padded_rows >= height is the row count of `touched` (world_size x band_rows).
 * A rank whose band lies past the end of the frame (small frames on many GPUs) skips steps 1 and the ACCUMULATE of 6 but still takes
 * part in every collective: it exports and imports the EMPTY range (height, height) -- its `merged` must be zeroed by the export,
 * or it would add the previous frame's all-reduced sum to this frame's. */
typedef struct DustHipGiExchange {
  uint32_t struct_size;
  uint32_t pool_size;      /* surfel slots */
  uint32_t width;          /* pixels per row of `touched` */
  uint32_t touched_rows;   /* rows of `touched` */
  void* slot_owner;        /* u32[pool_size]: 1 + highest pixel index that enqueued into the slot this frame, 0 = none */
  void* touched;           /* u32[touched_rows * width]: 1 + index of the hash entry the pixel's final gather stamped, 0 = none */
  void* merged;            /* 16 B x pool_size: SurfelEntry per slot */
} DustHipGiExchange;
DustStatus dust_hip_pipeline_gi_exchange(DustHipPipeline*, uint32_t padded_rows, DustHipGiExchange* out);
DustStatus dust_hip_gi_export(DustHipPipeline*, uint32_t row_begin, uint32_t row_end);
DustStatus dust_hip_gi_import(DustHipPipeline*, uint32_t row_begin, uint32_t row_end, uint32_t frame_index);
/* AutoExposurePipeline::render + ToneMappingPipeline::render (pipeline/auto_exposure.rs:96-248, tone_mapping.rs:76-200;
 * auto_exposure.comp, auto_exposure_avg.comp, tone_map.comp): 256-bin log-luminance histogram of the denoised radiance
 * (after DUST_PASS_ACCUMULATE: the N-frame mean), exponential adaptation of the average, then
 * radiance x albedo / avg -> display primaries -> ACES fit -> transfer function into DUST_PLANE_OUTPUT. */
typedef struct DustHipToneMapParams {
  uint32_t struct_size;
  uint32_t transfer_function;      /* ColorSpaceTransferFunction 0..8 (rhyolite utils/format.rs:683-693): 0 linear, 1 sRGB, ... */
  float color_space_conversion[9]; /* COLOR_SPACE_CONVERSION_0..8, column-major: scene (ACES AP1) -> display primaries */
  float min_log_luminance, max_log_luminance, time_coefficient; /* ExposureSettings (auto_exposure.rs:225-248): -6, 8.5, 0.2 */
} DustHipToneMapParams;
DustStatus dust_hip_tone_map(DustHipPipeline*, const DustHipToneMapParams*);
/* reads (and optionally first overwrites) the adapted average luminance the tone mapper divides by */
DustStatus dust_hip_pipeline_exposure(DustHipPipeline*, float* avg_luminance, const float* set_to);
/* ReblurSettings + CommonSettings as far as this filter has the knob (nrd.rs:693-785; defaults = what the reference sets or
 * NRD's own defaults): the reference's denoiser is NVIDIA NRD, a closed SDK -- DUST_PASS_DENOISE is a native filter of the same
 * shape, not its arithmetic. */
typedef struct DustHipDenoiseParams {
  uint32_t struct_size;
  uint32_t max_accumulated_frames; /* ReblurSettings::maxAccumulatedFrameNum, 30 */
  float disocclusion_threshold;    /* CommonSettings::disocclusion_threshold, 0.01: plane distance / view distance */
  float antilag_sigma_scale;       /* ReblurAntilagSettings::luminance_sigma_scale, 2.0 (nrd.rs:777) */
  float antilag_power;             /* ReblurAntilagSettings::luminance_antilag_power, 0.8 (nrd.rs:778); 0 = no antilag */
  float max_blur_radius;           /* ReblurSettings::blurRadius, 15 pixels; 0 = temporal accumulation only */
} DustHipDenoiseParams;
DustStatus dust_hip_pipeline_set_denoiser(DustHipPipeline*, const DustHipDenoiseParams*);
/* DenoiserEvent::Restart (nrd.rs:749-755): discard the history; the next DUST_PASS_DENOISE frame starts a new accumulation */
DustStatus dust_hip_pipeline_restart_denoiser(DustHipPipeline*);
/* zero every plane, the accumulation count and the denoiser history, and cancel a pending sharded surfel trace (its records are dropped:
 * dust_hip_gi_surfel_exchange_run then fails with DUST_ERR_NOT_READY). The spatial hash and the surfel pool are kept (with the
 * last_accessed_frame stamps the cancelled trace's hash reads made). */
DustStatus dust_hip_pipeline_clear(DustHipPipeline*);
/* How many frames the caller keeps in flight on this device, each on a pipeline and a context (stream) of its own -- the reference's
 * host runs up to three (rhyolite_bevy/src/lib.rs:58). The traversal kernels are persistent launches that take every workgroup slot
 * they are given and hold it until the launch's last tile is done; with n > 1 a launch of this pipeline's pixel passes starts about
 * 1/n of the slots, so that n frames' launches run side by side instead of each waiting behind the others' stragglers (row bands
 * of one frame on 8 GPUs, four in flight: 0.045 -> 0.037 ms per band). 1 (the default): a launch may take the whole device. 1..16. */
DustStatus dust_hip_pipeline_set_frames_in_flight(DustHipPipeline*, uint32_t n);
/* Everything that decides WHICH kernels a pipeline's frames run and on how much of the device -- what the reference's plugin takes as
 * its settings (RenderPlugin, crates/render/src/lib.rs:35-56; the frames in flight of rhyolite_bevy/src/lib.rs:58). Defaults (a
 * zeroed struct but for struct_size) are the production configuration; nothing here is read from the environment. May be called
 * between any two frames: launches enqueued afterwards follow it. */
#define DUST_GI_PATH_AUTO 0u     /* packets of 64 rays (k_final_gather, k_surfel_trace); the final gather of a scene that holds a 4096^3
                                    tree as a ray stream (one ray per lane, lanes refilled: DESIGN.md section 4) */
#define DUST_GI_PATH_PACKETS 1u  /* packets everywhere */
#define DUST_GI_PATH_STREAMS 2u  /* both GI passes as ray streams (measured slower on scenes of many instances) */
#define DUST_SIDE_STREAM_AUTO 0u /* the surfel pass on the context's second stream, beside the next frame's primary / AO kernel */
#define DUST_SIDE_STREAM_OFF 1u  /* in place, on the context's stream */
#define DUST_IN_FLIGHT_SHARE 0u  /* n frames in flight: every launch takes 1/n of the workgroup slots (row bands of an N-GPU frame) */
#define DUST_IN_FLIGHT_ALL 1u    /* every launch asks for ALL slots: the next frame's workgroups start on the CUs the previous frame's tail
                                    has left (whole frames on one GPU) */
#define DUST_RESERVE_AUTO 0xFFFFFFFFu
typedef struct DustHipPipelineConfig {
  uint32_t struct_size;
  uint32_t reserve_blocks;    /* workgroup slots (multiples of 8) the persistent traversal launches leave empty so that another queue's
                                 kernels -- RCCL's send / receive -- can become resident beside them (they hold every VGPR of the SIMDs
                                 they run on). DUST_RESERVE_AUTO (the default of dust_hip_pipeline_create): 0 until the pipeline takes part
                                 in a collective of a communicator with world > 1, 32 from then on. A value the device cannot spare (it keeps 8 slots) is ignored */
  uint32_t gi_path;           /* DUST_GI_PATH_* */
  uint32_t side_stream;       /* DUST_SIDE_STREAM_* */
  uint32_t side_share;        /* percent (5..90) of the slots the surfel pass takes on the second stream; 0 = calibrated from one timed frame */
  uint32_t frames_in_flight;  /* 1..16, as dust_hip_pipeline_set_frames_in_flight; 0 = leave as it is */
  uint32_t in_flight_slots;   /* DUST_IN_FLIGHT_* */
} DustHipPipelineConfig;
DustStatus dust_hip_pipeline_configure(DustHipPipeline*, const DustHipPipelineConfig*);
DustStatus dust_hip_pipeline_get_config(const DustHipPipeline*, DustHipPipelineConfig* out /* struct_size set by the caller */);

/* ===================================================================== multi-GPU: one process per GPU, RCCL over xGMI
 * The reference renders on one device; its plugin entry is where devices would be selected (crates/render/src/lib.rs:58-134).
 * north_star's partition: the pixels of a frame shard across the GPUs of a node as row bands (DustHipFrameParams.row_begin /
 * row_end; the scene is replicated), and the finished bands are gathered onto one GPU. A DustHipComm is this process's end of that:
 * an RCCL communicator bound to a context. librccl is opened on first use -- a single-GPU host never loads it. */
typedef struct DustHipComm DustHipComm;
#define DUST_HIP_COMM_ID_BYTES 128
/* ncclGetUniqueId: rank 0 makes the id and the host carries it to the other processes (any out-of-band way: a file, a socket, MPI) */
DustStatus dust_hip_comm_unique_id(uint8_t id[DUST_HIP_COMM_ID_BYTES]);
/* ncclCommInitRank on the context's device. Collective: every rank of the job calls it with the same id and world. */
DustStatus dust_hip_comm_create(DustHipContext*, uint32_t rank, uint32_t world, const uint8_t id[DUST_HIP_COMM_ID_BYTES], DustHipComm** out);
/* A LOOPBACK group: `world` ranks on ONE context (one device, one stream), out[0..world). The same entry points take these handles;
 * a collective is carried out -- with device copies and small reduction kernels, on the context's stream -- by the call that
 * completes it, i.e. when the group's last rank has made it, so every rank must make a call before any rank makes the next.
 * What a one-GPU box, the C++ host mirror and the tests drive the multi-GPU protocol with (each rank with a pipeline of its own). */
DustStatus dust_hip_comm_create_local(DustHipContext*, uint32_t world, DustHipComm** out);
void dust_hip_comm_destroy(DustHipComm*);
DustStatus dust_hip_comm_info(const DustHipComm*, uint32_t* rank, uint32_t* world, uint32_t* is_local);
/* Framebuffer gather. cuts: world + 1 row indices, 0 ... height, the same on every rank: rank r rendered rows [cuts[r], cuts[r+1]) of
 * `plane` (into the plane's current storage: the pipeline's own, or what dust_hip_pipeline_bind_plane gave it). Those rows travel to
 * rank `root` -- grouped ncclSend / ncclRecv, each peer over its own xGMI link -- into `dst` there (device memory of at least the
 * plane's size; NULL = the root pipeline's own plane, whose remaining rows are then filled in). Asynchronous: ordered behind
 * everything enqueued on the context's stream so far, carried out on the communicator's OWN stream, so that the next band frame
 * (rendering into another bound target) overlaps the transfer. *ticket (may be NULL) numbers the gather, from 1, per communicator.
 * Before a source target or `dst` is used again: dust_hip_comm_wait with that ticket. */
DustStatus dust_hip_gather_bands(DustHipPipeline*, DustHipComm*, DustHipPlane plane, const uint32_t* cuts, uint32_t root, void* dst, size_t dst_bytes,
                                 uint64_t* ticket);
/* The same for SEVERAL planes at once (plane_mask bit i = DustHipPlane i), each into the root pipeline's own plane: one RCCL group for
 * every plane and peer, one ticket. What a frame needs on the root before a pass that reads across rows -- the denoiser, which stands
 * in for the reference's NRD dispatch (crates/render/src/pipeline/nrd.rs:272-617; examples/castle.rs:190-231 runs render -> NRD -> tone
 * map in that order): gather illuminance | depth | normal | motion | voxel id (| denoised | albedo for the tone map), then
 * dust_hip_render_frame(root pipeline, passes = DUST_PASS_DENOISE) on the whole frame. */
DustStatus dust_hip_gather_planes(DustHipPipeline*, DustHipComm*, uint32_t plane_mask, const uint32_t* cuts, uint32_t root, uint64_t* ticket);
/* the context's stream waits (on the device) for gather `ticket` and every earlier one (0: for all enqueued so far) -- a host that
 * alternates two render targets waits for the gather that last read a target, not for the one still reading the other /
 * the host waits for every gather and for the context */
DustStatus dust_hip_comm_wait(DustHipComm*, uint64_t ticket);
DustStatus dust_hip_comm_sync(DustHipComm*);
/* Steps 2-5 of the multi-GPU GI protocol above (dust_hip_pipeline_gi_exchange), enqueued on the context's stream: all-reduce MAX of
 * slot_owner, all-gather of the `touched` bands (band r at row r * band_rows; every band is band_rows rows, the last may be
 * shorter in the frame), dust_hip_gi_export(row_begin, row_end), all-reduce SUM of `merged`, dust_hip_gi_import(..., frame_index).
 * A rank whose band lies past the end of the frame passes (height, height). */
DustStatus dust_hip_gi_exchange_run(DustHipPipeline*, DustHipComm*, uint32_t row_begin, uint32_t row_end, uint32_t band_rows, uint32_t frame_index);
/* Step 6b of the protocol: completes a surfel pass whose trace was sharded (dust_hip_render_frame with surfel_world >= 1, the same
 * world as the communicator's), on the context's stream: all-gather of the staged records (three ncclAllGather in one group; a loopback
 * group copies), then -- replicated on every rank -- records to their surfels + the trace's hash stamps, and the apply of the hash inserts
 * in surfel order (the deterministic apply of DUST_PASS_GI_ORDERED, whatever the frame asked for: every rank must end with the same hash).
 * A NULL communicator completes the pass with no exchange (a world of one; one emulated rank, whose peers' records are whatever the
 * staging arrays hold). DUST_ERR_NOT_READY without a sharded trace pending on the pipeline. */
DustStatus dust_hip_gi_surfel_exchange_run(DustHipPipeline*, DustHipComm*, uint32_t frame_index);

/* Device function evaluation: runs ONE of the device functions the traversal / shading kernels are built from on n
 * independent inputs (host arrays in, host arrays out, synchronous). The reference has no counterpart -- its shaders are
 * only reachable through vkCmdTraceRaysKHR -- this is how vectors of (ray, brick mask) -> (t, voxel) pairs and codec
 * round trips are checked against the device code directly (tests/golden/). Each input / output is a row of 32-bit
 * words (floats by bit pattern):
 *   fn  function (reference)                                          in words                          out words
 *   0   primary/hit.rint dda()            :43-131                      o[3] d[3] tmin mask_lo mask_hi    reported t voxel
 *   1   final_gather/ambient_occlusion.rint dda() :46-134              (same)                            (same; voxel 0xFF = threshold hit)
 *   2   final_gather/rough.rint dda()     :42-59                       (same)                            (same)
 *   3   EncodeRGBToLogLuv  (spatial_hash.glsl:28-60)                   rgb[3]                            packed
 *   4   DecodeLogLuvToRGB  (spatial_hash.glsl:64-93)                   packed                            rgb[3]
 *   5   NRD_FrontEnd_PackNormalAndRoughness -> A2B10G10R10 (nrd.glsl:25-52), roughness 1   n[3] materialID   texel
 *   6   NRD_FrontEnd_UnpackNormalAndRoughness (nrd.glsl:54-94)         texel                             n[3]
 *   7   REBLUR_FrontEnd_PackRadianceAndNormHitDist -> RGBA16F (nrd.glsl:127-147)   rgb[3] hitdist         2 words (4 halves)
 *   8   REBLUR_BackEnd_UnpackRadianceAndNormHitDist (nrd.glsl:107-125) 2 words                           rgb[3] hitdist
 *   9   float4 -> A2B10G10R10_UNORM                                    v[4]                              texel
 *   10  CubedNormalize + normal2FaceID (normal.glsl:9-18,39-43)        d[3]                              n[3] face
 *   11  rotateVectorByNormal (normal.glsl:31-37)                       n[3] target[3]                    v[3]
 *   12  (not per row) the surfel pass's stable radix sort of the n rows by key    key value              key value
 *   13  (not per row) the cost-ordered hand-out's sorter: the n rows are tile costs in tile order, 8 bands     cycles     tile index
 *   14  (not per row) the same with the bands cut at equal measured cost (what a frame uses), n >= 9           cycles     tile index, cut (the 9 band cuts in rows 0..8)
 *   15  arhosek_sky_radiance (sky.glsl:18-79)                          dir[3]                            rgb[3]
 *   16  arhosek_sun_radiance (sky.glsl:81-113)                         dir[3]                            rgb[3]
 *       15, 16: the 56 floats of the sky state, shared by the rows of a call, ride in rows 0..18 (3 words a row, the last word padding; n >= 19)
 *       and reach the functions through the kernel argument, as a frame's do; the output rows 0..18 are zero
 *   17  SRGBToLinear of the block's average albedo and sRGB2AECScg(AECScg2sRGB(r) * albedo) (color.glsl:1-23, final_gather.rchit:68-80)
 *                                                                      r[3] packed_albedo                albedo[3] rgb[3]
 *   18  SpatialHashKeyGetFingerprint, ...GetLocation (spatial_hash.glsl:128-142)   x y z (int32) dir capacity   fingerprint location (0 for capacity 0)
 *   19  SpatialHashInsert (spatial_hash.glsl:147-195) on a copy of the probe window in registers, as the deterministic apply runs it: three
 *       entries of (fingerprint, radiance, last_accessed_frame | sample_count << 16)   window[9] fingerprint value[3] frame_index   window[9] */
DustStatus dust_hip_device_eval(DustHipContext*, uint32_t fn, const uint32_t* in, uint32_t in_words, uint32_t* out,
                                uint32_t out_words, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif
