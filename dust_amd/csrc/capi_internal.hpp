// capi_internal.hpp -- the host runtime's internal header (not part of the C ABI): the accessors comm.hip needs, and what the
// runtime's translation units (capi.cpp, capi_model.cpp, capi_scene.cpp) share -- error helpers, DeviceBuffer, the handle structs.
// (What the model calls and the frame path compute without a device or a handle is model_records.hpp and frame_plan.hpp, which include none of this.)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dust_hip.h"
#include "dust_dev.h"
#include "grid.hpp"
#include "vox.hpp"

namespace dust_internal {
DustStatus set_error(DustStatus status, const std::string& message);  // dust_hip_last_error() of the calling thread
hipStream_t context_stream(DustHipContext*);
int context_device(DustHipContext*);
void context_retain(DustHipContext*);
void context_release(DustHipContext*);
DustHipContext* pipeline_context(DustHipPipeline*);
void pipeline_size(DustHipPipeline*, uint32_t* width, uint32_t* height);
// the pipeline takes part in a collective of a communicator with world > 1: DUST_RESERVE_AUTO leaves workgroup slots free from now on
void pipeline_note_collective(DustHipPipeline*);
// a pending sharded surfel trace (DustHipFrameParams::surfel_world): its slot-ordered staging arrays {32, 16, 16 bytes per slot}, and the pass's second half
struct SurfelStage { void* req; void* repl; void* sun; uint32_t slots_per_rank, rank, pool_size; };
DustStatus surfel_stage_view(DustHipPipeline*, uint32_t world, SurfelStage* out);
DustStatus surfel_finish(DustHipPipeline*, uint32_t frame_index);
// the exchange buffers dust_hip_pipeline_gi_exchange(p, padded_rows) made, WITHOUT (re)making them: DUST_ERR_NOT_READY when the
// pipeline's buffers were prepared for another padded_rows (or not at all) -- a frame's stamps must not be dropped by a re-allocation
DustStatus gi_exchange_view(DustHipPipeline*, uint32_t padded_rows, DustHipGiExchange* out);
// a stream of another object (a communicator's) that reads the context's pipelines: sync_stream waits for it too
void context_add_stream(DustHipContext*, hipStream_t);
void context_remove_stream(DustHipContext*, hipStream_t);
}  // namespace dust_internal

// ------------------------------------------------------------------ errors
inline DustStatus fail(DustStatus s, const std::string& msg) { return dust_internal::set_error(s, msg); }
inline DustStatus hip_fail(hipError_t e, const char* what) {
  return fail(DUST_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);   \
  } while (0)

// struct_size is the caller's sizeof of a versioned struct: at least the layout this build knows (a newer caller may pass
// more; the known prefix is what is read)
template <class T>
bool struct_ok(const T* s) { return s->struct_size >= sizeof(T); }
#define STRUCT_TRY(ptr, name) \
  do { if (!struct_ok(ptr)) return fail(DUST_ERR_INVALID_ARGUMENT, name ".struct_size is smaller than this library's " name); } while (0)

template <class F>
DustStatus guarded(F&& f) {  // nothing may unwind across the C boundary
  try {
    return f();
  } catch (const dust::vox::ParseError& e) {
    return fail(e.unsupported ? DUST_ERR_UNSUPPORTED : DUST_ERR_PARSE, e.what);
  } catch (const std::bad_alloc&) {
    return fail(DUST_ERR_OUT_OF_MEMORY, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(DUST_ERR_INVALID_ARGUMENT, e.what());
  } catch (...) {
    return fail(DUST_ERR_INVALID_ARGUMENT, "unknown error");
  }
}

struct DeviceBuffer {
  void* p = nullptr;
  size_t bytes = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
  void swap(DeviceBuffer& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
  hipError_t alloc(size_t n) {
    if (p) { (void)hipFree(p); p = nullptr; }
    bytes = n;
    return hipMalloc(&p, n ? n : 16);
  }
  // Host -> device on the CONTEXT's stream, then wait: a blocking hipMemcpy is a null-stream operation, which a
  // hipStreamNonBlocking stream is not ordered against (and from pageable memory it may return before the DMA has landed).
  hipError_t upload(const void* src, size_t n, hipStream_t st) {
    hipError_t e = alloc(n);
    if (e != hipSuccess || n == 0) return e;
    e = hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
  }
};

// Copies between host and device go through the context's stream and wait for it: the blocking hipMemcpy / hipMemset are
// null-stream operations, and the context's stream is created hipStreamNonBlocking, i.e. NOT ordered against those.
inline hipError_t copy_wait(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const hipError_t e = hipMemcpyAsync(dst, src, n, kind, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// Lifetimes. Every handle of the device side is reference-counted inside the library: a model, scene or pipeline keeps its
// context alive, a scene keeps the models it instances alive. dust_hip_*_destroy gives up the CALLER's reference; the object
// (and its device memory) goes when the last user does. So handles may be destroyed in any order -- a garbage collector
// finalising a context before its models (Python's cycle collector does exactly that, in creation order) is fine.
struct RefCounted {
  std::atomic<uint32_t> refs{1};
};
template <class T> T* retain(T* o) { if (o) o->refs.fetch_add(1, std::memory_order_relaxed); return o; }
// (release() per type below: what dies with the last reference differs)

struct DustHipContext : RefCounted {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  uint32_t lds_root_bytes = 64 * 1024;
  bool timing = false;
  uint32_t timing_stride = 1;  // DUST_HIP_CONTEXT_TIMING_SPARSE: event pairs around the launches of every 4th frame only
  int num_cus = 256;
  size_t max_lds = 64 * 1024;
  DeviceBuffer srgb_lut;  // edit.hip: avg_albedo's linear->sRGB curve per (voxel count, colour sum), built on first use
  uint64_t sync_epoch = 1;  // bumped whenever the library has waited for the stream: what was enqueued before is done
  // The surfel pass of a frame runs on a second stream of the context (run_surfel_pass): it is launched in its own frame, behind
  // that frame's final gather, and only has to be complete before the NEXT final gather reads the hash -- so the next frame's
  // primary / AO kernel runs beside it, each side on its share of the workgroup slots. Nothing is kept back:
  // what conflicts with it on the main stream (the next gather, a scene commit, anything that touches the GI state) waits
  // for `ev_side_done` first (join_side); every wait for the context covers both streams (sync_stream).
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_side_done = nullptr;
  bool side_busy = false;
  std::vector<hipStream_t> extra_streams;  // communicators' gather streams (comm.hip): they read pipelines' planes, so every wait for the context covers them
  hipStream_t copy = nullptr;  // scene commits upload on a stream of their own (the copy engine), beside the frame in flight -- never between two frames
  // Which frames of the stream have STARTED (FrameArgs::started_word): a word of pinned host memory that the first traversal launch of
  // every frame writes its sequence number into. `frame_seq` counts those launches as they are enqueued. 0 / null: not available.
  volatile uint32_t* started = nullptr;
  uint32_t frame_seq = 0;
  // Device staging of the SYNCHRONOUS calls (scene queries, island lookups and detaches): what the call uploads, what it downloads, and a
  // third array where a call has one (the box queries' records). Grown on demand (grow), shared by every kind: such a call has drained the
  // stream before it returns, so no two users overlap.
  DeviceBuffer stage_in, stage_out, stage_aux;
  // the scene queries' two work counters (a launch takes queries from one and zeroes the other for the next: query_parity says which is whose)
  DeviceBuffer query_counters;
  uint32_t query_parity = 0;
  // model islands (island.hip): the device-side scratch of a labelling or a detach besides the model's own label array -- a bit and a
  // counter per 64 keys, block sums, the records being accumulated
  DeviceBuffer island_mask, island_count, island_tmp, island_acc, island_records;
  // model stamps (stamp.hip): the source of a dust_hip_model_stamp call as a brick-major grid (16 MiB, allocated by the first call that
  // needs it) -- expanded from a source that is not editable, or the copy of a model stamped onto itself. Filled by every such call:
  // nothing is cached across calls
  DeviceBuffer stamp_grid;
  // model reductions (reduce.hip): the grid the levels of a dust_hip_model_reduce call with levels >= 2 take turns with the new model's
  // (16 MiB, allocated by the first such call). A grid of its own: stamp_grid may hold the expansion of the source the first level reads
  DeviceBuffer reduce_grid;
  // model floods (flood.hip): the worklists of a dust_hip_model_flood call -- two flag arrays and two brick lists that take turns, their
  // lengths and the accumulator of the result (dust::kFloodWorkWords); 4 MiB, allocated by the first call
  DeviceBuffer flood_work;
  // model casts (cast.hip): the brick masks of a dust_hip_model_cast source that is not editable (2 MiB, EditArgs::brick_mask's layout),
  // scattered from its blocks by every such call: nothing is cached across calls
  DeviceBuffer cast_mask;
  // model censuses (census.hip): one chunk's cell lists. The context's, not an EditState's: the model of a dust_hip_model_census may not
  // be editable (its shape records, accumulators and tables go through stage_in / stage_out / stage_aux)
  DeviceBuffer census_cells, census_starts, census_ids;
  // model surfaces (surface.hip): the listed voxels per brick of a dust_hip_model_surface call that lists, scanned in place, with the
  // scan's block sums and total behind them (1 MiB, allocated by the first such call). The context's: the model may not be editable.
  // A dust_hip_model_mesh call that lists (mesh.hip) keeps its quads per (direction, slice) in the same table: both calls are synchronous
  DeviceBuffer surface_table;
  // model deltas (delta.hip): a dust_hip_model_delta call reads two models at once. One that is not editable goes through cast_mask and
  // stamp_grid; when neither is, the second goes through this pair (2 MiB and 16 MiB, allocated by the first call that needs them).
  // Its listed voxels per brick are kept in surface_table
  DeviceBuffer delta_mask, delta_grid;
  // model settling (settle.hip): three arrays in EditArgs::brick_mask's layout (6 MiB, allocated by the first call that needs them) --
  // the loose voxels of every brick, and the pair of masks a slide writes beside the scratch grid
  DeviceBuffer settle_masks;
  // model voxelisation (triangle.hip): the inside bit of every voxel of a dust_hip_model_fill_mesh call, in EditArgs::brick_mask's
  // layout (2 MiB, allocated by the first such call; zeroed by every call)
  DeviceBuffer fill_volume;
  // model boxes (boxes.hip): a bit plane per slice of a dust_hip_model_boxes call's stacking axis -- the rects that continue the slice
  // before (2 MiB, allocated by the first such call). Every call writes the planes of the slices it reads: nothing is cached across calls
  DeviceBuffer boxes_volume;
};
// wait for everything enqueued on the context's streams (and remember that we did: scene commits recycle their pinned staging
// slots by this, without an event per commit)
hipError_t sync_stream(DustHipContext* c);
hipError_t join_side(DustHipContext* c);  // main stream: wait (on the device) for the side stream's pass, if one may still be running
hipError_t fork_side(DustHipContext* c);  // side stream: everything enqueued on the main stream so far comes first
// A buffer that only grows: too small, the streams are drained (sync_stream) before the old allocation goes, and the new one has half
// as much again. Out of device memory: the buffer is left released, DUST_ERR_OUT_OF_MEMORY.
DustStatus grow(DustHipContext* ctx, DeviceBuffer& b, size_t bytes);
const char* diag_env(const char* name);  // "NO_FUSE" -> $DUST_HIP_NO_FUSE: the library's one environment lookup (capi.cpp)
void release(DustHipContext* c);

// a uint16 per voxel of an editable model (field.hpp). `count`: the voxels that hold a value (0: an apply call has nothing to visit);
// `box`: the root cells that hold them -- the flood's reached voxels' bounds while count != 0, every cell for a distance field
struct VoxelField {
  DeviceBuffer values;
  bool valid = false;
  uint32_t count = 0;
  dust::CellBox box{};
};

// device-side voxel edits (edit.hip): the dense voxel grid and the scratch tables of the rebuild, created on a model's first edit
struct EditState {
  DeviceBuffer grid, brick_mask, flag_leaf, count_major, scan_tmp, header;
  DeviceBuffer xyz, values;  // a set_voxels / get_voxels call's coordinates and values, grown on demand
  // shape edits (dust_hip_model_edit_shapes): the call's shape records and counters, and one chunk's cell lists, grown on demand
  DeviceBuffer shapes, changed, shape_cells, shape_starts, shape_ids;
  // model islands (dust_hip_model_find_islands): per voxel, indexed by x << 16 | y << 8 | z, the key of its island (64 MiB, allocated by
  // the first labelling); valid until the next set_voxels / edit_shapes that may change a voxel
  DeviceBuffer labels;
  bool labels_valid = false;
  uint32_t labels_corners = 0;  // the connectivity of that labelling
  // model floods and model distances (dust_hip_model_flood, dust_hip_model_distance): per voxel, brick-major like the grid, its step
  // distance from the seeds / its distance to the nearest target (32 MiB each, allocated by the first call); valid until the next call
  // that may change a voxel
  VoxelField flood, distance;
  // model fracture (dust_hip_model_fracture): per voxel the index of its cell, DUST_HIP_NO_CELL where it has none (32 MiB, allocated by
  // the first call); `box` the root cells of the call's region; fracture_seeds the n_seeds of that call: the cell indices a detach may name
  VoxelField fracture;
  uint32_t fracture_seeds = 0;
};

struct DustHipModel : RefCounted {
  DustHipContext* ctx = nullptr;  // retained
  DeviceBuffer root, l2, l2_cells, mid, dense_mask, blocks, materials, palette;
  std::vector<uint8_t> host_root;  // 640 B: mask + prefix, what the kernels stage in LDS
  dust::DevModel dev{};
  uint32_t id = 0;
  uint64_t n_materials = 0;
  uint32_t n_mid = 0, n_l2 = 0;  // mid nodes and l2 nodes in use (an editable model's mid / dense_mask buffers hold room for 4096)
  uint32_t generation = 0;  // bumped by every edit: scenes record it at commit and refuse to render a stale copy
  bool has_material_255 = false;  // the edit grid stores palette index + 1 in a byte: such a model cannot become editable
  std::unique_ptr<EditState> edit;
};
void release(const DustHipModel* m);

struct HostInstance {
  const DustHipModel* model;  // retained
  float o2w[12];
  float prev[16];
};

// Where a committed scene lives on the device: ONE allocation, the arrays at offsets inside it -- what depends on the models
// first, what depends on the instance transforms behind it. A commit fills a pinned host image of the same layout and sends
// it (all of it after a structural change, the transform-dependent tail otherwise) with one asynchronous copy on the context's
// stream (tlas.rs:37-65 rebuilds the TLAS inside the frame's command stream the same way): no allocation, no wait, and the
// kernels' pointers stay what they were until instances are added.
struct SceneLayout {
  size_t models = 0, root_table = 0, instances = 0, boxes = 0, visits = 0, enters = 0, gboxes = 0, sboxes = 0, grid_cells = 0, grid_items = 0, total = 0;
  size_t cap_cells = 0, cap_items = 0;  // entries the two grid sections hold (a commit that needs more lays the image out again)
  static SceneLayout make(size_t n_inst, size_t n_models, size_t n_roots, size_t n_cells, size_t n_items) {
    SceneLayout l;
    auto place = [&l](size_t bytes) { const size_t at = l.total; l.total = (l.total + bytes + 255) & ~size_t(255); return at; };
    l.models = place(n_models * sizeof(dust::DevModel));
    l.root_table = place(n_roots * dust::kN16LdsBytes);
    l.instances = place(n_inst * sizeof(dust::DevInstance));
    l.boxes = place((n_inst + 1) * sizeof(dust::DevBox));
    l.visits = place((n_inst + 1) * sizeof(dust::DevVisit));
    l.enters = place((n_inst + 1) * sizeof(dust::DevEnter));
    l.gboxes = place(((n_inst + 63) / 64 + 1) * sizeof(dust::DevBox));  // the packet cull's hierarchy (scenes beyond kFlatCullMax instances)
    l.sboxes = place((n_inst + 1) * sizeof(dust::DevBox));
    // the top-level grid last, with room to spare: its size follows the instances' positions, not only their number
    l.cap_cells = n_cells + n_cells / 2 + 64;
    l.cap_items = n_items + n_items / 2 + 256;
    l.grid_cells = place((l.cap_cells + 4) * sizeof(uint32_t));
    l.grid_items = place((l.cap_items + 8) * sizeof(uint16_t));
    return l;
  }
};

struct DustHipScene : RefCounted {
  DustHipContext* ctx = nullptr;  // retained
  std::vector<HostInstance> instances;
  std::vector<uint8_t> dirty;                // per instance: transform changed since the last commit
  std::vector<const DustHipModel*> models;   // distinct models, index == DevModel slot (kept alive through `instances`)
  std::vector<uint32_t> model_generation;    // their edit generations when the scene was committed
  std::vector<uint32_t> instance_slot;       // per instance: its model's slot
  bool structure_dirty = true;               // instances were added (or a model edited): slots, roots and capacity are re-derived
  // The device image is a RING of kImages copies, each with a pinned host twin. A commit writes the whole image into the next
  // slot -- on the context's copy stream, waited for by the host, so nothing is enqueued between two frames on the launch stream
  // (one stream-ordered copy per frame used to cost a moving scene ~25 us of a 230 us frame: wait for the frame, copy, start the
  // next) -- and frames enqueued from then on read that slot. A slot is rewritten kImages commits later: the frames that read it
  // are done if the library has waited for the streams since they were enqueued (a frame loop does, to read its result or pace
  // itself); otherwise the host is kImages commits ahead of the GPU and waits here (the reference's host runs <= 3 frames ahead).
#ifndef DUST_SCENE_IMAGES
#define DUST_SCENE_IMAGES 16   // (8 until dust_hip_render_frames took moves: a launch of eight frames, each with an image of its own, left the host no image to
#endif                        //  prepare the next launch in while that one ran -- 0.2457 ms per frame of a moving view against 0.2257 with 16; an image is ~150 KB for the castle)
  static constexpr int kImages = DUST_SCENE_IMAGES;
  struct Slot {
    DeviceBuffer dev;
    void* host = nullptr;
    mutable uint64_t epoch = 0;  // the context's sync_epoch when a frame reading the slot was last enqueued
    mutable uint32_t last_seq = 0;  // ... and that frame's start sequence number (DustHipContext::frame_seq), 0 = it has none (no traversal launch, or no word)
  } slots[kImages];
  int current = -1;           // the slot frames read
  uint32_t next_slot = 0;
  SceneLayout layout;
  size_t image_capacity = 0;  // bytes per slot
  std::vector<uint8_t> master;   // host master copy of the image (dirty instances are re-derived in place)
  float world_min[3] = {0, 0, 0}, world_max[3] = {0, 0, 0};  // union of the instances' world boxes
  // the top-level grid over the instance boxes (dust_dev.h DevGrid; rebuilt by every commit): its header, and the two arrays
  // that are copied into the image
  dust::DevGrid grid{};
  bool grid_valid = true;            // false: some cell would list more instances than a cell word counts (the ray streams then stay off)
  std::vector<uint32_t> grid_cells;
  std::vector<uint16_t> grid_items;
  std::vector<uint32_t> slot_order;  // large scenes: the instances along a space-filling curve (made by a structural commit; a moved instance keeps its slot)
  uint32_t n_groups = 0;             // ... and how many groups of 64 consecutive slots (0: the cull tests every box)
  std::vector<float> world_boxes;  // per instance {lo[3], hi[3]}: what derive_instance writes into the image, kept for the grid
  uint32_t n_lds_models = 0;
  uint64_t revision = 0;  // bumped by every commit (what the cost-ordered hand-out keys its view on)
  bool committed = false;
  const uint8_t* dev(size_t off) const { return static_cast<const uint8_t*>(slots[current].dev.p) + off; }
  void touch() const { slots[current].epoch = ctx->sync_epoch; slots[current].last_seq = 0; }  // a frame reading the current slot is being enqueued
  void free_images() {  // (the caller has waited for the streams)
    for (Slot& sl : slots) {
      if (sl.host) { (void)hipHostFree(sl.host); sl.host = nullptr; }
      sl.dev.release();
      sl.epoch = 0; sl.last_seq = 0;
    }
    current = -1;
    image_capacity = 0;
  }
};
void release(const DustHipScene* s);
// a frame or a query reads the scene as committed: refused while it has uncommitted changes or a model was edited since
DustStatus check_scene_ready(const DustHipScene* s);

// the scene half of a launch descriptor: the current image's arrays (frames and scene ray queries)
inline void scene_args(const DustHipScene* s, dust::FrameArgs& a) {
  a.models = reinterpret_cast<const dust::DevModel*>(s->dev(s->layout.models));
  a.instances = reinterpret_cast<const dust::DevInstance*>(s->dev(s->layout.instances));
  a.n_models = uint32_t(s->models.size());
  a.n_instances = uint32_t(s->instances.size());
  a.n_lds_models = s->n_lds_models;
  a.root_table = s->dev(s->layout.root_table);
  a.boxes = reinterpret_cast<const dust::DevBox*>(s->dev(s->layout.boxes));
  a.visits = reinterpret_cast<const dust::DevVisit*>(s->dev(s->layout.visits));
  a.grid = s->grid;
  // (a grid that could not list every box -- build_grid -- is not handed to the kernels at all: the packet kernels, which never read it, run instead)
  a.grid.cells = s->grid_valid ? reinterpret_cast<const uint32_t*>(s->dev(s->layout.grid_cells)) : nullptr;
  a.grid.items = s->grid_valid ? reinterpret_cast<const uint16_t*>(s->dev(s->layout.grid_items)) : nullptr;
  a.enters = reinterpret_cast<const dust::DevEnter*>(s->dev(s->layout.enters));
  a.gboxes = reinterpret_cast<const dust::DevBox*>(s->dev(s->layout.gboxes));
  a.sboxes = reinterpret_cast<const dust::DevBox*>(s->dev(s->layout.sboxes));
  a.n_groups = s->n_groups;
}
