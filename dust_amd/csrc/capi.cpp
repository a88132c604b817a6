// capi.cpp -- the extern "C" boundary (include/dust_hip.h) and the host runtime behind it: the host-side wrappers, the context,
// persistent pipeline buffers, pass scheduling. Models live in capi_model.cpp, scenes and scene queries in capi_scene.cpp. What the frame
// path computes without a device -- every launch's shape, the tile schedule's decisions -- is frame_plan.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>

#include "capi_internal.hpp"
#include "frame_plan.hpp"
#include "vdb.hpp"
#include "png.hpp"
#include "sky.hpp"
#include "denoise.hpp"
#include "query.hpp"

namespace dust {
hipError_t launch_primary(const FrameArgs& a, uint32_t grid, uint32_t block, bool count, hipStream_t);
hipError_t launch_ambient_occlusion(const FrameArgs& a, uint32_t grid, uint32_t block, bool count, hipStream_t);
hipError_t launch_primary_ao(const FrameArgs& a, uint32_t grid, uint32_t block, bool count, hipStream_t);
hipError_t launch_primary_ao_batch(const FrameArgs* frames, uint32_t n, uint32_t grid, uint32_t block, hipStream_t);
hipError_t launch_final_gather(const FrameArgs& a, uint32_t grid, uint32_t block, bool count, bool commit, hipStream_t);
hipError_t launch_final_gather_shade(const FrameArgs& a, bool commit, hipStream_t);
hipError_t launch_gather_order(const FrameArgs& a, uint32_t n_tiles, hipStream_t);
hipError_t launch_gi_export(const FrameArgs& a, hipStream_t);
hipError_t launch_gi_import(const FrameArgs& a, hipStream_t);
hipError_t launch_surfel_keys(const FrameArgs& a, hipStream_t);
size_t radix_sort_scratch_bytes(uint32_t n);
hipError_t radix_sort_pairs(void* scratch, uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, uint32_t n,
                            uint32_t key_bits, bool* in_b, hipStream_t s);
hipError_t launch_surfel_trace(const FrameArgs& a, uint32_t grid, uint32_t block, bool count, hipStream_t);
hipError_t launch_surfel_apply(const FrameArgs& a, int mode, hipStream_t);
hipError_t launch_surfel_unstage(const FrameArgs& a, hipStream_t);
hipError_t launch_gather_rays(const FrameArgs& a, hipStream_t);
hipError_t launch_surfel_rays(const FrameArgs& a, hipStream_t);
hipError_t launch_surfel_shade(const FrameArgs& a, hipStream_t);
hipError_t launch_ray_walk(const FrameArgs& a, int rt, uint32_t grid, uint32_t block, bool count, hipStream_t);
hipError_t launch_accumulate(const FrameArgs& a, hipStream_t);
hipError_t launch_tone_map(const uint16_t* src, const uint32_t* albedo, uint16_t* dst, uint32_t n_pixels, uint32_t* hist, float* avg,
                           float min_log, float log_range, float time_coeff, const float conv[9], uint32_t tf, hipStream_t s);
hipError_t configure_kernels(size_t max_lds);
hipError_t launch_tile_order(const uint32_t* cost, uint32_t* order, uint32_t* cuts, bool reuse_cuts, uint32_t total, uint32_t per, hipStream_t s);
hipError_t launch_cost_blend(const uint32_t* raw, uint32_t* smooth, uint32_t total, uint32_t keep_shift, hipStream_t s);
hipError_t launch_cost_dilate(const uint32_t* in, uint32_t* out, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s);
hipError_t launch_device_eval(uint32_t fn, const uint32_t* in, uint32_t in_words, uint32_t* out, uint32_t out_words, uint32_t n, const float* sky,
                              hipStream_t s);
}  // namespace dust

namespace {
// sky.glsl:81-113 (sun disc radiance, limb darkening) at the sun's own direction, times the solid-angle factor of
// nee.rmiss:11-22, in single precision like the shader. The kernels read the result as a launch constant.
void sun_constants(const float* s, float* dir, float* term) {
  const float len = std::sqrt((s[48] * s[48] + s[49] * s[49]) + s[50] * s[50]);
  const float d[3] = {s[48] / len, s[49] / len, s[50] / len};
  for (int k = 0; k < 3; ++k) { dir[k] = d[k]; term[k] = 0.0f; }
  const float len2 = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);  // the shader normalises the direction again
  const float e[3] = {d[0] / len2, d[1] / len2, d[2] / len2};
  const float cos_gamma = (e[0] * s[48] + e[1] * s[49]) + e[2] * s[50];
  if (!(cos_gamma >= 0.0f) || e[1] < 0.0f) return;
  const float sol_rad_sin = std::sin(s[55]);
  const float ar2 = 1.0f / (sol_rad_sin * sol_rad_sin);
  const float singamma = 1.0f - cos_gamma * cos_gamma;
  const float sc2 = 1.0f - (ar2 * singamma) * singamma;
  if (!(sc2 > 0.0f)) return;
  const float sc = std::sqrt(sc2);
  float dark[3] = {s[10] + s[11] * sc, s[26] + s[27] * sc, s[42] + s[43] * sc};
  float cur = sc;
  for (int i = 0; i < 4; ++i) {
    cur *= sc;
    dark[0] += s[12 + i] * cur; dark[1] += s[28 + i] * cur; dark[2] += s[44 + i] * cur;
  }
  const float v[3] = {s[52] * dark[0], s[53] * dark[1], s[54] * dark[2]};
  const float kk = 1.0f - std::cos(s[55]);
  term[0] = ((1.6410228f * v[0] + -0.32480323f * v[1]) + -0.23642465f * v[2]) * kk;   // color.glsl:24-31
  term[1] = ((-0.66366285f * v[0] + 1.6153315f * v[1]) + 0.016756356f * v[2]) * kk;
  term[2] = ((0.011721907f * v[0] + -0.0082844375f * v[1]) + 0.9883947f * v[2]) * kk;
}
}  // namespace

static thread_local std::string g_last_error;  // dust_hip_last_error() of the calling thread (dust_internal::set_error writes it)

struct DustVdbTree { dust::vdb::Tree tree; DustVdbTree(const uint32_t* f, int n) : tree(f, n) {} };
struct DustVdbAccessor { dust::vdb::Tree::Accessor acc; explicit DustVdbAccessor(const dust::vdb::Tree& t) : acc(t) {} };
struct DustVdbPool { dust::vdb::Pool pool; DustVdbPool(size_t b, unsigned c) : pool(b, c) {} };
struct DustVoxScene { dust::vox::Scene scene; };
struct DustSkyDataset { dust::sky::Dataset data; };

hipError_t sync_stream(DustHipContext* c) {
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess && c->side) { e = hipStreamSynchronize(c->side); c->side_busy = false; }
  for (hipStream_t x : c->extra_streams)
    if (e == hipSuccess) e = hipStreamSynchronize(x);
  if (e == hipSuccess) ++c->sync_epoch;
  return e;
}
hipError_t join_side(DustHipContext* c) {
  if (!c->side_busy) return hipSuccess;
  c->side_busy = false;
  return hipStreamWaitEvent(c->stream, c->ev_side_done, 0);
}
hipError_t fork_side(DustHipContext* c) {
  hipError_t e = hipSuccess;
  if (!c->side) {
    e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_side_done, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  e = hipEventRecord(c->ev_fork, c->stream);
  return e != hipSuccess ? e : hipStreamWaitEvent(c->side, c->ev_fork, 0);
}
DustStatus grow(DustHipContext* ctx, DeviceBuffer& b, size_t bytes) {
  if (b.p && b.bytes >= bytes) return DUST_OK;
  HIP_TRY(sync_stream(ctx));
  const hipError_t e = b.alloc(std::max(bytes + bytes / 2, size_t(4096)));
  if (e == hipSuccess) return DUST_OK;
  b.release();
  if (e != hipErrorOutOfMemory) return hip_fail(e, "growing a device buffer");
  (void)hipGetLastError();  // (the error is sticky until read)
  return fail(DUST_ERR_OUT_OF_MEMORY, "device memory for a buffer that grows on demand");
}
void release(DustHipContext* c) {
  if (!c || c->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
  if (c->copy) { (void)hipStreamSynchronize(c->copy); (void)hipStreamDestroy(c->copy); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_side_done) (void)hipEventDestroy(c->ev_side_done);
  if (c->started) (void)hipHostFree(const_cast<uint32_t*>(c->started));
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;  // (and with it the context's device buffers)
}

// What decides which kernels a pipeline's frames run. Two kinds, kept apart:
//  * PRODUCTION knobs arrive through the C ABI (DustHipPipelineConfig, dust_hip_pipeline_configure): slots left free for other queues'
//    kernels, which form the GI passes take, the surfel pass's second stream and its share, how several frames in flight split the slots;
//  * DIAGNOSTIC switches (ablations, A/B runs, the stress drivers' random draws) come from the environment, read ONCE when a pipeline
//    is created through the one lookup below. None of them is needed for any production frame; DESIGN.md section 9 lists them.
const char* diag_env(const char* name) {   // "NO_FUSE" -> $DUST_HIP_NO_FUSE (the library's only environment lookup besides DUST_HIP_DEBUG-class reads here)
  char full[64];
  std::snprintf(full, sizeof full, "DUST_HIP_%s", name);
  return std::getenv(full);
}
struct Tuning {
  // ---- production (DustHipPipelineConfig)
  uint32_t reserve_blocks = 0xFFFFFFFFu;  // workgroup slots left free for another queue's kernels; 0xFFFFFFFF = auto (32 once the pipeline has taken part in a collective of world > 1)
  uint32_t gi_path = DUST_GI_PATH_AUTO;   // packets / ray streams (auto: packets, except the final gather of a scene with a 4096^3 tree)
  bool no_side_stream = false;            // the surfel pass on the main stream, in place
  uint32_t side_share = 0;                // percent of the workgroup slots the surfel pass takes on the second stream (0: calibrated)
  uint32_t in_flight_slots = DUST_IN_FLIGHT_SHARE;  // frames in flight: every launch on 1/n of the slots, or every launch asking for all of them
  // ---- diagnostics (environment)
  uint32_t debug = 0;           // DEBUG ablation bits (FrameArgs::debug)
  uint32_t block = 512;         // BLOCK: threads per workgroup, whole wavefronts, <= the kernels' launch bounds
  uint32_t blocks_per_cu = 2;   // BLOCKS_PER_CU
  bool no_fuse = false;         // NO_FUSE: primary and AO passes as two launches (the reference's shape)
  bool no_gather_order = false; // NO_GATHER_ORDER: plain 8x8 pixel packets in the final gather
  bool no_surfel_sort = false;  // NO_SURFEL_SORT: trace the surfel pool in pool order
  bool no_tile_order = false;   // NO_TILE_ORDER: hand tiles out in screen order, not most expensive first
  bool equal_bands = false;     // EQUAL_BANDS: bands of equal tile count (round 3) instead of equal measured cost
  bool no_lds_boxes = false;    // NO_LDS_BOXES: the packet cull reads the instance boxes from memory
  uint32_t static_rounds = 0xFFFFFFFFu;  // STATIC_ROUNDS: dealt rounds of the hand-out (default: one, kernels.hip with_schedule)
  uint32_t still_refresh_max = 64;  // cap of the launches between two re-measurements of a view that stands still
  uint32_t cost_keep_shift = 1; // a tile's cost estimate moves 1 / 2^k of the way to each new measurement
  bool wide_fused = true;       // NO_WIDE_FUSED: the fused kernel always as two 512-thread workgroups per CU
  bool dilate = true;           // NO_DILATE: a moving view's order from the tiles' own costs only
  bool force_moving = false;    // FORCE_MOVING: treat every view as a moving one
  uint32_t cuts_reuse = 4;      // re-orderings of a moving view that keep one set of band cuts
  uint32_t moving_refresh = 4;  // launches between two re-orderings of a view that moves (order_tiles)
  uint32_t side_prio = 3;       // issue priority floor of the surfel pass on the second stream
  uint32_t stream_refill = 16;  // STREAM_REFILL, STREAM_TOP_ITERS: FrameArgs::stream_refill / stream_top_iters
  uint32_t stream_top_iters = 8;
  uint32_t in_flight_oversub = 0;  // IN_FLIGHT_OVERSUB (percent)
  bool wide_share = false;         // WIDE_SHARE: two frames in flight on half of the slots each as 1024-thread workgroups, one per CU (experiment)
  bool no_stream_lds = false;   // NO_STREAM_LDS: the ray streams read grid, boxes and enter records from memory
  bool no_shared_view = false;  // NO_SHARED_VIEW: same-view frames of a launch each trace their own camera and sun rays (k_primary_ao_batch, never k_primary_ao_runs)
  static uint32_t num(const char* name, uint32_t dflt) {
    const char* e = diag_env(name);
    return e ? uint32_t(std::strtoul(e, nullptr, 10)) : dflt;
  }
  static bool flag(const char* name) { return diag_env(name) != nullptr; }
  static Tuning from_environment() {
    Tuning t;
    t.debug = num("DEBUG", 0);
#ifndef DUST_MAX_BLOCK
#define DUST_MAX_BLOCK 512u   // the kernels' launch bounds (an experiment build may raise both)
#endif
    t.block = std::min(DUST_MAX_BLOCK, std::max(128u, num("BLOCK", 512) & ~127u));  // <= the kernels' launch bounds (512); an even number of
                                                                                    // waves keeps the LDS areas behind the per-wave lists 16-byte aligned
    t.blocks_per_cu = std::max(1u, num("BLOCKS_PER_CU", 2));
    t.no_fuse = flag("NO_FUSE");
    t.no_gather_order = flag("NO_GATHER_ORDER");
    t.no_surfel_sort = flag("NO_SURFEL_SORT");
    t.no_tile_order = flag("NO_TILE_ORDER");
    t.equal_bands = flag("EQUAL_BANDS");
    t.no_lds_boxes = flag("NO_LDS_BOXES");
    t.no_stream_lds = flag("NO_STREAM_LDS");
    t.stream_refill = std::min(64u, std::max(1u, num("STREAM_REFILL", 16)));
    t.stream_top_iters = std::max(1u, num("STREAM_TOP_ITERS", 8));
    t.static_rounds = num("STATIC_ROUNDS", 0xFFFFFFFFu);
    t.dilate = !flag("NO_DILATE");
    t.wide_fused = !flag("NO_WIDE_FUSED") && !flag("BLOCK");
    t.force_moving = flag("FORCE_MOVING");
    t.in_flight_oversub = std::min(100u, num("IN_FLIGHT_OVERSUB", 0));
    t.wide_share = flag("WIDE_SHARE");
    t.no_shared_view = flag("NO_SHARED_VIEW");
    return t;
  }
};

struct DustHipPipeline {
  DustHipContext* ctx = nullptr;  // retained
  Tuning tune;
  uint32_t frames_in_flight = 1;  // dust_hip_pipeline_set_frames_in_flight
  bool in_collective = false;     // the pipeline has taken part in a collective of a communicator with world > 1 (comm.hip): DUST_RESERVE_AUTO then leaves 32 slots free
  uint32_t width = 0, height = 0;
  DeviceBuffer planes[DUST_PLANE_COUNT];
  void* bound[DUST_PLANE_COUNT] = {};  // caller-owned storage a plane was redirected to (dust_hip_pipeline_bind_plane), or null
  void* plane(int i) const { return bound[i] ? bound[i] : planes[i].p; }
  DeviceBuffer noise0, noise5, counters, stats;
  uint32_t counter_parity[4] = {0, 0, 0, 0};  // per pass kind: which of its two counter sets the next launch uses
  // per pass kind: cycles each tile took in the pass's last launch and the hand-out order made from them (k_tile_order);
  // valid for the tile grid they were recorded on
  struct TileHistory : dust::TileState {   // (the schedule's state and its step function: frame_plan.hpp)
    DeviceBuffer cost, order;
    DeviceBuffer spread;     // a moving view: each tile's estimate or its dearest neighbour's (k_cost_dilate)
    DeviceBuffer smooth;     // running mean of the measurements of each tile: what the order is made from (k_cost_blend)
    DeviceBuffer cuts;       // kRegions + 1 tile indices: the cost-balanced bands order[] was made for (FrameArgs::band_cuts)
  } tile_history[4];
  uint64_t view_key = 0;     // this frame's camera + scene revision + sun + row band
  DeviceBuffer exposure;  // Histogram {u32 histogram[256]; f32 avg} (auto_exposure.playout)
  // hash-fed GI state (standard.rs:334-358): spatial hash, surfel pool, per-frame scratch
  DeviceBuffer gi_hash, gi_pool, gi_owner, gi_pixel_surfel, gi_requests, gi_replacement, gi_sun_payload;
  DeviceBuffer gi_apply_alive, gi_apply_dead;  // the deterministic apply's marks (k_surfel_apply_mark)
  DeviceBuffer gi_sort_keys[2], gi_sort_vals[2], gi_sort_scratch;  // radix sort ping-pong (position order of the pool, then the apply order)
  DeviceBuffer gi_fg_hits;  // per pixel: the hit record of its gather ray (k_ray_stream / k_final_gather -> k_final_gather_shade)
  // ray streams (gi.hip): the compacted rays of the two GI passes, the surfel rays' hit records, and per pass two ray counters used in turn
  DeviceBuffer gi_rays_fg, gi_rays_sf, gi_hits_sf, gi_groups_fg, gi_groups_sf, gi_unbinned;
  DeviceBuffer gi_order, gi_order_count;  // final gather: live pixels of each 64x64 tile grouped by ray direction bin
  DeviceBuffer gi_touched, gi_merged;  // multi-GPU exchange buffers (dust_hip_pipeline_gi_exchange)
  // sharded surfel trace (DustHipFrameParams::surfel_world >= 1): the records in slot order (made on first use, gi_stage_slots slots each;
  // released by dust_hip_pipeline_configure_gi), and what the pending pass's second half (dust_hip_gi_surfel_exchange_run) needs of its first
  DeviceBuffer gi_stage_req, gi_stage_repl, gi_stage_sun;
  size_t gi_stage_slots = 0;
  struct { bool pending = false; const uint32_t* perm = nullptr; uint32_t rank = 0, world = 0, slots_per_rank = 0; } sf_shard;
  uint32_t gi_touched_rows = 0;
  uint32_t gi_capacity = 0, gi_pool_size = 0;
  uint32_t noise0_layers = 0, noise5_layers = 0;
  uint32_t accum_count = 0;
  // DUST_PASS_DENOISE: two history sets used in turn {rgb + frame count (16 B); depth, normal, instance as one 16 B record}, the camera
  // of the frame that wrote the current one, and the filter's settings
  DeviceBuffer hist_accum[2], hist_geo[2];
  uint32_t hist_parity = 0;
  bool have_history = false;
  bool hist_traded = true;  // the radiance history is DUST_PLANE_ACCUM's own buffer (not a caller-bound one)
  dust::DevCamera prev_cam{};
  DustHipDenoiseParams denoise{sizeof(DustHipDenoiseParams), 30, 0.01f, 2.0f, 0.8f, 15.0f};
  // HIP-event pairs around the launches of the four pass kinds (primary or fused, AO, final gather, surfel pass), a ring per kind:
  // the last pair is what dust_hip_pipeline_pass_stats reports, the pairs since the last mark what dust_hip_pipeline_kernel_times sums
  static constexpr uint32_t kEvRing = 256;
  std::vector<hipEvent_t> ev_ring[4][2];
  uint32_t ev_head[4] = {0, 0, 0, 0}, ev_mark[4] = {0, 0, 0, 0};
  hipEvent_t ev_begin(int kind) { return ev_ring[kind][0][ev_head[kind]++ % kEvRing]; }
  hipEvent_t ev_end(int kind) { return ev_ring[kind][1][(ev_head[kind] - 1u) % kEvRing]; }
  bool ev_valid[4] = {false, false, false, false};  // primary, ao
  bool stats_valid = false;
  bool fused_last = false;  // the last frame ran primary + AO as one kernel: its time is reported under pass 0
  uint32_t frame_counter = 0;
  bool timed_frame = false;  // this frame's launches are bracketed by event pairs (see dust_hip_render_frame)
  dust::DevStats* host_stats = nullptr;  // pinned, 8 records: where the counting build's statistics land
  // How the workgroup slots are split while a surfel pass runs beside the next frame's primary / AO kernels: the pipeline's first
  // GI frame runs its surfel pass in place and is timed (P: primary / AO kernels, Q: the pass); once those events have completed --
  // looked at without waiting, some frames later -- the pass's share is 100 Q / (Q + 1.05 P) - 3, which is where the measured optima
  // of three workloads lie (castle 1080p 50 %, 4K 20 %, the 4096^3 tree 25 %). Until then: a guess from the ray counts.
  struct { hipEvent_t p0 = nullptr, p1 = nullptr, q0 = nullptr, q1 = nullptr; int state = 0; uint32_t share = 0; uint32_t gi_frames = 0; } side_cal;
};

static const size_t kPlaneBytesPerPixel[DUST_PLANE_COUNT] = {8, 8, 4, 4, 4, 8, 4, 16, 8};

extern "C" {

const char* dust_hip_last_error(void) { return g_last_error.c_str(); }

int dust_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ===================================================================== vdb
DustStatus dust_vdb_tree_create(const uint32_t* fanout_log2, uint32_t n_levels, DustVdbTree** out) {
  if (!fanout_log2 || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] { *out = new DustVdbTree(fanout_log2, int(n_levels)); return DUST_OK; });
}
void dust_vdb_tree_destroy(DustVdbTree* t) { delete t; }
DustStatus dust_vdb_tree_set(DustVdbTree* t, uint32_t x, uint32_t y, uint32_t z, int32_t value) {
  if (!t) return fail(DUST_ERR_INVALID_ARGUMENT, "null tree");
  const uint32_t e = 1u << t->tree.extent_log2();
  if (x >= e || y >= e || z >= e) return fail(DUST_ERR_INVALID_ARGUMENT, "coordinate outside the tree extent");
  return guarded([&] {
    if (!t->tree.set(x, y, z, value < 0 ? -1 : (value ? 1 : 0)))
      return fail(DUST_ERR_UNSUPPORTED, "clearing voxels through internal nodes is todo!() in the reference");
    return DUST_OK;
  });
}
DustStatus dust_vdb_tree_get(const DustVdbTree* t, uint32_t x, uint32_t y, uint32_t z, int32_t* value) {
  if (!t || !value) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  const uint32_t e = 1u << t->tree.extent_log2();
  if (x >= e || y >= e || z >= e) return fail(DUST_ERR_INVALID_ARGUMENT, "coordinate outside the tree extent");
  *value = t->tree.get(x, y, z);
  return DUST_OK;
}
DustStatus dust_vdb_tree_iter(const DustVdbTree* t, uint32_t* xyz, size_t cap, size_t* count) {
  if (!t || !count) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  size_t n = 0;
  t->tree.for_each_voxel([&](uint32_t x, uint32_t y, uint32_t z) {
    if (xyz && n < cap) { xyz[n * 3] = x; xyz[n * 3 + 1] = y; xyz[n * 3 + 2] = z; }
    ++n;
  });
  *count = n;
  return DUST_OK;
}
DustStatus dust_vdb_tree_iter_leaf(const DustVdbTree* t, uint32_t* xyz, uint64_t* occupancy, uint32_t* material_ptr,
                                   size_t cap, size_t* count) {
  if (!t || !count) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  size_t n = 0;
  t->tree.for_each_leaf([&](dust::vdb::LeafRef& l) {
    if (n < cap) {
      if (xyz) { xyz[n * 3] = l.origin[0]; xyz[n * 3 + 1] = l.origin[1]; xyz[n * 3 + 2] = l.origin[2]; }
      if (occupancy) occupancy[n] = l.occupancy;
      if (material_ptr) material_ptr[n] = *l.material_ptr;
    }
    ++n;
  });
  *count = n;
  return DUST_OK;
}
DustStatus dust_vdb_tree_meta(const DustVdbTree* t, uint32_t* meta_mask, uint32_t* root_level) {
  if (!t) return fail(DUST_ERR_INVALID_ARGUMENT, "null tree");
  if (meta_mask) *meta_mask = t->tree.meta_mask();
  if (root_level) *root_level = uint32_t(t->tree.root_level());
  return DUST_OK;
}
uint32_t dust_vdb_lca_level(const uint32_t a[3], const uint32_t b[3], uint32_t meta_mask, uint32_t root_level) {
  if (!a || !b) { (void)fail(DUST_ERR_INVALID_ARGUMENT, "null coordinates"); return 0xFFFFFFFFu; }
  return dust::vdb::Tree::lca_level(a, b, meta_mask, root_level);
}
DustStatus dust_vdb_accessor_create(const DustVdbTree* t, DustVdbAccessor** out) {
  if (!t || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] { *out = new DustVdbAccessor(t->tree); return DUST_OK; });
}
void dust_vdb_accessor_destroy(DustVdbAccessor* a) { delete a; }
DustStatus dust_vdb_accessor_get(DustVdbAccessor* a, uint32_t x, uint32_t y, uint32_t z, int32_t* value) {
  if (!a || !value) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  const uint32_t e = 1u << a->acc.tree().extent_log2();
  if (x >= e || y >= e || z >= e) return fail(DUST_ERR_INVALID_ARGUMENT, "coordinate outside the tree extent");
  *value = a->acc.get(x, y, z);
  return DUST_OK;
}
DustStatus dust_vdb_pool_create(size_t item_size, uint32_t chunk_size_log2, DustVdbPool** out) {
  if (!out || item_size < 4 || chunk_size_log2 > 24) return fail(DUST_ERR_INVALID_ARGUMENT, "bad pool parameters");
  return guarded([&] { *out = new DustVdbPool(item_size, chunk_size_log2); return DUST_OK; });
}
void dust_vdb_pool_destroy(DustVdbPool* p) { delete p; }
uint32_t dust_vdb_pool_alloc(DustVdbPool* p) {
  if (!p) { (void)fail(DUST_ERR_INVALID_ARGUMENT, "null pool"); return 0xFFFFFFFFu; }
  try { return p->pool.alloc(); } catch (...) { (void)fail(DUST_ERR_OUT_OF_MEMORY, "pool chunk allocation failed"); return 0xFFFFFFFFu; }
}
void dust_vdb_pool_free(DustVdbPool* p, uint32_t index) {
  if (!p || !p->pool.owns(index)) { (void)fail(DUST_ERR_INVALID_ARGUMENT, "index was not allocated from this pool"); return; }
  p->pool.free(index);
}
size_t dust_vdb_pool_num_chunks(const DustVdbPool* p) { return p ? p->pool.num_chunks() : 0; }
void dust_vdb_bitmask_set(uint64_t* words, size_t index, int32_t value) {
  if (!words) { (void)fail(DUST_ERR_INVALID_ARGUMENT, "null bit mask"); return; }
  dust::vdb::bit_set(words, index, value != 0);
}
size_t dust_vdb_bitmask_iter_set_bits(const uint64_t* words, size_t n_words, uint32_t* out, size_t cap) {
  if (!words && n_words) { (void)fail(DUST_ERR_INVALID_ARGUMENT, "null bit mask"); return 0; }
  size_t n = 0;
  dust::vdb::for_each_set_bit(words, n_words, [&](uint32_t i) {
    if (out && n < cap) out[n] = i;
    ++n;
  });
  return n;
}

// ===================================================================== vox
DustStatus dust_vox_load_frame(const uint8_t* bytes, size_t n_bytes, uint32_t frame, DustVoxScene** out) {
  if (!bytes || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    std::unique_ptr<DustVoxScene> s(new DustVoxScene);
    s->scene = dust::vox::load(bytes, n_bytes, frame);
    *out = s.release();
    return DUST_OK;
  });
}
DustStatus dust_vox_load(const uint8_t* bytes, size_t n_bytes, DustVoxScene** out) { return dust_vox_load_frame(bytes, n_bytes, 0, out); }
void dust_vox_scene_destroy(DustVoxScene* s) { delete s; }
DustStatus dust_png_load_array(const uint8_t* bytes, size_t n_bytes, DustPngInfo* info, uint8_t** texels) {
  if (!bytes || !info || !texels) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    const dust::png::ImageArray img = dust::png::load(bytes, n_bytes);
    uint8_t* out = static_cast<uint8_t*>(std::malloc(img.texels.size() ? img.texels.size() : 1));
    if (!out) throw std::bad_alloc();
    std::memcpy(out, img.texels.data(), img.texels.size());
    info->width = img.width; info->height = img.height; info->layers = img.layers;
    info->channels = img.channels; info->bytes_per_channel = img.bytes_per_channel;
    *texels = out;
    return DUST_OK;
  });
}
DustStatus dust_vox_scene_counts(const DustVoxScene* s, uint32_t* n_models, uint32_t* n_instances) {
  if (!s) return fail(DUST_ERR_INVALID_ARGUMENT, "null scene");
  if (n_models) *n_models = uint32_t(s->scene.models.size());
  if (n_instances) *n_instances = uint32_t(s->scene.instances.size());
  return DUST_OK;
}
DustStatus dust_vox_scene_model_info(const DustVoxScene* s, uint32_t model, DustVoxModelInfo* out) {
  if (!s || !out || model >= s->scene.models.size()) return fail(DUST_ERR_INVALID_ARGUMENT, "bad model index");
  const auto& m = s->scene.models[model];
  std::memcpy(out->size, m.size, sizeof(out->size));
  out->n_voxels = uint32_t(m.xyzi.size() / 4);
  out->n_blocks = uint32_t(m.blocks.size());
  out->n_materials = m.materials.size();
  out->used = m.used ? 1u : 0u;
  return DUST_OK;
}
DustStatus dust_vox_scene_model_data(const DustVoxScene* s, uint32_t model, const DustHipBlock** blocks,
                                     const uint8_t** materials) {
  if (!s || model >= s->scene.models.size()) return fail(DUST_ERR_INVALID_ARGUMENT, "bad model index");
  const auto& m = s->scene.models[model];
  if (blocks) *blocks = m.blocks.data();
  if (materials) *materials = m.materials.data();
  return DUST_OK;
}
DustStatus dust_vox_scene_palette(const DustVoxScene* s, const uint8_t** rgba) {
  if (!s || !rgba) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  *rgba = s->scene.palette;
  return DUST_OK;
}
DustStatus dust_vox_scene_instances(const DustVoxScene* s, DustVoxInstance* out, uint32_t cap) {
  if (!s || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  const size_t n = std::min<size_t>(cap, s->scene.instances.size());
  std::memcpy(out, s->scene.instances.data(), n * sizeof(DustVoxInstance));
  return DUST_OK;
}
DustStatus dust_vox_flatten_model(const uint8_t* xyzi, size_t n_voxels, const uint32_t size[3], const uint8_t* palette,
                                  DustHipBlock** blocks, uint32_t* n_blocks, uint8_t** materials,
                                  uint64_t* n_materials) {
  if ((!xyzi && n_voxels) || !size || !palette || !blocks || !n_blocks || !materials || !n_materials)
    return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (size[0] > 256 || size[1] > 256 || size[2] > 256) return fail(DUST_ERR_INVALID_ARGUMENT, "model larger than 256^3");
  for (size_t i = 0; i < n_voxels; ++i)
    if (xyzi[i * 4] >= size[0] || xyzi[i * 4 + 1] >= size[1] || xyzi[i * 4 + 2] >= size[2])
      return fail(DUST_ERR_INVALID_ARGUMENT, "voxel outside model size");
  return guarded([&] {
    std::vector<DustHipBlock> b;
    std::vector<uint8_t> m;
    dust::vox::flatten_model(xyzi, n_voxels, size, palette, b, m);
    *blocks = static_cast<DustHipBlock*>(std::malloc(std::max<size_t>(1, b.size()) * sizeof(DustHipBlock)));
    *materials = static_cast<uint8_t*>(std::malloc(std::max<size_t>(1, m.size())));
    if (!*blocks || !*materials) return fail(DUST_ERR_OUT_OF_MEMORY, "host allocation failed");
    std::memcpy(*blocks, b.data(), b.size() * sizeof(DustHipBlock));
    std::memcpy(*materials, m.data(), m.size());
    *n_blocks = uint32_t(b.size());
    *n_materials = m.size();
    return DUST_OK;
  });
}
void dust_vox_free(void* p) { std::free(p); }

// ===================================================================== sky
DustStatus dust_sky_dataset_create(const uint8_t* dataset, size_t n_dataset, const uint8_t* solar, size_t n_solar, DustSkyDataset** out) {
  if (!dataset || !solar || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    std::unique_ptr<DustSkyDataset> d(new DustSkyDataset);
    if (!dust::sky::load_dataset(dataset, n_dataset, solar, n_solar, d->data))
      return fail(DUST_ERR_INVALID_ARGUMENT, "sky tables must be 14400 bytes (dataset.bin) and 21672 bytes (datasetSolar.bin)");
    *out = d.release();
    return DUST_OK;
  });
}
void dust_sky_dataset_destroy(DustSkyDataset* d) { delete d; }
DustStatus dust_sky_bake(const DustSkyDataset* d, float turbidity, const float albedo[3], const float direction[3], DustHipSky* out) {
  if (!d || !albedo || !direction || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (!dust::sky::bake(d->data, turbidity, albedo, direction, out->state))
    return fail(DUST_ERR_INVALID_ARGUMENT, "turbidity must lie in [1, 10] and the sun above the horizon (0 < direction.y <= 1)");
  return DUST_OK;
}

// ===================================================================== device side
DustStatus dust_hip_context_create(const DustHipConfig* cfg, DustHipContext** out) {
  if (!out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (cfg) STRUCT_TRY(cfg, "DustHipConfig");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(DUST_ERR_NO_DEVICE, "no HIP device visible: the MI355X path has no CPU fallback");
  std::unique_ptr<DustHipContext> c(new DustHipContext);
  int dev = cfg ? cfg->device : -1;
  if (dev < 0) HIP_TRY(hipGetDevice(&dev));
  if (dev >= n) return fail(DUST_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  HIP_TRY(hipSetDevice(dev));
  c->device = dev;
  if (cfg && cfg->stream) c->stream = static_cast<hipStream_t>(cfg->stream);
  else { HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
  if (cfg && cfg->lds_root_bytes) c->lds_root_bytes = cfg->lds_root_bytes;
  c->timing = cfg && (cfg->flags & DUST_HIP_CONTEXT_TIMING);
  c->timing_stride = (cfg && (cfg->flags & DUST_HIP_CONTEXT_TIMING_SPARSE)) ? 4u : 1u;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->max_lds = (prop.sharedMemPerBlock ? prop.sharedMemPerBlock : 64 * 1024) - 256;  // dynamic LDS a launch may ask for: the kernels hold 128 bytes of static LDS (earned priorities)
  if (const char* env = diag_env("LDS_ROOT_BYTES")) c->lds_root_bytes = uint32_t(std::strtoul(env, nullptr, 10));  // (diagnostic: DustHipConfig::lds_root_bytes is the knob)
  // what a 512-thread workgroup needs besides the staged roots: 8 candidate lists, the tile queue, and the static
  // buckets of the profiling / debug builds (kernels.hip lds_bytes(), configure_kernels())
  const size_t reserve = size_t(8) * (dust::kMaxCand * 8 + 8) + 16 + 4096;
  const size_t cap = c->max_lds > reserve ? c->max_lds - reserve : 0;
  if (c->lds_root_bytes > cap) c->lds_root_bytes = uint32_t(cap);
  HIP_TRY(dust::configure_kernels(c->max_lds));
  HIP_TRY(dust::configure_query_kernels(c->max_lds));
  {  // (a context without the word works as before: commits that find the host a ring ahead wait for the whole stream)
    void* w = nullptr;
    if (!diag_env("NO_START_WORD") && hipHostMalloc(&w, 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess && w) {
      std::memset(w, 0, 64);
      c->started = static_cast<volatile uint32_t*>(w);
    } else (void)hipGetLastError();
  }
  *out = c.release();
  return DUST_OK;
}
void dust_hip_context_destroy(DustHipContext* c) { release(c); }  // (models, scenes and pipelines made from it keep it alive)
DustStatus dust_hip_sync(DustHipContext* c) {
  if (!c) return fail(DUST_ERR_INVALID_ARGUMENT, "null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_stream(c));
  return DUST_OK;
}

static void destroy_pipeline(DustHipPipeline* p) {
  if (!p) return;
  DustHipContext* c = p->ctx;
  (void)hipSetDevice(c->device);
  (void)sync_stream(c);  // both streams: the surfel pass writes the GI buffers on the second one
  for (auto& kind : p->ev_ring)
    for (auto& side : kind)
      for (auto& e : side) if (e) (void)hipEventDestroy(e);
  if (p->host_stats) (void)hipHostFree(p->host_stats);
  for (hipEvent_t e : {p->side_cal.p0, p->side_cal.p1, p->side_cal.q0, p->side_cal.q1}) if (e) (void)hipEventDestroy(e);
  delete p;
  release(c);
}
DustStatus dust_hip_pipeline_create(DustHipContext* ctx, uint32_t width, uint32_t height, DustHipPipeline** out) {
  if (!ctx || !out || width == 0 || height == 0 || width > 16384 || height > 16384)
    return fail(DUST_ERR_INVALID_ARGUMENT, "bad pipeline size");
  return guarded([&]() -> DustStatus {
    HIP_TRY(hipSetDevice(ctx->device));
    struct Drop { DustHipPipeline* p; ~Drop() { destroy_pipeline(p); } } owner{new DustHipPipeline};
    DustHipPipeline* p = owner.p;
    p->ctx = retain(ctx);
    p->tune = Tuning::from_environment();
    p->width = width; p->height = height;
    const hipStream_t st = ctx->stream;  // (every fill below is ordered on the stream the frames run on)
    const size_t px = size_t(width) * height;
    for (int i = 0; i < DUST_PLANE_COUNT; ++i) {
      HIP_TRY(p->planes[i].alloc(px * kPlaneBytesPerPixel[i]));
      HIP_TRY(hipMemsetAsync(p->planes[i].p, 0, px * kPlaneBytesPerPixel[i], st));
    }
    HIP_TRY(p->counters.alloc(8 * dust::kRegions * dust::kCounterStride * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(p->counters.p, 0, 8 * dust::kRegions * dust::kCounterStride * sizeof(uint32_t), st));
    HIP_TRY(p->stats.alloc(8 * sizeof(dust::DevStats)));
    HIP_TRY(hipMemsetAsync(p->stats.p, 0, 8 * sizeof(dust::DevStats), st));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p->host_stats), 8 * sizeof(dust::DevStats), hipHostMallocDefault));
    std::memset(p->host_stats, 0, 8 * sizeof(dust::DevStats));
    HIP_TRY(p->exposure.alloc(257 * 4));
    HIP_TRY(hipMemsetAsync(p->exposure.p, 0, 257 * 4, st));  // auto_exposure.rs:117: fill_buffer(0)
    // timing only (nothing waits on them for visibility): without the system-scope fence a record does not flush L2 between passes
    if (ctx->timing)
      for (auto& kind : p->ev_ring)
        for (auto& side : kind) {
          side.assign(DustHipPipeline::kEvRing, nullptr);
          for (auto& e : side) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
        }
    HIP_TRY(hipStreamSynchronize(st));
    owner.p = nullptr;
    *out = p;
    return DUST_OK;
  });
}
void dust_hip_pipeline_destroy(DustHipPipeline* p) { destroy_pipeline(p); }
DustStatus dust_hip_pipeline_set_noise(DustHipPipeline* p, uint32_t texture, const uint8_t* texels, uint32_t layers) {
  if (!p || !texels || layers == 0 || (texture != 0 && texture != 5))
    return fail(DUST_ERR_INVALID_ARGUMENT, "noise texture must be 0 (scalar R8) or 5 (unitvec3_cosine RGBA8)");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(sync_stream(p->ctx));  // (frames that read the old texture are done before it is replaced)
  const size_t bytes = size_t(128) * 128 * layers * (texture == 0 ? 1 : 4);
  if (texture == 0) { HIP_TRY(p->noise0.upload(texels, bytes, p->ctx->stream)); p->noise0_layers = layers; }
  else { HIP_TRY(p->noise5.upload(texels, bytes, p->ctx->stream)); p->noise5_layers = layers; }
  return DUST_OK;
}

extern "C" DustStatus dust_hip_pipeline_configure_gi(DustHipPipeline* p, uint32_t hash_capacity, uint32_t surfel_pool_size);
#define DUST_TRY(expr) do { const DustStatus s_ = (expr); if (s_ != DUST_OK) return s_; } while (0)

// ---- what a pipeline contributes to a launch descriptor, wherever one is filled (frames, the GI exchange, a sharded surfel pass's second half)
static void frame_size_args(const DustHipPipeline* p, dust::FrameArgs& a) {
  a.width = p->width; a.height = p->height;
  a.inv_width = 1.0f / float(p->width); a.inv_height = 1.0f / float(p->height); a.aspect = float(p->width) / float(p->height);
}
static void gi_args(const DustHipPipeline* p, dust::DevGI& gi) {
  gi.hash = static_cast<uint32_t*>(p->gi_hash.p);
  gi.hash_capacity = p->gi_capacity;
  gi.pool = static_cast<dust::DevSurfel*>(p->gi_pool.p);
  gi.pool_size = p->gi_pool_size;
  gi.slot_owner = static_cast<uint32_t*>(p->gi_owner.p);
  gi.pixel_surfel = static_cast<dust::DevSurfel*>(p->gi_pixel_surfel.p);
  gi.requests = static_cast<dust::DevHashRequest*>(p->gi_requests.p);
  gi.replacement = static_cast<dust::DevSurfel*>(p->gi_replacement.p);
  gi.sun_payload = static_cast<float*>(p->gi_sun_payload.p);
}
// the radix sort's ping-pong pairs; the first pair is where a kernel leaves the keys and values to sort
static void sort_args(const DustHipPipeline* p, dust::FrameArgs& b, uint32_t* sk[2], uint32_t* sv[2]) {
  for (int k = 0; k < 2; ++k) { sk[k] = static_cast<uint32_t*>(p->gi_sort_keys[k].p); sv[k] = static_cast<uint32_t*>(p->gi_sort_vals[k].p); }
  b.gi.sort_keys = sk[0];
  b.gi.sort_vals = sv[0];
}
static void exchange_view(const DustHipPipeline* p, uint32_t padded_rows, DustHipGiExchange* out) {
  out->pool_size = p->gi_pool_size;
  out->width = p->width;
  out->touched_rows = padded_rows;
  out->slot_owner = p->gi_owner.p;
  out->touched = p->gi_touched.p;
  out->merged = p->gi_merged.p;
}
// the event pair around the launches of pass kind `kind`, in a timed frame
static hipError_t ev_open(DustHipPipeline* p, int kind, hipStream_t st) { return p->timed_frame ? hipEventRecord(p->ev_begin(kind), st) : hipSuccess; }
static hipError_t ev_close(DustHipPipeline* p, int kind, hipStream_t st) {
  if (!p->timed_frame) return hipSuccess;
  const hipError_t e = hipEventRecord(p->ev_end(kind), st);
  if (e == hipSuccess) p->ev_valid[kind] = true;
  return e;
}

// Cost-ordered hand-out for the launch about to be made: the decisions are dust::tile_step's (frame_plan.hpp), carried out here on the pass
// kind's buffers. The history advances as far as the calls get: a failed one leaves the fields behind it as they were.
static DustStatus order_tiles(DustHipPipeline* p, uint32_t kind, dust::FrameArgs& a, hipStream_t st) {
  a.tile_order = nullptr; a.tile_cost = nullptr; a.band_cuts = nullptr;
  DustHipPipeline::TileHistory& h = p->tile_history[kind];
  const Tuning& t = p->tune;
  dust::TileState next = h;
  const dust::TileStep d = dust::tile_step(next, a.tiles_x, a.tiles_y, p->view_key,
                                           {t.no_tile_order, t.equal_bands, t.dilate, t.force_moving, t.cuts_reuse, t.moving_refresh, t.still_refresh_max});
  auto words = [](const DeviceBuffer& b) { return static_cast<uint32_t*>(b.p); };
  if (d.allocate) {
    HIP_TRY(hipStreamSynchronize(st));
    for (DeviceBuffer* b : {&h.cost, &h.order, &h.smooth, &h.spread}) HIP_TRY(b->alloc(size_t(d.total) * 4));
    if (!h.cuts.p) HIP_TRY(h.cuts.alloc(size_t(dust::kRegions + 1) * 4));
    h.capacity = d.total; h.tiles_x = h.tiles_y = 0;
  }
  if (d.reset) {
    h.recorded = false; h.ordered = false; h.measured = false; h.tiles_x = a.tiles_x; h.tiles_y = a.tiles_y;
    HIP_TRY(hipMemsetAsync(h.cost.p, 0, size_t(d.total) * 4, st));
    HIP_TRY(hipMemsetAsync(h.smooth.p, 0, size_t(d.total) * 4, st));
  }
  if (d.blend) {
    HIP_TRY(dust::launch_cost_blend(words(h.cost), words(h.smooth), d.total, t.cost_keep_shift, st));
    if (d.dilate) HIP_TRY(dust::launch_cost_dilate(words(h.smooth), words(h.spread), a.tiles_x, a.tiles_y, st));
    HIP_TRY(dust::launch_tile_order(words(d.dilate ? h.spread : h.smooth), words(h.order), t.equal_bands ? nullptr : words(h.cuts), d.reuse_cuts, d.total, d.per_band, st));
  }
  static_cast<dust::TileState&>(h) = next;
  if (d.hand_order) a.tile_order = words(h.order);
  if (d.hand_cuts) a.band_cuts = words(h.cuts);
  if (d.measure) a.tile_cost = words(h.cost);
  return DUST_OK;
}
// Work counters without a memset per launch: every pass kind owns two sets; a launch pulls tiles from one and its
// first workgroup zeroes the other, which is the set the next launch of that kind (stream-ordered behind it) will use.
static void take_counters(DustHipPipeline* p, uint32_t kind, dust::FrameArgs& a) {
  uint32_t* base = static_cast<uint32_t*>(p->counters.p) + size_t(kind) * 2 * dust::kRegions * dust::kCounterStride;
  const uint32_t par = p->counter_parity[kind];
  a.work_counters = base + size_t(par) * dust::kRegions * dust::kCounterStride;
  a.next_work_counters = base + size_t(par ^ 1u) * dust::kRegions * dust::kCounterStride;
  p->counter_parity[kind] = par ^ 1u;
}

// The ray stream of pass kind `kind` (0: final gather, 1: surfel pass) for the launch about to be made: its buffers, this launch's
// ray counter (zero: the previous launch of the kind zeroed it) and the one the next launch will use.
static void stream_args(DustHipPipeline* p, int kind, dust::FrameArgs& a, float tmin, float tmax) {
  a.stream.unbinned = static_cast<uint32_t*>(p->gi_unbinned.p) + kind * 2;
  a.stream.rays = static_cast<dust::DevRay*>(kind == 0 ? p->gi_rays_fg.p : p->gi_rays_sf.p);
  a.stream.group_count = static_cast<uint32_t*>(kind == 0 ? p->gi_groups_fg.p : p->gi_groups_sf.p);
  if (kind == 0) {  // a group = a 16 x 16 pixel tile of the band (k_gather_rays)
    a.stream.n_groups = ((p->width + 15u) / 16u) * ((a.row_end - a.row_begin + 15u) / 16u);
    a.stream.group_rays = 256;
  } else {          // a group = 256 consecutive surfels of the (ordered) pool, two rays each (k_surfel_rays)
    a.stream.n_groups = (p->gi_pool_size + 255u) / 256u;
    a.stream.group_rays = 512;
  }
  a.stream.ray_hits = static_cast<dust::DevGatherHit*>(kind == 0 ? p->gi_fg_hits.p : p->gi_hits_sf.p);
  a.stream.ray_tmin = tmin; a.stream.ray_tmax = tmax;
  a.tile_order = nullptr; a.tile_cost = nullptr; a.band_cuts = nullptr;  // (the stream hands out rays, not tiles)
  a.tiles_x = a.tiles_y = 1;
}
// The ray streams' buffers (gi.hip), made when a frame first takes a stream path -- the packet kernels, the default everywhere but the
// final gather of a scene with a 4096^3 tree, never read them (130 MB at 1080p, 530 MB at 4K): a ray per pixel / two per surfel at most,
// the hit records, the group counters. Waits for the streams once (an allocation is not stream-ordered).
static DustStatus ensure_stream_buffers(DustHipPipeline* p, bool gather, bool surfel) {
  const bool need_fg = gather && !p->gi_rays_fg.p, need_sf = surfel && !p->gi_rays_sf.p;
  if (!need_fg && !need_sf && p->gi_unbinned.p) return DUST_OK;
  HIP_TRY(sync_stream(p->ctx));
  if (!p->gi_unbinned.p) {
    HIP_TRY(p->gi_unbinned.alloc(4 * 4));
    HIP_TRY(hipMemsetAsync(p->gi_unbinned.p, 0, 4 * 4, p->ctx->stream));
  }
  if (need_fg) {
    const size_t tiles = size_t((p->width + 15) / 16) * ((p->height + 15) / 16);
    HIP_TRY(p->gi_rays_fg.alloc(tiles * 256 * sizeof(dust::DevRay)));
    HIP_TRY(p->gi_groups_fg.alloc(tiles * 4));
    HIP_TRY(p->gi_fg_hits.alloc(size_t(p->width) * p->height * sizeof(dust::DevGatherHit)));
  }
  if (need_sf) {
    const size_t runs = (size_t(p->gi_pool_size) + 255) / 256;
    HIP_TRY(p->gi_rays_sf.alloc(runs * 512 * sizeof(dust::DevRay)));
    HIP_TRY(p->gi_groups_sf.alloc(runs * 4));
    HIP_TRY(p->gi_hits_sf.alloc(size_t(p->gi_pool_size) * 2 * sizeof(dust::DevGatherHit)));
  }
  return DUST_OK;
}
// the recorded hash inserts, applied in surfel-index order (DUST_PASS_GI_ORDERED): in parallel over independent probe-window clusters (the serial
// one-wavefront loop it is checked against stays reachable through DUST_HIP_DEBUG bit 16)
static DustStatus apply_ordered(DustHipPipeline* p, dust::FrameArgs& b, hipStream_t st) {
  uint32_t *sk[2], *sv[2];
  // keys -> sort by hash location -> marks (which requests the frame applies: k_surfel_apply_mark) -> the apply, parallel over clusters
  // or (DUST_HIP_DEBUG bit 16) the serial loop in surfel order it is checked against
  sort_args(p, b, sk, sv);
  b.apply_alive = static_cast<unsigned long long*>(p->gi_apply_alive.p);
  b.apply_dead = static_cast<uint8_t*>(p->gi_apply_dead.p);
  b.apply_words = (p->gi_pool_size + 63u) / 64u;
  b.apply_starts = b.apply_alive + b.apply_words + 1;
  HIP_TRY(dust::launch_surfel_apply(b, 2, st));
  bool in_b = false;
  HIP_TRY(dust::radix_sort_pairs(p->gi_sort_scratch.p, sk[0], sv[0], sk[1], sv[1], p->gi_pool_size, dust::apply_key_bits(p->gi_capacity), &in_b, st));
  b.gi.apply_keys = sk[in_b ? 1 : 0];
  b.gi.apply_vals = sv[in_b ? 1 : 0];
  HIP_TRY(dust::launch_surfel_apply(b, 4, st));
  HIP_TRY(dust::launch_surfel_apply(b, (p->tune.debug & 16u) ? 1 : 3, st));
  return DUST_OK;
}
// The surfel pass of one frame (surfel.rgen + the spatial hash update) on stream `st`, on at most `resident` workgroup slots.
// shard_world >= 1: the trace of rank shard_rank's share of the ordered pool only, records staged in slot order, nothing applied
// (dust_hip_gi_surfel_exchange_run completes the pass)
static DustStatus run_surfel_pass(DustHipPipeline* p, const dust::FrameArgs& a, uint32_t passes, bool count, hipStream_t st, uint32_t resident,
                                  bool as_stream, uint32_t shard_rank = 0, uint32_t shard_world = 0) {
  const Tuning& tune = p->tune;
  dust::FrameArgs b = a;  // 64 consecutive surfels x one ray kind per wavefront: one row of "tiles", cosine items then sun items
  // on the second stream the pass is the longer of the two sides that share the SIMDs: its waves win the issue arbitration
  if (st != p->ctx->stream) b.prio_floor = tune.side_prio;
  b.tiles_x = 2 * ((p->gi_pool_size + 63) / 64);
  b.tiles_y = 1;
  b.stats = static_cast<dust::DevStats*>(p->stats.p) + 4;
  uint32_t *sk[2], *sv[2];
  sort_args(p, b, sk, sv);
  HIP_TRY(ev_open(p, 3, st));
  if (!tune.no_surfel_sort) {  // phase 0: 16-bit space-filling-curve keys + radix sort -> gi.perm
    HIP_TRY(dust::launch_surfel_keys(b, st));
    bool in_b = false;
    HIP_TRY(dust::radix_sort_pairs(p->gi_sort_scratch.p, sk[0], sv[0], sk[1], sv[1], p->gi_pool_size, 16, &in_b, st));
    b.gi.perm = sv[in_b ? 1 : 0];
  }
  const bool staged = shard_world >= 1;
  if (staged) {
    const dust::ShardRange r = dust::shard_range(p->gi_pool_size, shard_rank, shard_world);
    if (p->gi_stage_slots < r.cap) {   // (made for the pool size of the frame that needs them: the slots of every rank's share index all three)
      HIP_TRY(hipStreamSynchronize(st));
      p->gi_stage_slots = 0;
      HIP_TRY(p->gi_stage_req.alloc(r.cap * sizeof(dust::DevHashRequest)));
      HIP_TRY(p->gi_stage_repl.alloc(r.cap * 16));
      HIP_TRY(p->gi_stage_sun.alloc(r.cap * 16));
      HIP_TRY(hipMemsetAsync(p->gi_stage_req.p, 0, r.cap * sizeof(dust::DevHashRequest), st));
      HIP_TRY(hipMemsetAsync(p->gi_stage_repl.p, 0xFF, r.cap * 16, st));   // direction 0xFFFFFFFF: "keep"
      HIP_TRY(hipMemsetAsync(p->gi_stage_sun.p, 0, r.cap * 16, st));
      p->gi_stage_slots = r.cap;
    }
    b.sf_stage_req = static_cast<dust::DevHashRequest*>(p->gi_stage_req.p);
    b.sf_stage_repl = static_cast<dust::DevSurfel*>(p->gi_stage_repl.p);
    b.sf_stage_sun = static_cast<float*>(p->gi_stage_sun.p);
    b.sf_group_begin = r.group_begin;
    b.sf_group_count = r.group_count;
    b.tiles_x = 2 * b.sf_group_count;   // (a rank past the end of the pool traces nothing)
    p->sf_shard.pending = true; p->sf_shard.perm = b.gi.perm; p->sf_shard.rank = shard_rank; p->sf_shard.world = shard_world;
    p->sf_shard.slots_per_rank = r.slots_per_rank;
  }
  if (!as_stream || staged) {   // (a sharded trace runs as packets: the stream's shading kernel writes by surfel index)
    if (b.tiles_x) {   // (a rank past the end of the pool traces nothing)
      take_counters(p, 3, b);
      DUST_TRY(order_tiles(p, 3, b, st));
      HIP_TRY(dust::launch_surfel_trace(b, dust::packet_grid(resident, b.tiles_x), tune.block, count, st));
    }
  } else {
    // phase 1 as a ray stream (gi.hip): the pool's rays, compacted -> one ray per lane, lanes refilled -> the hash lookups over the hit records
    stream_args(p, 1, b, 0.1f, 10000.0f);  // surfel.rgen:33-62
    take_counters(p, 3, b);
    b.stream.count_unbinned = count ? 1u : 0u;
    if (count) HIP_TRY(hipMemsetAsync(b.stream.unbinned, 0, 2 * 4, st));
    HIP_TRY(dust::launch_surfel_rays(b, st));
    const uint32_t want = (p->gi_pool_size * 2u + 1023u) / 1024u;
    HIP_TRY(dust::launch_ray_walk(b, 3, dust::ray_walk_grid(resident, tune.block, want), 1024, count, st));
    HIP_TRY(dust::launch_surfel_shade(b, st));
  }
  // phase 2: apply the recorded inserts. Default: concurrently, like the reference's shaders. DUST_PASS_GI_ORDERED: the
  // result of applying them in surfel-index order (apply_ordered). A sharded trace stops here: its records are not complete yet.
  if (!staged && !(passes & DUST_PASS_GI_ORDERED)) HIP_TRY(dust::launch_surfel_apply(b, 0, st));
  else if (!staged) DUST_TRY(apply_ordered(p, b, st));
  HIP_TRY(ev_close(p, 3, st));
  return DUST_OK;
}
// Several frames in one persistent launch (dust_hip_render_frames): the frames are PREPARED in order -- the scene as each of them sees it, its
// descriptor, work counters, tile order -- and left in `frames[]`; the preparation of the last one launches k_primary_ao_batch over all of them.
struct BatchJoin {
  dust::FrameArgs frames[dust::kMaxBatch];
  uint32_t image_of[dust::kMaxBatch] = {};   // which of the scene's ring of device images each frame reads (the scene may be committed between two frames of a launch)
  // View runs (dust_dev.h, FrameArgs::view_run): frame i CONTINUES frame i - 1's run when camera and sky are byte-identical and both read the same scene
  // image. Decided while frame i is prepared -- a follower of a run takes no tile order and measures nothing: the launch reads its leader's --, turned
  // into run lengths by the Lead.
  const DustHipCamera* cams[dust::kMaxBatch] = {};
  const DustHipSky* skies[dust::kMaxBatch] = {};
  bool continues[dust::kMaxBatch] = {};
  bool took_counters[dust::kMaxBatch] = {};  // the frame's pipeline has flipped its counter parity for this launch (dust_hip_render_frames gives it back if the launch is never made)
  bool launched = false;                     // the launch was enqueued: the counter sets are in use as taken
  DustHipPipeline* timer = nullptr;          // frame 0's pipeline: its HIP-event pair brackets the launch
  uint32_t n = 0;      // frames of the launch
  uint32_t slot = 0;   // the frame being prepared
};
// Follower: frames 0 .. n - 2 of a launch, prepared in order; Lead: frame n - 1 -- prepared last, launches all of them
enum class FrameRole { Single, Follower, Lead };
// every argument check of a frame, before anything is enqueued or changed (a frame that has started is finished); fp_copy: the caller's
// parameters widened to this library's struct
static DustStatus check_frame(DustHipPipeline* p, const DustHipScene* s, const DustHipCamera* cam, const DustHipSky* sky,
                              const DustHipFrameParams* fp_in, DustHipFrameParams& fp_copy) {
  if (!p || !s || !cam || !sky || !fp_in) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  // (round 6 appended surfel_rank / surfel_world: a caller compiled against the struct that ends at row_end gets zeroes for them)
  if (fp_in->struct_size < offsetof(DustHipFrameParams, surfel_rank)) return fail(DUST_ERR_INVALID_ARGUMENT, "DustHipFrameParams.struct_size is smaller than this library's DustHipFrameParams");
  fp_copy = DustHipFrameParams{};
  std::memcpy(&fp_copy, fp_in, std::min<size_t>(fp_in->struct_size, sizeof fp_copy));
  const DustHipFrameParams* fp = &fp_copy;
  if (p->ctx != s->ctx) return fail(DUST_ERR_INVALID_ARGUMENT, "pipeline and scene belong to different contexts");
  DUST_TRY(check_scene_ready(s));
  const uint32_t need5 = DUST_PASS_AMBIENT_OCCLUSION | DUST_PASS_FINAL_GATHER | DUST_PASS_SURFEL;
  if ((fp->passes & need5) && !p->noise5.p)
    return fail(DUST_ERR_NOT_READY, "blue-noise texture 5 (unitvec3_cosine) not loaded");  // standard.rs:254
  if ((fp->passes & (DUST_PASS_FINAL_GATHER | DUST_PASS_SURFEL)) && !p->noise0.p)
    return fail(DUST_ERR_NOT_READY, "blue-noise texture 0 (scalar) not loaded");
  const bool sharded = (fp->passes & DUST_PASS_GI_SHARDED) != 0;
  // (argument checks all come before the first launch: a frame that has started is finished)
  if ((fp->passes & DUST_PASS_ACCUMULATE) && (fp->passes & DUST_PASS_DENOISE))
    return fail(DUST_ERR_INVALID_ARGUMENT, "DUST_PASS_ACCUMULATE and DUST_PASS_DENOISE both keep their running result in DUST_PLANE_ACCUM: one per frame");
  if ((fp->passes & DUST_PASS_DENOISE) && (fp->row_begin != 0 || (fp->row_end != 0 && fp->row_end != p->height)))
    return fail(DUST_ERR_UNSUPPORTED, "DUST_PASS_DENOISE reprojects and blurs across rows: run it on the whole (gathered) frame");
  if (!sharded && (fp->passes & (DUST_PASS_FINAL_GATHER | DUST_PASS_SURFEL)) && (fp->row_begin != 0 || (fp->row_end != 0 && fp->row_end != p->height)))
    return fail(DUST_ERR_UNSUPPORTED, "a GI pass on a row band needs DUST_PASS_GI_SHARDED and the exchange of dust_hip_pipeline_gi_exchange");
  if (sharded && (fp->passes & DUST_PASS_FINAL_GATHER) && (fp->passes & DUST_PASS_SURFEL))
    return fail(DUST_ERR_INVALID_ARGUMENT, "DUST_PASS_GI_SHARDED: the surfel pass runs after the exchange, in its own call");
  if (fp->surfel_world != 0 && (fp->passes & DUST_PASS_SURFEL) &&
      (!sharded || !(fp->passes & DUST_PASS_GI_ORDERED) || fp->surfel_world > 64 || fp->surfel_rank >= fp->surfel_world))
    return fail(DUST_ERR_INVALID_ARGUMENT, "a sharded surfel trace wants DUST_PASS_GI_SHARDED, DUST_PASS_GI_ORDERED, surfel_world <= 64 and surfel_rank < surfel_world");
  if (p->sf_shard.pending && (fp->passes & (DUST_PASS_FINAL_GATHER | DUST_PASS_SURFEL)))
    return fail(DUST_ERR_NOT_READY, "a sharded surfel trace is pending on this pipeline: dust_hip_gi_surfel_exchange_run completes it before the next GI pass");
  if (sharded && (fp->passes & DUST_PASS_FINAL_GATHER) && !p->gi_touched.p)
    return fail(DUST_ERR_NOT_READY, "DUST_PASS_GI_SHARDED: call dust_hip_pipeline_gi_exchange first");
  {
    const uint32_t re = fp->row_end ? fp->row_end : p->height;
    if (fp->row_begin >= re || re > p->height) return fail(DUST_ERR_INVALID_ARGUMENT, "bad row range");
  }
  return DUST_OK;
}

// ---- one frame. What its passes share: the handles, the frame's flags and its plan (frame_plan.hpp). The descriptor `a` goes from pass to pass
// as each one left it (statistics slot, work counters, tile order, start sequence number): a later pass's copy holds exactly what it always held.
struct Frame {
  DustHipPipeline* p; DustHipContext* ctx; const DustHipScene* s; const DustHipFrameParams* fp; hipStream_t st;
  bool count = false, sharded = false;
  bool fg_stream = false, sf_stream = false;   // the GI passes that run as ray streams (gather_as_stream, surfel_as_stream)
  bool calibrate = false;                      // the frame runs its surfel pass in place, timed (side_share)
  uint32_t share = 0;                          // the surfel pass's percent of the slots on the second stream
  dust::SlotInputs si; dust::SlotPlan plan;
  // the frame's first traversal launch tells the host that the frame has started (DustHipContext::started; dust_hip_scene_commit)
  bool start_said = false;
  void say_start(dust::FrameArgs& x) {
    if (start_said || !ctx->started) return;
    start_said = true;
    x.started_word = const_cast<uint32_t*>(ctx->started);
    x.started_seq = ++ctx->frame_seq;
    s->slots[s->current].last_seq = x.started_seq;
  }
};
// the frame's descriptor: what the scene, the pipeline, the camera and the sky contribute (a pass adds its own: counters, tile order, stream)
static void frame_args(const DustHipPipeline* p, const DustHipScene* s, const DustHipCamera* cam, const DustHipSky* sky, const DustHipFrameParams* fp,
                       dust::FrameArgs& a) {
  const Tuning& tune = p->tune;
  scene_args(s, a);
  for (int k = 0; k < 3; ++k) { a.world_min[k] = s->world_min[k]; a.world_max[k] = s->world_max[k]; }
  for (const DustHipModel* m : s->models) a.deep |= m->dev.n_levels == 3 ? 1u : 0u;
  a.stream_refill = tune.stream_refill; a.stream_top_iters = tune.stream_top_iters;
  a.sl_bin = dust::stream_lds(dust::kStreamBinBudget, true, a.grid.dim, a.grid.n_items, a.n_instances, tune.no_stream_lds);
  a.sl_walk = dust::stream_lds(dust::stream_walk_budget(p->ctx->max_lds, a.n_lds_models), false, a.grid.dim, a.grid.n_items, a.n_instances, tune.no_stream_lds);
  std::memcpy(a.cam.col0, cam->view_col0, 12); std::memcpy(a.cam.col1, cam->view_col1, 12);
  std::memcpy(a.cam.col2, cam->view_col2, 12); std::memcpy(a.cam.pos, cam->position, 12);
  a.cam.tan_half_fov = cam->tan_half_fov; a.cam.far_ = cam->far_; a.cam.near_ = cam->near_;
  std::memcpy(a.sky, sky->state, sizeof(a.sky));
  sun_constants(a.sky, a.sun_dir, a.sun_term);
  a.g.illuminance = static_cast<uint16_t*>(p->plane(DUST_PLANE_ILLUMINANCE));
  a.g.denoised = static_cast<uint16_t*>(p->plane(DUST_PLANE_DENOISED));
  a.g.albedo = static_cast<uint32_t*>(p->plane(DUST_PLANE_ALBEDO));
  a.g.normal = static_cast<uint32_t*>(p->plane(DUST_PLANE_NORMAL));
  a.g.depth = static_cast<float*>(p->plane(DUST_PLANE_DEPTH));
  a.g.motion = static_cast<uint16_t*>(p->plane(DUST_PLANE_MOTION));
  a.g.voxel_id = static_cast<uint32_t*>(p->plane(DUST_PLANE_VOXEL_ID));
  a.g.accum = static_cast<float*>(p->plane(DUST_PLANE_ACCUM));
  frame_size_args(p, a);
  a.row_begin = fp->row_begin;
  a.row_end = fp->row_end ? fp->row_end : p->height;   // (check_frame has seen the range)
  a.tiles_x = (p->width + dust::kTileW - 1) / dust::kTileW;
  a.tiles_y = (a.row_end - a.row_begin + dust::kTileH - 1) / dust::kTileH;
  a.rand = fp->rand; a.frame_index = fp->frame_index;
  if (p->noise0.p) a.noise0 = static_cast<const uint8_t*>(p->noise0.p) + size_t(fp->frame_index % p->noise0_layers) * 128 * 128;
  if (p->noise5.p) a.noise5 = static_cast<const uint8_t*>(p->noise5.p) + size_t(fp->frame_index % p->noise5_layers) * 128 * 128 * 4;  // noise.rs:50
  a.stats = static_cast<dust::DevStats*>(p->stats.p);
  a.accum_count = p->accum_count;
  a.debug = tune.debug;
  a.static_rounds_request = tune.static_rounds;
  gi_args(p, a.gi);
}
static dust::SlotInputs slot_inputs(const DustHipPipeline* p, const dust::FrameArgs& a) {   // (the share is the caller's to add)
  const Tuning& t = p->tune;
  dust::SlotInputs in;
  in.num_cus = uint32_t(p->ctx->num_cus); in.max_lds = p->ctx->max_lds;
  in.block = t.block; in.blocks_per_cu = t.blocks_per_cu;
  in.n_lds_models = a.n_lds_models; in.n_instances = a.n_instances; in.n_groups = a.n_groups;
  in.no_lds_boxes = t.no_lds_boxes;
  in.reserve_request = t.reserve_blocks; in.in_collective = p->in_collective; in.side_busy = p->ctx->side_busy;
  in.frames_in_flight = p->frames_in_flight; in.in_flight_slots = t.in_flight_slots; in.in_flight_oversub = t.in_flight_oversub;
  in.total_tiles = a.tiles_x * a.tiles_y;
  return in;
}
// The surfel pass's share of the slots for this frame, and whether the frame calibrates it: the configured share, or the calibrated one
// once the pipeline has it (DustHipPipeline::side_cal), or the guess from the ray counts.
static DustStatus side_share(Frame& f, const dust::FrameArgs& a) {
  DustHipPipeline* p = f.p;
  const Tuning& tune = p->tune;
  f.share = tune.side_share;
  if (f.share) return DUST_OK;
  auto& cal = p->side_cal;
  if (cal.state == 1 && hipEventQuery(cal.q1) == hipSuccess) {
    float P = 0.0f, Q = 0.0f;
    if (hipEventElapsedTime(&P, cal.p0, cal.p1) == hipSuccess && hipEventElapsedTime(&Q, cal.q0, cal.q1) == hipSuccess && P > 0.0f && Q > 0.0f)
      cal.share = dust::calibrated_share(P, Q, a.deep != 0);
    cal.state = 2;
  }
  (void)hipGetLastError();  // (hipEventQuery's "not ready" is not an error of this call)
  const bool gi_frame = (f.fp->passes & DUST_PASS_PRIMARY) && (f.fp->passes & DUST_PASS_SURFEL);
  // (not the pipeline's first GI frames: they touch the hash and the pool for the first time -- 400 MB of first-touch page faults inside the
  //  timed pass; one deep-tree run in five calibrated a share half as large again from it: 4.66 ms per frame against 4.27-4.30)
  if (gi_frame && cal.state == 0) ++cal.gi_frames;
  f.calibrate = cal.state == 0 && cal.gi_frames >= 3u && gi_frame && !tune.no_side_stream && !f.count && !f.sharded && !(tune.debug & 16u);
  if (f.calibrate) HIP_TRY(join_side(f.ctx));   // (the timed frame runs its passes one after the other, behind the previous frame's surfel pass)
  if (f.calibrate && !cal.p0)
    for (hipEvent_t* e : {&cal.p0, &cal.p1, &cal.q0, &cal.q1}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableSystemFence));
  f.share = cal.share ? cal.share : dust::guessed_share(p->gi_pool_size, p->width, a.row_end - a.row_begin);
  return DUST_OK;
}

// The Lead's launch of all the frames of a BatchJoin, `a.started_seq` and the view runs filled in
static DustStatus launch_batch(Frame& f, BatchJoin* join, const dust::FusedShape& shape) {
  const DustHipScene* s = f.s;
  f.say_start(join->frames[0]);   // (the kernel's first descriptor says it)
  for (uint32_t i = 0; i < join->n; ++i) {
    // Every scene image a frame of the launch reads is in use from NOW until the launch is done. dust_hip_scene_commit recycles an image by
    // `epoch` (has anybody waited for the stream since a frame reading it was enqueued?) and `last_seq`: both were stamped when the frame
    // was PREPARED (touch()), and a commit between then and now may have waited for the stream -- the image would pass for idle
    // (found by tools/stress_host.py frames: 17 to 19 frames per call with moves, the third launch's commits landing on the second's images).
    s->slots[join->image_of[i]].epoch = f.ctx->sync_epoch;
    s->slots[join->image_of[i]].last_seq = join->frames[0].started_seq;
    // the boxes staged in LDS are frame 0's image's: a frame of another image (an instance moved in between) reads its own from memory
    if (join->image_of[i] != join->image_of[0]) join->frames[i].n_lds_boxes = 0;
  }
  uint32_t runs[dust::kMaxBatch];
  dust::view_runs(join->continues, join->n, runs);
  for (uint32_t i = 0; i < join->n; ++i) join->frames[i].view_run = runs[i];
  join->launched = true;
  if ((f.p->tune.debug & 32u) || dust::launch_primary_ao_batch(join->frames, join->n, shape.fgrid, shape.fblock, f.st) != hipSuccess) {   // (DUST_HIP_DEBUG bit 32: as if refused)
    // (the launch carries 8.5 KB of kernel arguments -- probed on this runtime, which takes 16 KB. Should a runtime refuse it: the prepared
    //  frames one launch each, the same results)
    (void)hipGetLastError();
    for (uint32_t i = 0; i < join->n; ++i) HIP_TRY(dust::launch_primary_ao(join->frames[i], shape.fgrid, shape.fblock, false, f.st));
  }
  return DUST_OK;
}
// The fused pixel pass: primary + AO in one launch. Single: this frame's own launch. Follower: the frame is prepared and left in the join.
// Lead: prepared likewise, then all of the join's frames are launched.
static DustStatus fused_pass(Frame& f, dust::FrameArgs& a, const DustHipCamera* cam, const DustHipSky* sky, FrameRole role, BatchJoin* join) {
  DustHipPipeline* p = f.p;
  const Tuning& tune = p->tune;
  take_counters(p, 0, a);
  bool continues = false;
  if (role != FrameRole::Single) {
    const uint32_t i = join->slot;
    join->took_counters[i] = true;
    join->cams[i] = cam; join->skies[i] = sky;
    continues = i > 0 && !tune.no_shared_view && join->image_of[i - 1] == uint32_t(f.s->current) &&
                std::memcmp(cam, join->cams[i - 1], sizeof *cam) == 0 && std::memcmp(sky, join->skies[i - 1], sizeof *sky) == 0;
    join->continues[i] = continues;
  }
  if (continues) {
    // a follower of a view run: the launch hands out the run's tiles by its leader's order and writes the leader's cost buffer. This pipeline's tile
    // history is left as it stands -- nothing of it is read, nothing is measured for it --, valid for its next launch, alone or grouped differently.
    a.tile_order = nullptr; a.tile_cost = nullptr; a.band_cuts = nullptr;
  } else {
    DUST_TRY(order_tiles(p, 0, a, f.st));
  }
  a.stats = static_cast<dust::DevStats*>(p->stats.p);
  if (role != FrameRole::Single) {   // a frame of a launch of several: prepared; the last one launches them all
    join->frames[join->slot] = a;
    join->image_of[join->slot] = f.s->current;
    if (join->slot == 0) join->timer = p;
    if (role == FrameRole::Follower) return DUST_OK;
  }
  DustHipPipeline* tp = role == FrameRole::Lead ? join->timer : p;   // whose event pair brackets the launch
  HIP_TRY(ev_open(tp, 0, f.st));
  const dust::FusedShape shape = dust::fused_shape(f.si, f.plan, tune.wide_fused, tune.wide_share, role == FrameRole::Lead ? join->n : 1u);
  if (shape.too_big) return fail(DUST_ERR_INVALID_ARGUMENT, "staged roots and candidate lists exceed the device's LDS");
  if (role == FrameRole::Lead) {
    DUST_TRY(launch_batch(f, join, shape));
  } else {
    f.say_start(a);
    HIP_TRY(dust::launch_primary_ao(a, shape.fgrid, shape.fblock, f.count, f.st));
  }
  a.started_word = nullptr;
  HIP_TRY(ev_close(tp, 0, f.st));
  if (tp->timed_frame) tp->ev_valid[1] = false;
  return DUST_OK;
}
// The unfused pixel passes (DUST_HIP_NO_FUSE=1 keeps the reference's one-launch-per-pass shape), kind 0: primary, 1: AO
static DustStatus pixel_pass(Frame& f, dust::FrameArgs& a, int kind) {
  DustHipPipeline* p = f.p;
  take_counters(p, kind, a);
  DUST_TRY(order_tiles(p, kind, a, f.st));
  a.stats = static_cast<dust::DevStats*>(p->stats.p) + kind;
  HIP_TRY(ev_open(p, kind, f.st));
  f.say_start(a);
  HIP_TRY(kind == 0 ? dust::launch_primary(a, f.plan.grid, p->tune.block, f.count, f.st) : dust::launch_ambient_occlusion(a, f.plan.grid, p->tune.block, f.count, f.st));
  a.started_word = nullptr;
  HIP_TRY(ev_close(p, kind, f.st));
  return DUST_OK;
}
// The final gather as a ray stream (gi.hip): make and bin the band's gather rays (a thread per pixel) -> walk them one per lane, lanes refilled
// (k_ray_walk) -> shade the hit records (a thread per pixel). Behind the previous frame's surfel pass, like the packet kernel: rays and
// hit records touch no GI state and COULD run beside that pass, but two persistent launches sharing the slots both get slower
// (the 4096^3 tree's GI frame: 5.40 ms beside it, 4.56 behind it).
static DustStatus gather_stream_pass(Frame& f, const dust::FrameArgs& a) {
  DustHipPipeline* p = f.p;
  const hipStream_t st = f.st;
  HIP_TRY(join_side(f.ctx));
  dust::FrameArgs g = a;
  stream_args(p, 0, g, 8.0f, a.cam.far_);  // final_gather.rgen:47-50
  g.gi.fg_hits = g.stream.ray_hits;
  take_counters(p, 2, g);
  g.stream.count_unbinned = f.count ? 1u : 0u;
  if (f.count) HIP_TRY(hipMemsetAsync(g.stream.unbinned, 0, 2 * 4, st));
  HIP_TRY(ev_open(p, 2, st));
  HIP_TRY(dust::launch_gather_rays(g, st));
  const uint32_t want = uint32_t((size_t(p->width) * (a.row_end - a.row_begin) + 1023u) / 1024u);
  HIP_TRY(dust::launch_ray_walk(g, 2, dust::ray_walk_grid(f.plan.resident, p->tune.block, want), 1024, f.count, st));
  dust::FrameArgs sh = a;   // (pixel order over the band)
  sh.gi.fg_hits = g.gi.fg_hits;
  HIP_TRY(dust::launch_final_gather_shade(sh, !f.sharded, st));
  HIP_TRY(ev_close(p, 2, st));
  return DUST_OK;
}
// The final gather as packets of 64 rays (k_final_gather)
// (Round 4 also built the gather as a trace-only kernel beside the previous frame's surfel pass + a shading pass over hit records, and
//  round 3 as refilled ray lanes inside the packet kernel: both measured slower and were removed in round 6 -- docs/EXPERIMENTS.md.)
static DustStatus gather_packet_pass(Frame& f, const dust::FrameArgs& a) {
  DustHipPipeline* p = f.p;
  const hipStream_t st = f.st;
  dust::FrameArgs g = a;
  if (!p->tune.no_gather_order) {  // pre-pass: regroup the band's live pixels by ray-direction octant
    const uint32_t otx = (p->width + 63) / 64, oty = (a.row_end - a.row_begin + 63) / 64;
    g.gi.order = static_cast<uint32_t*>(p->gi_order.p);
    g.gi.order_count = static_cast<uint32_t*>(p->gi_order_count.p);
    g.gi.order_tiles_x = otx;
    HIP_TRY(dust::launch_gather_order(g, otx * oty, st));
    // work items: 64 packets of 64 per tile, the empty ones skipped by the kernel
    g.tiles_x = otx * oty * 64u;
    g.tiles_y = 1;
  }
  HIP_TRY(join_side(f.ctx));  // the previous frame's surfel pass has written the hash and the pool this gather reads
  take_counters(p, 2, g);
  DUST_TRY(order_tiles(p, 2, g, st));
  HIP_TRY(ev_open(p, 2, st));  // (behind the regrouping pre-pass: the gather kernel)
  HIP_TRY(dust::launch_final_gather(g, dust::packet_grid(f.plan.resident, g.tiles_x * g.tiles_y), p->tune.block, f.count, !f.sharded, st));
  HIP_TRY(ev_close(p, 2, st));
  return DUST_OK;
}
// The surfel pass: on the context's second stream, behind this frame's final gather (see DustHipContext::side): the pass is a handful of
// latency-bound launches around a trace that is as long as its longest ray, and nothing of THIS frame waits for it. In place -- on the
// main stream, on all the slots -- in a counting, sharded or calibrating frame.
static DustStatus surfel_pass(Frame& f, const dust::FrameArgs& a) {
  DustHipPipeline* p = f.p;
  DustHipContext* ctx = f.ctx;
  const Tuning& tune = p->tune;
  const bool aside = !tune.no_side_stream && !f.count && !f.sharded && !(tune.debug & 16u) && !f.calibrate;
  if (aside) HIP_TRY(fork_side(ctx));
  else HIP_TRY(join_side(ctx));
  if (f.calibrate) HIP_TRY(hipEventRecord(p->side_cal.q0, f.st));
  DustStatus rs = run_surfel_pass(p, a, f.fp->passes, f.count, aside ? ctx->side : f.st, aside ? dust::side_resident(f.plan.resident, f.share) : f.plan.resident,
                                  f.sf_stream, f.fp->surfel_rank, f.fp->surfel_world);
  // (whatever of the pass was enqueued -- all of it, or what came before a failed launch -- is waited for by the next user of the GI state)
  if (aside) { ctx->side_busy = true; const hipError_t re = hipEventRecord(ctx->ev_side_done, ctx->side); if (rs == DUST_OK && re != hipSuccess) rs = hip_fail(re, "hipEventRecord(ev_side_done)"); }
  if (rs != DUST_OK) return rs;
  if (f.calibrate) { HIP_TRY(hipEventRecord(p->side_cal.q1, f.st)); p->side_cal.state = 1; }
  return DUST_OK;
}
static DustStatus accumulate_pass(Frame& f, const dust::FrameArgs& a) {
  f.p->have_history = false;  // the plane now holds an N-frame mean, not the denoiser's history
  HIP_TRY(dust::launch_accumulate(a, f.st));
  f.p->accum_count += 1;
  return DUST_OK;
}
static DustStatus denoise_pass(Frame& f, const dust::FrameArgs& a) {
  DustHipPipeline* p = f.p;
  const size_t px = size_t(p->width) * p->height;
  if (!p->hist_accum[0].p) {
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(p->hist_accum[k].alloc(px * 16)); HIP_TRY(p->hist_geo[k].alloc(px * 16));
    }
    p->have_history = false;
  }
  dust::DenoiseArgs d{};
  d.illuminance = a.g.illuminance; d.denoised = a.g.denoised; d.normal = a.g.normal; d.depth = a.g.depth;
  d.motion = a.g.motion; d.voxel_id = a.g.voxel_id;
  const uint32_t in = p->hist_parity, out = in ^ 1u;
  // The radiance history lives in DUST_PLANE_ACCUM itself (it is what that plane shows while the denoiser runs): this frame
  // reads the plane's buffer and writes the spare one, and the two then trade places -- no copy. A caller-bound plane cannot
  // trade: it takes part as one side of an ordinary pair and receives a copy.
  const bool trade = p->bound[DUST_PLANE_ACCUM] == nullptr;
  d.hist_in_accum = static_cast<const float*>(trade ? p->planes[DUST_PLANE_ACCUM].p : p->hist_accum[in].p);
  d.hist_out_accum = static_cast<float*>(trade ? p->hist_accum[0].p : p->hist_accum[out].p);
  d.hist_in_geo = static_cast<const uint32_t*>(p->hist_geo[in].p);
  d.hist_out_geo = static_cast<uint32_t*>(p->hist_geo[out].p);
  if (trade != p->hist_traded) p->have_history = false;  // the plane was bound or released since the last frame: start over
  p->hist_traded = trade;
  d.cam = a.cam; d.prev = p->prev_cam;
  d.have_history = p->have_history ? 1u : 0u;
  d.width = p->width; d.height = p->height; d.frame_index = f.fp->frame_index;
  d.aspect = a.aspect;
  d.max_frames = float(std::max(1u, p->denoise.max_accumulated_frames));
  d.disocclusion = p->denoise.disocclusion_threshold;
  d.antilag_sigma = p->denoise.antilag_sigma_scale;
  d.antilag_power = p->denoise.antilag_power;
  d.max_radius = p->denoise.max_blur_radius;
  HIP_TRY(dust::launch_denoise(d, f.st));
  // DUST_PLANE_ACCUM shows the temporal accumulation (rgb + frame count) of the frame just filtered
  if (trade) { std::swap(p->planes[DUST_PLANE_ACCUM].p, p->hist_accum[0].p); std::swap(p->planes[DUST_PLANE_ACCUM].bytes, p->hist_accum[0].bytes); }
  else HIP_TRY(hipMemcpyAsync(p->plane(DUST_PLANE_ACCUM), d.hist_out_accum, px * 16, hipMemcpyDeviceToDevice, f.st));
  p->hist_parity = out;
  p->have_history = true;
  p->prev_cam = a.cam;
  return DUST_OK;
}

// One frame: its descriptor, its plan, then its passes in order, each a function above.
static DustStatus render_frame_impl(DustHipPipeline* p, const DustHipScene* s, const DustHipCamera* cam, const DustHipSky* sky,
                                    const DustHipFrameParams* fp_in, FrameRole role, BatchJoin* join) {
  DustHipFrameParams fp_copy{};
  DUST_TRY(check_frame(p, s, cam, sky, fp_in, fp_copy));
  const DustHipFrameParams* fp = &fp_copy;
  if ((fp->passes & (DUST_PASS_FINAL_GATHER | DUST_PASS_SURFEL)) && !p->gi_hash.p)
    DUST_TRY(dust_hip_pipeline_configure_gi(p, dust::kSpatialHashCapacity, dust::kSurfelPoolSize));
  DustHipContext* ctx = p->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const Tuning& tune = p->tune;
  const bool batched = role != FrameRole::Single;
  // ---- 1. the descriptor
  dust::FrameArgs a{};
  s->touch();
  frame_args(p, s, cam, sky, fp, a);
  Frame f{p, ctx, s, fp, ctx->stream};
  const hipStream_t st = f.st;
  f.count = fp->passes & DUST_PASS_COUNT_STATS;
  f.sharded = (fp->passes & DUST_PASS_GI_SHARDED) != 0;
  f.fg_stream = dust::gather_as_stream(fp->passes, a.grid.cells != nullptr, tune.gi_path, a.deep != 0, tune.debug, tune.no_gather_order);
  f.sf_stream = dust::surfel_as_stream(fp->passes, a.grid.cells != nullptr, tune.gi_path);
  if (f.fg_stream || f.sf_stream) DUST_TRY(ensure_stream_buffers(p, f.fg_stream, f.sf_stream));
  // ---- 2. the plan (frame_plan.hpp). Whether the roots and lists fit does not depend on the share: asked first, before anything of the pipeline changes
  f.si = slot_inputs(p, a);
  if (dust::slot_plan(f.si).too_big) return fail(DUST_ERR_INVALID_ARGUMENT, "staged roots and candidate lists exceed the device's LDS");
  p->stats_valid = false;
  // (the further frames of a batched launch have no launch of their own to time: frame 0's pair brackets the launch of all of them)
  const uint32_t stride = dust::timing_stride(ctx->timing_stride, batched, batched ? join->n : 1u);
  const bool times_launch = !batched || join->slot == 0;   // (a launch of several frames: frame 0's pipeline)
  p->timed_frame = times_launch && ctx->timing && dust::launch_timed(p->frame_counter++, stride);
  // (a frame that is not timed has no times: dust_hip_pipeline_pass_stats must not hand out an earlier frame's)
  if (!p->timed_frame) for (bool& v : p->ev_valid) v = false;
  DUST_TRY(side_share(f, a));
  f.si.share = f.share;
  f.plan = dust::slot_plan(f.si);
  a.n_lds_boxes = f.plan.n_lds_boxes;
  p->view_key = dust::view_key(*cam, s, s->revision, *sky, a.row_begin, a.row_end);
  if (f.count) HIP_TRY(hipMemsetAsync(p->stats.p, 0, 8 * sizeof(dust::DevStats), st));
  // ---- 3. the passes. Primary + AO in one launch unless told otherwise (DUST_HIP_NO_FUSE=1 keeps the reference's one-launch-per-pass shape)
  const bool fuse = (fp->passes & DUST_PASS_PRIMARY) && (fp->passes & DUST_PASS_AMBIENT_OCCLUSION) && !tune.no_fuse;
  p->fused_last = fuse;
  if (f.calibrate) HIP_TRY(hipEventRecord(p->side_cal.p0, st));
  if (batched && (!fuse || f.count)) return fail(DUST_ERR_INVALID_ARGUMENT, "a batched frame must be a fused primary + AO frame");  // (dust_hip_render_frames checks)
  if (fuse) {
    DUST_TRY(fused_pass(f, a, cam, sky, role, join));
    if (role == FrameRole::Follower) return DUST_OK;   // (prepared: the Lead launches it)
  }
  if (!fuse && (fp->passes & DUST_PASS_PRIMARY)) DUST_TRY(pixel_pass(f, a, 0));
  if (!fuse && (fp->passes & DUST_PASS_AMBIENT_OCCLUSION)) DUST_TRY(pixel_pass(f, a, 1));
  if (f.calibrate) HIP_TRY(hipEventRecord(p->side_cal.p1, st));
  if (fp->passes & DUST_PASS_FINAL_GATHER) {
    if (f.sharded) {  // pixels that stamp nothing must read 0 after the all-gather
      a.gi.touched = static_cast<uint32_t*>(p->gi_touched.p);
      a.gi.merged = static_cast<dust::DevSurfel*>(p->gi_merged.p);
      HIP_TRY(hipMemsetAsync(a.gi.touched + size_t(a.row_begin) * p->width, 0, size_t(a.row_end - a.row_begin) * p->width * 4, st));
    }
    a.stats = static_cast<dust::DevStats*>(p->stats.p) + 3;
    DUST_TRY(f.fg_stream ? gather_stream_pass(f, a) : gather_packet_pass(f, a));
  }
  if (fp->passes & DUST_PASS_SURFEL) DUST_TRY(surfel_pass(f, a));
  if (fp->passes & DUST_PASS_ACCUMULATE) DUST_TRY(accumulate_pass(f, a));
  if (fp->passes & DUST_PASS_DENOISE) DUST_TRY(denoise_pass(f, a));
  if (f.count) {
    HIP_TRY(hipMemcpyAsync(p->host_stats, p->stats.p, 8 * sizeof(dust::DevStats), hipMemcpyDeviceToHost, st));
    p->stats_valid = true;
  }
  return DUST_OK;
}

DustStatus dust_hip_render_frame(DustHipPipeline* p, const DustHipScene* s, const DustHipCamera* cam,
                                 const DustHipSky* sky, const DustHipFrameParams* fp_in) {
  return render_frame_impl(p, s, cam, sky, fp_in, FrameRole::Single, nullptr);
}
// The frames [0, n) can share one launch: fused primary + AO frames and nothing else, of distinct pipelines of the scene's context with one
// frame size, one row band and the same launch-shaping settings, and no surfel pass outstanding beside them.
static bool batchable(uint32_t n, DustHipPipeline* const* pipes, const DustHipScene* s, const DustHipFrameParams* fps) {
  if (n < 2 || n > dust::kMaxBatch) return false;
  const DustHipPipeline* p0 = pipes[0];
  if (p0->ctx != s->ctx || p0->ctx->side_busy) return false;
  const uint32_t want = DUST_PASS_PRIMARY | DUST_PASS_AMBIENT_OCCLUSION;
  for (uint32_t i = 0; i < n; ++i) {
    const DustHipPipeline* p = pipes[i];
    const Tuning& t = p->tune; const Tuning& t0 = p0->tune;
    if (p->ctx != p0->ctx || p->width != p0->width || p->height != p0->height) return false;
    if (fps[i].passes != want || fps[i].row_begin != fps[0].row_begin || fps[i].row_end != fps[0].row_end) return false;
    if (t.no_fuse || t.block != t0.block || t.blocks_per_cu != t0.blocks_per_cu || t.no_lds_boxes != t0.no_lds_boxes || t.wide_fused != t0.wide_fused ||
        t.debug != t0.debug || t.static_rounds != t0.static_rounds || t.no_shared_view != t0.no_shared_view || t.reserve_blocks != t0.reserve_blocks || p->in_collective != p0->in_collective ||
        p->frames_in_flight != p0->frames_in_flight || (p->frames_in_flight > 1 && t.in_flight_slots != t0.in_flight_slots))
      return false;
    for (uint32_t j = 0; j < i; ++j)
      if (pipes[j] == p) return false;   // (the same pipeline twice: the second frame overwrites the first -- in sequence)
  }
  return true;
}
// what the host does to the scene before frame i (the reference's tlas_system pushes the moved entities every frame, tlas.rs:79-128)
static DustStatus apply_moves(DustHipScene* s, const DustHipFrameMoves& m) {
  if (!m.n) return DUST_OK;
  for (uint32_t j = 0; j < m.n; ++j) {
    DustStatus ms = dust_hip_scene_set_transform(s, m.instance_ids[j], m.obj_to_world + size_t(j) * 12, m.prev_obj_to_world ? m.prev_obj_to_world + size_t(j) * 16 : nullptr);
    if (ms != DUST_OK) return ms;
  }
  return dust_hip_scene_commit(s);
}
DustStatus dust_hip_render_frames(uint32_t n_frames, DustHipPipeline* const* pipelines, DustHipScene* s, const DustHipCamera* cameras,
                                  const DustHipSky* skies, const DustHipFrameParams* params, const DustHipFrameMoves* moves) {
  if (!pipelines || !s || !cameras || !skies || !params) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (!n_frames) return DUST_OK;
  return guarded([&]() -> DustStatus {
  // every frame's arguments are checked before the first one is enqueued (and before the scene is touched)
  std::vector<DustHipFrameParams> fps(n_frames);
  for (uint32_t i = 0; i < n_frames; ++i) {
    // (params[] is an array of THIS library's struct: every element must say so, or the stride is not ours)
    if (params[i].struct_size != sizeof(DustHipFrameParams)) return fail(DUST_ERR_INVALID_ARGUMENT, "dust_hip_render_frames: params[i].struct_size must be sizeof(DustHipFrameParams)");
    DustStatus cs = check_frame(pipelines[i], s, &cameras[i], &skies[i], &params[i], fps[i]);
    if (cs != DUST_OK) return cs;
    if (moves && moves[i].n) {
      if (!moves[i].instance_ids || !moves[i].obj_to_world) return fail(DUST_ERR_INVALID_ARGUMENT, "dust_hip_render_frames: moves[i] without instance ids or transforms");
      for (uint32_t j = 0; j < moves[i].n; ++j)
        if (moves[i].instance_ids[j] >= s->instances.size()) return fail(DUST_ERR_INVALID_ARGUMENT, "dust_hip_render_frames: moves[i] names an instance the scene does not have");
    }
  }
  for (uint32_t at = 0; at < n_frames;) {
    uint32_t n = std::min<uint32_t>(dust::kMaxBatch, n_frames - at);
    while (n >= 2 && !batchable(n, pipelines + at, s, fps.data() + at)) --n;   // the longest run from here that can share a launch
    if (n < 2) {   // one frame, or a frame that cannot share a launch with its successor: in sequence, the same results
      if (moves) { DustStatus ms = apply_moves(s, moves[at]); if (ms != DUST_OK) return ms; }
      DustStatus rs = render_frame_impl(pipelines[at], s, &cameras[at], &skies[at], &params[at], FrameRole::Single, nullptr);
      if (rs != DUST_OK) return rs;
      at += 1;
      continue;
    }
    // in frame order: the scene as frame i sees it (its moves committed: a scene image of its own in the ring), then frame i's descriptor against it;
    // the last frame's preparation launches them all. At most kMaxBatch commits lie between two launches -- the ring holds as many images --, so no
    // commit of this run lands on an image one of its own frames still waits to read.
    static_assert(dust::kMaxBatch <= DustHipScene::kImages, "a launch's frames must fit the scene's ring of images");
    BatchJoin join;
    join.n = n;
    for (uint32_t i = 0; i < n; ++i) {
      DustStatus rs = moves ? apply_moves(s, moves[at + i]) : DUST_OK;
      join.slot = i;
      if (rs == DUST_OK) rs = render_frame_impl(pipelines[at + i], s, &cameras[at + i], &skies[at + i], &params[at + i], i + 1 == n ? FrameRole::Lead : FrameRole::Follower, &join);
      if (rs != DUST_OK) {
        // (a HIP failure or a commit that could not grow the scene: the frames prepared so far are never launched -- their pipelines took a set of
        //  work counters for nothing, and no launch zeroed the other one: give it back, or their next launch would pull tiles from a set that an
        //  earlier launch has counted up)
        // (frame i's own too, when it failed behind take_counters; not once the launch is enqueued: the sets are then in use as taken)
        for (uint32_t j = 0; j <= i && !join.launched; ++j)
          if (join.took_counters[j]) pipelines[at + j]->counter_parity[0] ^= 1u;
        return rs;
      }
    }
    at += n;
  }
  return DUST_OK;
  });
}

DustStatus dust_hip_pipeline_pass_stats(DustHipPipeline* p, uint32_t pass, DustHipPassStats* out) {
  if (!p || !out || pass > 5) return fail(DUST_ERR_INVALID_ARGUMENT, "bad pass index");
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(sync_stream(p->ctx));
  // pass 0: primary kernel; 1, 2: the two ray classes of the AO kernel (share its time); 3: final gather (+ surfel
  // commit); 4, 5: the two ray classes of the surfel pass (trace + apply kernels)
  const int kernel = pass == 0 ? 0 : (pass <= 2 ? 1 : (pass == 3 ? 2 : 3));
  if (kernel >= 0 && p->ctx->timing && p->ev_valid[kernel]) {
    float ms = 0.0f;
    const uint32_t slot = (p->ev_head[kernel] - 1u) % DustHipPipeline::kEvRing;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev_ring[kernel][0][slot], p->ev_ring[kernel][1][slot]));
    out->ms = ms;
  }
  if (p->stats_valid) {
    const dust::DevStats& s = p->host_stats[pass];
    out->rays = s.rays; out->instances_tested = s.instances_tested; out->upper_descents = s.upper_descents;
    out->mid_descents = s.mid_descents; out->bricks_tested = s.bricks_tested; out->hits = s.hits;
  }
  return DUST_OK;
}
DustStatus dust_hip_pipeline_kernel_times(DustHipPipeline* p, int mark, float ms_sum[4], uint32_t launches[4]) {
  if (!p) return fail(DUST_ERR_INVALID_ARGUMENT, "null pipeline");
  if (mark && !ms_sum && !launches) {  // "from here": no wait, nothing read (a timed region starts right behind it)
    for (int k = 0; k < 4; ++k) p->ev_mark[k] = p->ev_head[k];
    return DUST_OK;
  }
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(sync_stream(p->ctx));
  for (int k = 0; k < 4; ++k) {
    double sum = 0.0;
    uint32_t n = 0;
    if (p->ctx->timing) {
      const uint32_t head = p->ev_head[k];
      uint32_t from = p->ev_mark[k];
      if (head - from > DustHipPipeline::kEvRing) from = head - DustHipPipeline::kEvRing;  // older pairs have been recorded over
      for (uint32_t i = from; i != head; ++i) {
        const uint32_t slot = i % DustHipPipeline::kEvRing;
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev_ring[k][0][slot], p->ev_ring[k][1][slot]));
        sum += ms; ++n;
      }
      if (mark) p->ev_mark[k] = head;
    }
    if (ms_sum) ms_sum[k] = float(sum);
    if (launches) launches[k] = n;
  }
  return DUST_OK;
}
DustStatus dust_hip_pipeline_plane_device_ptr(DustHipPipeline* p, DustHipPlane plane, void** ptr, size_t* bytes) {
  if (!p || int(plane) < 0 || plane >= DUST_PLANE_COUNT) return fail(DUST_ERR_INVALID_ARGUMENT, "bad plane");
  if (ptr) *ptr = p->plane(plane);
  if (bytes) *bytes = p->planes[plane].bytes;
  return DUST_OK;
}
DustStatus dust_hip_pipeline_bind_plane(DustHipPipeline* p, DustHipPlane plane, void* device_ptr, size_t bytes) {
  if (!p || int(plane) < 0 || plane >= DUST_PLANE_COUNT) return fail(DUST_ERR_INVALID_ARGUMENT, "bad plane");
  if (device_ptr && bytes < p->planes[plane].bytes) return fail(DUST_ERR_INVALID_ARGUMENT, "bound storage is smaller than the plane");
  if (device_ptr && (reinterpret_cast<uintptr_t>(device_ptr) & 15u)) return fail(DUST_ERR_INVALID_ARGUMENT, "bound storage must be 16-byte aligned");
  p->bound[plane] = device_ptr;  // launches enqueued from now on use it; the caller orders its own use of the memory on the stream
  return DUST_OK;
}
DustStatus dust_hip_pipeline_read_plane(DustHipPipeline* p, DustHipPlane plane, void* dst, size_t dst_bytes) {
  if (!p || !dst || int(plane) < 0 || plane >= DUST_PLANE_COUNT) return fail(DUST_ERR_INVALID_ARGUMENT, "bad plane");
  if (dst_bytes < p->planes[plane].bytes) return fail(DUST_ERR_INVALID_ARGUMENT, "destination too small");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(sync_stream(p->ctx));
  HIP_TRY(copy_wait(dst, p->plane(plane), p->planes[plane].bytes, hipMemcpyDeviceToHost, p->ctx->stream));
  ++p->ctx->sync_epoch;  // (copy_wait waited for the stream)
  return DUST_OK;
}
DustStatus dust_hip_pipeline_configure_gi(DustHipPipeline* p, uint32_t hash_capacity, uint32_t surfel_pool_size) {
  if (!p || hash_capacity < 4 || surfel_pool_size == 0) return fail(DUST_ERR_INVALID_ARGUMENT, "bad GI configuration");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(sync_stream(p->ctx));
  // a pending sharded surfel trace is cancelled (its permutation lives in gi_sort_vals, re-made below), and its staging arrays, sized
  // for the old pool, go (the next sharded trace makes them for the new one)
  p->sf_shard = {};
  for (DeviceBuffer* b : {&p->gi_stage_req, &p->gi_stage_repl, &p->gi_stage_sun}) b->release();
  p->gi_stage_slots = 0;
  const size_t hash_bytes = (size_t(hash_capacity) + 2) * 12;  // probes run up to 2 past the end (spatial_hash.glsl:154-158)
  HIP_TRY(p->gi_hash.alloc(hash_bytes));
  HIP_TRY(hipMemsetAsync(p->gi_hash.p, 0, hash_bytes, p->ctx->stream));             // standard.rs:348-358 relies on a zeroed allocation
  HIP_TRY(p->gi_pool.alloc(size_t(surfel_pool_size) * 16));
  HIP_TRY(hipMemsetAsync(p->gi_pool.p, 0xFF, size_t(surfel_pool_size) * 16, p->ctx->stream));  // fill_buffer(u32::MAX), standard.rs:345-347
  HIP_TRY(p->gi_owner.alloc(size_t(surfel_pool_size) * 4));
  HIP_TRY(hipMemsetAsync(p->gi_owner.p, 0, size_t(surfel_pool_size) * 4, p->ctx->stream));
  HIP_TRY(p->gi_pixel_surfel.alloc(size_t(p->width) * p->height * 16));
  {
    const size_t tiles = size_t((p->width + 63) / 64) * ((p->height + 63) / 64 + 1);
    HIP_TRY(p->gi_order.alloc(tiles * 4096 * 4));
    HIP_TRY(p->gi_order_count.alloc(tiles * 4));
  }
  HIP_TRY(p->gi_requests.alloc(size_t(surfel_pool_size) * sizeof(dust::DevHashRequest)));
  HIP_TRY(p->gi_replacement.alloc(size_t(surfel_pool_size) * 16));
  HIP_TRY(p->gi_sun_payload.alloc(size_t(surfel_pool_size) * 16));
  for (DeviceBuffer* b : {&p->gi_sort_keys[0], &p->gi_sort_keys[1], &p->gi_sort_vals[0], &p->gi_sort_vals[1]}) HIP_TRY(b->alloc(size_t(surfel_pool_size) * 4));
  HIP_TRY(p->gi_sort_scratch.alloc(dust::radix_sort_scratch_bytes(surfel_pool_size)));
  HIP_TRY(p->gi_apply_alive.alloc(((size_t(surfel_pool_size) + 63) / 64 + 1) * 8 * 3));   // alive, cluster starts, run starts
  HIP_TRY(p->gi_apply_dead.alloc(size_t(surfel_pool_size)));
  HIP_TRY(hipMemsetAsync(p->gi_apply_dead.p, 0, size_t(surfel_pool_size), p->ctx->stream));
  // (the ray streams' buffers -- 48 B per pixel and more -- are made by the first frame that takes a stream path: ensure_stream_buffers)
  for (DeviceBuffer* b : {&p->gi_rays_fg, &p->gi_groups_fg, &p->gi_fg_hits, &p->gi_rays_sf, &p->gi_groups_sf, &p->gi_unbinned, &p->gi_hits_sf}) b->release();
  p->gi_capacity = hash_capacity;
  p->gi_pool_size = surfel_pool_size;
  p->gi_touched_rows = 0;  // the exchange buffers follow the pool size: dust_hip_pipeline_gi_exchange re-creates them
  p->gi_touched.release();
  p->gi_merged.release();
  return DUST_OK;
}
DustStatus dust_hip_pipeline_gi_exchange(DustHipPipeline* p, uint32_t padded_rows, DustHipGiExchange* out) {
  if (!p || !out || padded_rows < p->height) return fail(DUST_ERR_INVALID_ARGUMENT, "padded_rows must cover the frame");
  STRUCT_TRY(out, "DustHipGiExchange");
  HIP_TRY(hipSetDevice(p->ctx->device));
  if (!p->gi_hash.p) {
    DustStatus gs = dust_hip_pipeline_configure_gi(p, dust::kSpatialHashCapacity, dust::kSurfelPoolSize);
    if (gs != DUST_OK) return gs;
  }
  if (!p->gi_touched.p || p->gi_touched_rows != padded_rows) {
    HIP_TRY(sync_stream(p->ctx));
    HIP_TRY(p->gi_touched.alloc(size_t(padded_rows) * p->width * 4));
    HIP_TRY(hipMemsetAsync(p->gi_touched.p, 0, size_t(padded_rows) * p->width * 4, p->ctx->stream));
    HIP_TRY(p->gi_merged.alloc(size_t(p->gi_pool_size) * 16));
    HIP_TRY(hipMemsetAsync(p->gi_merged.p, 0, size_t(p->gi_pool_size) * 16, p->ctx->stream));
    p->gi_touched_rows = padded_rows;
  }
  exchange_view(p, padded_rows, out);
  return DUST_OK;
}
static DustStatus gi_exchange_launch(DustHipPipeline* p, uint32_t row_begin, uint32_t row_end, uint32_t frame_index, bool import) {
  if (!p || !p->gi_touched.p) return fail(DUST_ERR_NOT_READY, "call dust_hip_pipeline_gi_exchange first");
  // an EMPTY range is fine: a rank whose band lies past the end of the frame still repeats the others' stamps and commits the
  // winners (import), and must contribute zeroes -- not last frame's all-reduced sum -- to the merge (export)
  if (row_begin > row_end || row_end > p->height) return fail(DUST_ERR_INVALID_ARGUMENT, "bad row range");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(join_side(p->ctx));
  dust::FrameArgs a{};
  frame_size_args(p, a);
  a.row_begin = row_begin; a.row_end = row_end;
  a.frame_index = frame_index;
  gi_args(p, a.gi);
  a.gi.touched = static_cast<uint32_t*>(p->gi_touched.p);
  a.gi.merged = static_cast<dust::DevSurfel*>(p->gi_merged.p);
  HIP_TRY(import ? dust::launch_gi_import(a, p->ctx->stream) : dust::launch_gi_export(a, p->ctx->stream));
  return DUST_OK;
}
DustStatus dust_hip_gi_export(DustHipPipeline* p, uint32_t row_begin, uint32_t row_end) {
  return gi_exchange_launch(p, row_begin, row_end, 0, false);
}
DustStatus dust_hip_gi_import(DustHipPipeline* p, uint32_t row_begin, uint32_t row_end, uint32_t frame_index) {
  return gi_exchange_launch(p, row_begin, row_end, frame_index, true);
}
DustStatus dust_hip_pipeline_read_gi(DustHipPipeline* p, uint32_t which, void* dst, size_t dst_bytes) {
  if (!p || !dst || which > 1 || !p->gi_hash.p) return fail(DUST_ERR_INVALID_ARGUMENT, "GI state not configured");
  const DeviceBuffer& b = which == 0 ? p->gi_hash : p->gi_pool;
  if (dst_bytes < b.bytes) return fail(DUST_ERR_INVALID_ARGUMENT, "destination too small");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(join_side(p->ctx));
  HIP_TRY(sync_stream(p->ctx));
  HIP_TRY(copy_wait(dst, b.p, b.bytes, hipMemcpyDeviceToHost, p->ctx->stream));
  return DUST_OK;
}
DustStatus dust_hip_pipeline_write_gi(DustHipPipeline* p, uint32_t which, const void* src, size_t src_bytes) {
  if (!p || !src || which > 1 || !p->gi_hash.p) return fail(DUST_ERR_INVALID_ARGUMENT, "GI state not configured");
  const DeviceBuffer& b = which == 0 ? p->gi_hash : p->gi_pool;
  if (src_bytes != b.bytes) return fail(DUST_ERR_INVALID_ARGUMENT, "saved GI state does not match the configured capacity / pool size");
  if (p->sf_shard.pending)   // (its completion would overwrite the pool and stamp the hash over what is restored here)
    return fail(DUST_ERR_NOT_READY, "a sharded surfel trace is pending on this pipeline: complete it (dust_hip_gi_surfel_exchange_run) or cancel it (dust_hip_pipeline_clear) first");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(join_side(p->ctx));
  HIP_TRY(copy_wait(b.p, src, b.bytes, hipMemcpyHostToDevice, p->ctx->stream));
  return DUST_OK;
}
DustStatus dust_hip_tone_map(DustHipPipeline* p, const DustHipToneMapParams* tp) {
  if (!p || !tp) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(tp, "DustHipToneMapParams");
  if (tp->transfer_function > 8) return fail(DUST_ERR_INVALID_ARGUMENT, "transfer function must be 0..8");
  if (!(tp->max_log_luminance > tp->min_log_luminance)) return fail(DUST_ERR_INVALID_ARGUMENT, "empty luminance range");
  HIP_TRY(hipSetDevice(p->ctx->device));
  uint32_t* hist = static_cast<uint32_t*>(p->exposure.p);
  HIP_TRY(dust::launch_tone_map(static_cast<const uint16_t*>(p->plane(DUST_PLANE_DENOISED)),
                                static_cast<const uint32_t*>(p->plane(DUST_PLANE_ALBEDO)),
                                static_cast<uint16_t*>(p->plane(DUST_PLANE_OUTPUT)), p->width * p->height, hist,
                                reinterpret_cast<float*>(hist + 256), tp->min_log_luminance,
                                tp->max_log_luminance - tp->min_log_luminance, tp->time_coefficient, tp->color_space_conversion,
                                tp->transfer_function, p->ctx->stream));
  return DUST_OK;
}
DustStatus dust_hip_pipeline_exposure(DustHipPipeline* p, float* avg_luminance, const float* set_to) {
  if (!p) return fail(DUST_ERR_INVALID_ARGUMENT, "null pipeline");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(sync_stream(p->ctx));
  float* avg = reinterpret_cast<float*>(static_cast<uint32_t*>(p->exposure.p) + 256);
  if (set_to) HIP_TRY(copy_wait(avg, set_to, 4, hipMemcpyHostToDevice, p->ctx->stream));
  if (avg_luminance) HIP_TRY(copy_wait(avg_luminance, avg, 4, hipMemcpyDeviceToHost, p->ctx->stream));
  return DUST_OK;
}
DustStatus dust_hip_device_eval(DustHipContext* ctx, uint32_t fn, const uint32_t* in, uint32_t in_words, uint32_t* out,
                                uint32_t out_words, uint32_t n) {
  static const uint32_t kWords[20][2] = {{9, 3}, {9, 3}, {9, 3}, {3, 1}, {1, 3}, {4, 1}, {1, 3}, {4, 2}, {2, 4}, {4, 1}, {3, 4}, {6, 3}, {2, 2}, {1, 1}, {1, 2},
                                         {3, 3}, {3, 3}, {4, 6}, {5, 2}, {14, 9}};
  if (!ctx || !in || !out || fn >= 20) return fail(DUST_ERR_INVALID_ARGUMENT, "bad device function");
  if (in_words != kWords[fn][0] || out_words != kWords[fn][1]) return fail(DUST_ERR_INVALID_ARGUMENT, "row width does not match the function");
  if (n == 0) return DUST_OK;
  // fns 15, 16: the 56 floats of the sky state ride in the first 19 rows (3 words each, the last word padding) and go into the kernel argument
  const bool with_sky = fn == 15 || fn == 16;
  if (with_sky && n < 19) return fail(DUST_ERR_INVALID_ARGUMENT, "fns 15 and 16 want the sky state in rows 0..18");
  HIP_TRY(hipSetDevice(ctx->device));
  if (fn == 12) {  // the surfel pass's radix sort on caller-given (key, value) rows, all 32 key bits
    std::vector<uint32_t> k(n), v(n);
    for (uint32_t i = 0; i < n; ++i) { k[i] = in[size_t(i) * 2]; v[i] = in[size_t(i) * 2 + 1]; }
    DeviceBuffer ka, va, kb, vb, scratch;
    HIP_TRY(ka.upload(k.data(), size_t(n) * 4, ctx->stream)); HIP_TRY(va.upload(v.data(), size_t(n) * 4, ctx->stream));
    HIP_TRY(kb.alloc(size_t(n) * 4)); HIP_TRY(vb.alloc(size_t(n) * 4));
    HIP_TRY(scratch.alloc(dust::radix_sort_scratch_bytes(n)));
    bool in_b = false;
    HIP_TRY(dust::radix_sort_pairs(scratch.p, static_cast<uint32_t*>(ka.p), static_cast<uint32_t*>(va.p), static_cast<uint32_t*>(kb.p),
                                   static_cast<uint32_t*>(vb.p), n, in_words == 2 ? 32u : 32u, &in_b, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(copy_wait(k.data(), in_b ? kb.p : ka.p, size_t(n) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(copy_wait(v.data(), in_b ? vb.p : va.p, size_t(n) * 4, hipMemcpyDeviceToHost, ctx->stream));
    for (uint32_t i = 0; i < n; ++i) { out[size_t(i) * 2] = k[i]; out[size_t(i) * 2 + 1] = v[i]; }
    return DUST_OK;
  }
  if (fn == 13 || fn == 14) {  // the cost-ordered hand-out's sorter (k_tile_order) on caller-given tile costs: rows in = cycles, rows out = tile order
    // fn 14: with cost-balanced bands; out rows are then {order, cut}: the kRegions + 1 cuts in the second word of the first rows (n >= 9)
    if (fn == 14 && (out_words != 2 || n < dust::kRegions + 1)) return fail(DUST_ERR_INVALID_ARGUMENT, "fn 14 wants 2 output words and at least 9 rows");
    DeviceBuffer cost, order, cuts;
    HIP_TRY(cost.upload(in, size_t(n) * 4, ctx->stream));
    HIP_TRY(order.alloc(size_t(n) * 4));
    HIP_TRY(cuts.alloc(size_t(dust::kRegions + 1) * 4));
    HIP_TRY(hipMemsetAsync(order.p, 0xFF, size_t(n) * 4, ctx->stream));
    HIP_TRY(dust::launch_tile_order(static_cast<const uint32_t*>(cost.p), static_cast<uint32_t*>(order.p), fn == 14 ? static_cast<uint32_t*>(cuts.p) : nullptr, false,
                                    n, (n + dust::kRegions - 1) / dust::kRegions, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (fn == 13) { HIP_TRY(copy_wait(out, order.p, size_t(n) * 4, hipMemcpyDeviceToHost, ctx->stream)); return DUST_OK; }
    std::vector<uint32_t> o(n), c(dust::kRegions + 1);
    HIP_TRY(copy_wait(o.data(), order.p, size_t(n) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(copy_wait(c.data(), cuts.p, c.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    for (uint32_t i = 0; i < n; ++i) { out[size_t(i) * 2] = o[i]; out[size_t(i) * 2 + 1] = i < c.size() ? c[i] : 0u; }
    return DUST_OK;
  }
  DeviceBuffer din, dout;
  HIP_TRY(din.upload(in, size_t(n) * in_words * 4, ctx->stream));
  HIP_TRY(dout.alloc(size_t(n) * out_words * 4));
  HIP_TRY(hipMemsetAsync(dout.p, 0, size_t(n) * out_words * 4, ctx->stream));
  HIP_TRY(dust::launch_device_eval(fn, static_cast<const uint32_t*>(din.p), in_words, static_cast<uint32_t*>(dout.p), out_words, n,
                                   with_sky ? reinterpret_cast<const float*>(in) : nullptr, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(copy_wait(out, dout.p, size_t(n) * out_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  return DUST_OK;
}
DustStatus dust_hip_pipeline_tile_costs(DustHipPipeline* p, uint32_t pass_kind, uint32_t* cycles, uint32_t capacity, uint32_t* tiles_x, uint32_t* tiles_y) {
  if (!p || pass_kind > 3) return fail(DUST_ERR_INVALID_ARGUMENT, "bad pass kind");
  const DustHipPipeline::TileHistory& h = p->tile_history[pass_kind];
  if (tiles_x) *tiles_x = h.measured ? h.tiles_x : 0;
  if (tiles_y) *tiles_y = h.measured ? h.tiles_y : 0;
  if (!cycles || !h.measured) return DUST_OK;
  if (capacity < h.tiles_x * h.tiles_y) return fail(DUST_ERR_INVALID_ARGUMENT, "destination too small");
  HIP_TRY(hipSetDevice(p->ctx->device));
  HIP_TRY(sync_stream(p->ctx));
  HIP_TRY(copy_wait(cycles, h.cost.p, size_t(h.tiles_x) * h.tiles_y * 4, hipMemcpyDeviceToHost, p->ctx->stream));
  return DUST_OK;
}
DustStatus dust_hip_pipeline_set_denoiser(DustHipPipeline* p, const DustHipDenoiseParams* dp) {
  if (!p || !dp) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(dp, "DustHipDenoiseParams");
  if (dp->max_accumulated_frames == 0 || !(dp->disocclusion_threshold > 0.0f) || !(dp->antilag_sigma_scale >= 0.0f) ||
      !(dp->antilag_power >= 0.0f && dp->antilag_power <= 1.0f) || !(dp->max_blur_radius >= 0.0f && dp->max_blur_radius <= 64.0f))
    return fail(DUST_ERR_INVALID_ARGUMENT, "denoiser settings out of range");
  p->denoise = *dp;
  p->denoise.struct_size = sizeof(DustHipDenoiseParams);
  return DUST_OK;
}
DustStatus dust_hip_pipeline_restart_denoiser(DustHipPipeline* p) {
  if (!p) return fail(DUST_ERR_INVALID_ARGUMENT, "null pipeline");
  p->have_history = false;  // DenoiserEvent::Restart (nrd.rs:749-755): the next frame starts a new accumulation
  return DUST_OK;
}
DustStatus dust_hip_pipeline_set_frames_in_flight(DustHipPipeline* p, uint32_t n) {
  if (!p) return fail(DUST_ERR_INVALID_ARGUMENT, "null pipeline");
  if (n < 1 || n > 16) return fail(DUST_ERR_INVALID_ARGUMENT, "frames in flight: 1..16");
  p->frames_in_flight = n;
  return DUST_OK;
}
DustStatus dust_hip_pipeline_configure(DustHipPipeline* p, const DustHipPipelineConfig* cfg) {
  if (!p || !cfg) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(cfg, "DustHipPipelineConfig");
  if (cfg->gi_path > DUST_GI_PATH_STREAMS || cfg->side_stream > DUST_SIDE_STREAM_OFF || cfg->in_flight_slots > DUST_IN_FLIGHT_ALL ||
      cfg->frames_in_flight > 16 || (cfg->side_share != 0 && (cfg->side_share < 5 || cfg->side_share > 90)))
    return fail(DUST_ERR_INVALID_ARGUMENT, "DustHipPipelineConfig: a field is out of range");
  Tuning& t = p->tune;
  t.reserve_blocks = cfg->reserve_blocks == DUST_RESERVE_AUTO ? DUST_RESERVE_AUTO : (cfg->reserve_blocks & ~7u);  // whole rounds over the 8 XCDs
  t.gi_path = cfg->gi_path;
  t.no_side_stream = cfg->side_stream == DUST_SIDE_STREAM_OFF;
  t.side_share = cfg->side_share;
  t.in_flight_slots = cfg->in_flight_slots;
  if (cfg->frames_in_flight) p->frames_in_flight = cfg->frames_in_flight;
  return DUST_OK;
}
DustStatus dust_hip_pipeline_get_config(const DustHipPipeline* p, DustHipPipelineConfig* out) {
  if (!p || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(out, "DustHipPipelineConfig");
  const Tuning& t = p->tune;
  out->reserve_blocks = t.reserve_blocks;
  out->gi_path = t.gi_path;
  out->side_stream = t.no_side_stream ? DUST_SIDE_STREAM_OFF : DUST_SIDE_STREAM_AUTO;
  out->side_share = t.side_share;
  out->frames_in_flight = p->frames_in_flight;
  out->in_flight_slots = t.in_flight_slots;
  return DUST_OK;
}
DustStatus dust_hip_pipeline_clear(DustHipPipeline* p) {
  if (!p) return fail(DUST_ERR_INVALID_ARGUMENT, "null pipeline");
  HIP_TRY(hipSetDevice(p->ctx->device));
  for (int i = 0; i < DUST_PLANE_COUNT; ++i) HIP_TRY(hipMemsetAsync(p->plane(i), 0, p->planes[i].bytes, p->ctx->stream));
  p->have_history = false;
  p->accum_count = 0;
  p->sf_shard = {};   // a pending sharded surfel trace is cancelled (its records are dropped)
  return DUST_OK;
}

}  // extern "C"

// ---- what comm.hip needs of the handles (capi_internal.hpp)
namespace dust_internal {
DustStatus set_error(DustStatus status, const std::string& message) { g_last_error = message; return status; }
hipStream_t context_stream(DustHipContext* c) { return c->stream; }
int context_device(DustHipContext* c) { return c->device; }
void context_retain(DustHipContext* c) { retain(c); }
void context_release(DustHipContext* c) { release(c); }
DustHipContext* pipeline_context(DustHipPipeline* p) { return p->ctx; }
void pipeline_size(DustHipPipeline* p, uint32_t* width, uint32_t* height) { *width = p->width; *height = p->height; }
DustStatus gi_exchange_view(DustHipPipeline* p, uint32_t padded_rows, DustHipGiExchange* out) {
  if (!p->gi_touched.p || p->gi_touched_rows != padded_rows)
    return fail(DUST_ERR_NOT_READY, "the GI exchange buffers were not prepared for this world x band_rows: call dust_hip_pipeline_gi_exchange(p, world * band_rows) "
                                    "BEFORE the frame's final gather (a later call would re-create them and drop the frame's stamps)");
  exchange_view(p, padded_rows, out);
  return DUST_OK;
}
void pipeline_note_collective(DustHipPipeline* p) { p->in_collective = true; }
DustStatus surfel_stage_view(DustHipPipeline* p, uint32_t world, SurfelStage* out) {
  if (!p->sf_shard.pending || !p->gi_stage_req.p) return fail(DUST_ERR_NOT_READY, "no sharded surfel trace is pending on this pipeline (dust_hip_render_frame with surfel_world >= 1 first)");
  if (world != 0 && p->sf_shard.world != world) return fail(DUST_ERR_INVALID_ARGUMENT, "the pending surfel trace was sharded for another world size than the communicator's");
  out->req = p->gi_stage_req.p; out->repl = p->gi_stage_repl.p; out->sun = p->gi_stage_sun.p;
  out->slots_per_rank = p->sf_shard.slots_per_rank; out->rank = p->sf_shard.rank; out->pool_size = p->gi_pool_size;
  return DUST_OK;
}
// the second half of a sharded surfel pass, on the context's stream behind the all-gather: records to their surfels + the trace's hash stamps, ordered apply
DustStatus surfel_finish(DustHipPipeline* p, uint32_t frame_index) {
  HIP_TRY(hipSetDevice(p->ctx->device));
  dust::FrameArgs a{};
  a.frame_index = frame_index;
  gi_args(p, a.gi);
  a.gi.perm = p->sf_shard.perm;
  a.sf_stage_req = static_cast<dust::DevHashRequest*>(p->gi_stage_req.p);
  a.sf_stage_repl = static_cast<dust::DevSurfel*>(p->gi_stage_repl.p);
  a.sf_stage_sun = static_cast<float*>(p->gi_stage_sun.p);
  const hipStream_t st = p->ctx->stream;
  HIP_TRY(dust::launch_surfel_unstage(a, st));
  p->sf_shard.pending = false;
  return apply_ordered(p, a, st);
}
void context_add_stream(DustHipContext* c, hipStream_t s) { c->extra_streams.push_back(s); }
void context_remove_stream(DustHipContext* c, hipStream_t s) {
  c->extra_streams.erase(std::remove(c->extra_streams.begin(), c->extra_streams.end(), s), c->extra_streams.end());
}
}  // namespace dust_internal
