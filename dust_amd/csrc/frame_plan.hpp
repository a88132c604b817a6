// frame_plan.hpp -- the device-free half of the frame path (capi.cpp): the integer and float arithmetic that decides every launch's shape --
// LDS budget, workgroup slots and their split, grids, the fused kernel's shape, the ray streams' LDS layout, the view key and view runs --
// and the tile schedule's state machine. No HIP call, no handle, no error state: tests/cpp/frame_plan_test.cpp drives it on a CPU.
#pragma once
#include <algorithm>
#include <cstddef>

#include "dust_dev.h"

namespace dust {

constexpr uint32_t kTileOrderMaxBand = 65536;  // (kernels.hip)

// ---- grids of the persistent launches
// packets: a workgroup per 8 tiles (one per XCD band), at least one round over the 8 XCDs, at most the slots the launch may hold
inline uint32_t packet_grid(uint32_t slots, uint32_t tiles) { return std::max(8u, std::min<uint32_t>(slots, (tiles + 7) / 8)); }
// k_ray_walk (one 1024-thread workgroup per CU: sixteen waves share one staged copy of the top-level data): `want` workgroups of 1024 rays
inline uint32_t ray_walk_grid(uint32_t slots, uint32_t block, uint32_t want) {
  return std::max(8u, std::min<uint32_t>((slots * block / 1024u) & ~7u, (want + 7u) & ~7u));
}

// ---- which GI passes of a frame run as ray streams (asked once per frame: the buffers and the launches follow the one answer)
// (the gather of a 4096^3 tree: long walks through one instance -- the one workload where a lane of its own per ray pays: 1.66 against 1.82 ms)
inline bool gather_as_stream(uint32_t passes, bool has_grid, uint32_t gi_path, bool deep, uint32_t debug, bool no_gather_order) {
  return (passes & DUST_PASS_FINAL_GATHER) && has_grid &&
         (gi_path == DUST_GI_PATH_STREAMS || (deep && gi_path != DUST_GI_PATH_PACKETS && !(debug & 12u) && !no_gather_order));
}
// (a sharded trace still runs as packets: the stream's shading kernel writes by surfel index -- run_surfel_pass)
inline bool surfel_as_stream(uint32_t passes, bool has_grid, uint32_t gi_path) {
  return (passes & DUST_PASS_SURFEL) && has_grid && gi_path == DUST_GI_PATH_STREAMS;
}

// ---- what the ray-stream kernels stage in LDS, as far as it goes. The ray-making kernels (bin; 256 threads, many workgroups per CU): grid cells,
// items and instance boxes within their budget (40 KB); k_ray_walk (one 1024-thread workgroup per CU): the enter records behind its roots.
constexpr size_t kStreamBinBudget = 40 * 1024;
inline size_t stream_walk_budget(size_t max_lds, uint32_t n_lds_models) { return max_lds - std::min<size_t>(max_lds, size_t(n_lds_models) * kN16LdsBytes); }
inline DevStreamLds stream_lds(size_t budget, bool bin, const uint32_t dim[3], uint32_t n_items, uint32_t n_instances, bool no_stream_lds) {
  DevStreamLds l;
  size_t at = 0;
  auto place = [&](size_t bytes) -> uint32_t {
    bytes = (bytes + 15) & ~size_t(15);
    if (no_stream_lds || at + bytes > budget) return 0xFFFFFFFFu;
    const uint32_t off = uint32_t(at);
    at += bytes;
    return off;
  };
  const size_t n_cells = size_t(dim[0]) * dim[1] * dim[2];
  l.cells = bin ? place(n_cells * 4) : 0xFFFFFFFFu;
  l.items = bin ? place(size_t(n_items) * 2) : 0xFFFFFFFFu;
  l.boxes = bin ? place(size_t(n_instances) * 32) : 0xFFFFFFFFu;
  l.enters = bin ? 0xFFFFFFFFu : place(size_t(n_instances) * sizeof(DevEnter));
  l.total = uint32_t(at);
  return l;
}

// ---- the surfel pass's share (percent) of the workgroup slots while it runs on the second stream beside the next frame's primary / AO kernels
// Calibrated: P, Q = the measured times of the pixel kernels and of the pass in place; 100 Q / (Q + k P) - 3 is where the measured optima of three
// workloads lie (castle 1080p 50 %, 4K 20 %, the 4096^3 tree 25 %). In single precision, as measured.
// (a scene of many instances: the pass in place is as long as its longest items, 0.19 ms for 0.10 ms of work per wave, so it needs
// fewer slots than its time says -- share sweeps of round 5's last session: 39 % at 1080p and 16 % at 4K where 1.05 gave 47 and 21,
// GI frame 0.691 -> 0.667 ms. The 4096^3 tree's pass, one instance and long walks, is as long as its work: 1.05 stays there.)
inline uint32_t calibrated_share(float P, float Q, bool deep) {
  const float k = deep ? 1.05f : 1.4f;
  return uint32_t(std::min(65.0f, std::max(10.0f, 100.0f * Q / (Q + k * P) - 3.0f)));
}
// Until then, a guess: the pass's rays against the pixel passes' (pool x 18 surfel-ray costs to 3 rays per pixel, which puts the castle at
// 50 % at 1080p and 20 % at 4K -- where round 2's feedback loop settled, without its calibration frame, event probes and waits). In double precision.
inline uint32_t guessed_share(uint32_t pool_size, uint32_t width, uint32_t rows) {
  const double surfel = double(pool_size) * 18.0, pixel = 3.0 * double(width) * double(rows);
  return uint32_t(std::min(60.0, std::max(15.0, 100.0 * surfel / (surfel + pixel))));
}

// ---- the slot plan: dynamic LDS of the packet kernels, workgroups per CU, and how the resident workgroup slots are split
struct SlotInputs {
  uint32_t num_cus = 0;
  size_t max_lds = 0;
  uint32_t block = 512, blocks_per_cu = 2;       // Tuning
  uint32_t n_lds_models = 0, n_instances = 0, n_groups = 0;
  bool no_lds_boxes = false;
  uint32_t reserve_request = DUST_RESERVE_AUTO;  // Tuning::reserve_blocks
  bool in_collective = false, side_busy = false;
  uint32_t share = 0;                            // percent of the slots a surfel pass on the second stream holds
  uint32_t frames_in_flight = 1, in_flight_slots = DUST_IN_FLIGHT_SHARE, in_flight_oversub = 0;
  uint32_t total_tiles = 0;
};
struct SlotPlan {
  bool too_big = false;      // staged roots and candidate lists exceed the device's LDS (nothing else is filled in)
  size_t lds = 0;            // a `block`-thread workgroup's: roots, a candidate list per wave, the tile queue, the boxes if they ride along
  uint32_t n_lds_boxes = 0, bpc = 0;
  uint32_t resident = 0;     // every slot of every CU, minus the reserve
  uint32_t reserve_blocks = 0, side_slots = 0, main_resident = 0;
  bool share_slots = false;
  uint32_t frame_slots = 0, grid = 0;
};
inline SlotPlan slot_plan(const SlotInputs& in) {
  SlotPlan pl;
  pl.bpc = in.blocks_per_cu;
  pl.lds = size_t(in.n_lds_models) * kN16LdsBytes + (in.block / 64) * (kMaxCand * 8 + 8) + 16;
  if (pl.lds > in.max_lds) { pl.too_big = true; return pl; }
  // the instance boxes ride along when the workgroups of a CU still fit side by side (the packet cull reads all of them, per packet)
  const uint32_t cull_boxes = in.n_groups ? in.n_groups : in.n_instances;  // (a large scene stages the boxes of its groups of 64)
  if (!in.no_lds_boxes && (pl.lds + size_t(cull_boxes) * 32) * pl.bpc <= 160 * 1024 && pl.lds + size_t(cull_boxes) * 32 <= in.max_lds) {
    pl.n_lds_boxes = cull_boxes;
    pl.lds += size_t(cull_boxes) * 32;
  }
  while (pl.bpc > 1 && pl.lds * pl.bpc > 160 * 1024) --pl.bpc;
  // Workgroups per persistent launch: every slot of every CU, minus what the caller asks to be left free. The traversal
  // kernels hold all VGPRs of the SIMDs they run on, so a kernel of another queue (an RCCL send/receive moving the previous
  // frame to another GPU) can only become resident next to them where a workgroup slot was left empty.
  pl.resident = in.num_cus * pl.bpc;
  // (DUST_RESERVE_AUTO: nothing until the pipeline has been seen in a collective of world > 1 -- comm.hip says so --, 32 from then on: without
  //  them RCCL's kernels wait 36 us - 0.2 ms behind a persistent launch, with them under 10 us; they cost the traversal 5 %)
  pl.reserve_blocks = (in.reserve_request == DUST_RESERVE_AUTO ? (in.in_collective ? 32u : 0u) : in.reserve_request) & ~7u;
  if (pl.reserve_blocks && pl.reserve_blocks + 8u <= pl.resident) pl.resident -= pl.reserve_blocks;
  // while a surfel pass may be running on the second stream, the primary / AO kernels leave it its share of the slots (persistent
  // launches hold what they get: whichever came first would otherwise own the GPU until it is done)
  pl.side_slots = in.side_busy ? std::max(8u, (pl.resident * in.share / 100u) & ~7u) : 0u;
  pl.main_resident = std::max(8u, pl.resident - std::min(pl.resident - 8u, pl.side_slots));
  // (a caller with several frames in flight, each on a pipeline of its own: this launch takes its share of the slots -- whole
  // rounds over the 8 XCDs -- and leaves the rest to the others, dust_hip_pipeline_set_frames_in_flight)
  // (DUST_IN_FLIGHT_ALL: every launch asks for all of them -- whole frames one behind the other on two or three streams: the next frame's
  //  workgroups become resident on the CUs the previous frame's last tiles have left)
  pl.share_slots = in.frames_in_flight > 1 && in.in_flight_slots == DUST_IN_FLIGHT_SHARE;
  // (diagnostic IN_FLIGHT_OVERSUB = percent: each of the n launches asks for that much more than its 1/n -- the extra workgroups wait for a slot)
  pl.frame_slots = pl.share_slots ? std::min(pl.main_resident, std::max(8u, ((pl.main_resident / in.frames_in_flight) * (100u + in.in_flight_oversub) / 100u) & ~7u))
                                  : pl.main_resident;
  pl.grid = packet_grid(pl.frame_slots, in.total_tiles);
  return pl;
}
// beside the next frame's kernels the surfel pass takes its share of the workgroup slots (both are persistent launches: with all slots
// taken by the first, the second would simply run after it)
inline uint32_t side_resident(uint32_t resident, uint32_t share) { return std::max(8u, (resident * share / 100u) & ~7u); }

// ---- the fused primary + AO kernel's shape. One 1024-thread workgroup per CU when the kernel has the device to itself (no surfel pass beside it,
// one frame in flight, no slots reserved, the default block size): the roots are staged once per CU and sixteen waves share a tile queue
struct FusedShape { bool too_big = false; uint32_t fblock = 0, fgrid = 0; };
inline FusedShape fused_shape(const SlotInputs& in, const SlotPlan& pl, bool wide_fused, bool wide_share, uint32_t batch_frames) {
  FusedShape f;
  f.fblock = in.block; f.fgrid = pl.grid;
  const size_t batch_lds = 16u * (batch_frames - 1u);   // a tile queue per further frame of the launch
  if (pl.lds + batch_lds > in.max_lds) { f.too_big = true; return f; }
  const size_t lds_wide = size_t(in.n_lds_models) * kN16LdsBytes + 16u * (kMaxCand * 8 + 8) + 16 + size_t(pl.n_lds_boxes) * 32 + batch_lds;
  const bool alone = wide_fused && in.block == 512 && pl.bpc == 2 && !in.side_busy && !pl.reserve_blocks && lds_wide <= in.max_lds;
  if (alone && !pl.share_slots && pl.grid == pl.resident) {
    f.fblock = 1024;
    f.fgrid = packet_grid(in.num_cus, in.total_tiles);
  } else if (alone && wide_share && pl.share_slots && in.frames_in_flight == 2 && pl.grid == pl.frame_slots && pl.frame_slots * 2u == pl.resident) {
    // two whole frames in flight, each on half of the slots: half of the CUs each, one 1024-thread workgroup per CU
    f.fblock = 1024;
    f.fgrid = std::max(8u, (pl.frame_slots / 2u) & ~7u);
  }
  return f;
}

// ---- FNV-1a, and the view key: a hash of what decides a tile's cost -- camera, scene (handle and revision), sky, row band
constexpr uint64_t kFnvOffsetBasis = 14695981039346656037ull, kFnvPrime = 1099511628211ull;
// (where the view key has always begun: the published basis less its last digit. A key is only ever compared with another key of the same
//  process, so any start serves; this one keeps the keys what they were)
constexpr uint64_t kViewKeyBasis = 1469598103934665603ull;
struct Fnv1a {
  uint64_t k = kFnvOffsetBasis;
  void mix(const void* data, size_t n) { const uint8_t* b = static_cast<const uint8_t*>(data); for (size_t i = 0; i < n; ++i) { k ^= b[i]; k *= kFnvPrime; } }
};
inline uint64_t view_key(const DustHipCamera& cam, const void* scene, uint64_t revision, const DustHipSky& sky, uint32_t row_begin, uint32_t row_end) {
  Fnv1a h{kViewKeyBasis};
  h.mix(&cam, sizeof cam); h.mix(&scene, sizeof scene); h.mix(&revision, sizeof revision); h.mix(sky.state, sizeof sky.state);
  h.mix(&row_begin, sizeof row_begin); h.mix(&row_end, sizeof row_end);
  return h.k;
}
// view runs of a launch of n frames (FrameArgs::view_run): the leader says how many frames follow it with the same view, a follower says 0
inline void view_runs(const bool* continues, uint32_t n, uint32_t* view_run) {
  for (uint32_t i = 0; i < n;) {
    uint32_t run = 1;
    while (i + run < n && continues[i + run]) ++run;
    view_run[i] = run;
    for (uint32_t m = 1; m < run; ++m) view_run[i + m] = 0;
    i += run;
  }
}

// ---- which frames' launches are bracketed by event pairs. An event pair around a launch costs the stream ~6 us per record (a marker packet the
// next dispatch waits behind): 5 % of a 0.23 ms frame. A context that only wants averages over a run of frames (bench.py) times every 4th frame's
// launches -- at the same rate PER FRAME as single launches are: a launch of n frames counts as n of the stride.
inline uint32_t timing_stride(uint32_t context_stride, bool batched, uint32_t batch_frames) { return batched ? std::max(1u, context_stride / batch_frames) : context_stride; }
inline bool launch_timed(uint32_t frame_counter, uint32_t stride) { return frame_counter % stride == 0; }

// ---- the tile schedule: per pass kind, what the launch about to be made does about its cost-ordered hand-out (kernels.hip, k_tile_order).
// Orders the tiles by what the pass's previous launch measured, if that was on the same tile grid, and has this launch measure again.
// While the view stands still (same camera, scene revision, sun and rows) the costs do too: the order is kept and re-measured
// only every kOrderRefresh launches, which takes k_tile_order (~8 us) and the cost recording out of most frames.
// An order that a re-measurement of the same view has just confirmed is trusted for twice as long, up to 64 launches (the GI
// kernels' costs drift as the hash fills: they keep being looked at).
constexpr uint32_t kOrderRefresh = 8, kOrderRefreshMax = 64;
struct TileState {
  uint32_t tiles_x = 0, tiles_y = 0, capacity = 0, age = 0;
  uint32_t refresh = kOrderRefresh;  // launches between two measurements of a view that stands still (doubling up to kOrderRefreshMax)
  uint64_t view = 0;       // view_key() of the launch the costs / the order were taken under
  bool recorded = false;   // cost[] holds the previous launch's measurements
  bool ordered = false;    // order[] is a valid permutation of this tile grid
  bool measured = false;   // cost[] holds a launch's measurements (maybe not the last launch's)
  bool moving = false;     // the previous launch's view differed from the one before it
  uint32_t cuts_age = 0;   // re-orderings since cuts[] was worked out
};
struct TileTuning { bool no_tile_order, equal_bands, dilate, force_moving; uint32_t cuts_reuse, moving_refresh, still_refresh_max; };  // (Tuning's)
struct TileStep {          // in the order they are carried out
  bool allocate = false;   // the buffers are too small for this grid
  bool reset = false;      // a new grid: tiles nobody has timed count as free (cost and smooth zeroed)
  bool blend = false;      // the previous launch measured: blend its costs into the running means and re-order ...
  bool dilate = false;     // ... by each tile's estimate or its dearest neighbour's
  bool reuse_cuts = false; // ... keeping the band cuts
  bool hand_order = false, hand_cuts = false;  // the launch gets order[] / cuts[]
  bool measure = false;    // the launch records its tiles' costs: the next one re-orders
  uint32_t total = 0, per_band = 0;
};
inline TileStep tile_step(TileState& h, uint32_t tiles_x, uint32_t tiles_y, uint64_t view, const TileTuning& t) {
  TileStep d;
  if (t.no_tile_order) return d;
  d.total = tiles_x * tiles_y;
  d.per_band = (d.total + kRegions - 1) / kRegions;
  if (d.per_band > kTileOrderMaxBand) return d;  // beyond 8K: screen order
  if (d.total > h.capacity) { d.allocate = true; h.capacity = d.total; h.tiles_x = h.tiles_y = 0; }
  if (h.tiles_x != tiles_x || h.tiles_y != tiles_y) {
    d.reset = true;
    h.recorded = false; h.ordered = false; h.measured = false; h.tiles_x = tiles_x; h.tiles_y = tiles_y;
  }
  if (h.recorded) {
    // (the cost-balanced cuts drift slowly: a view that moves keeps them for kCutsReuse re-orderings -- the scan for them is the longer half of the sorter)
    d.reuse_cuts = h.ordered && h.cuts_age + 1 < t.cuts_reuse && h.moving;
    d.blend = true;
    d.dilate = h.moving && t.dilate && tiles_y > 1u;
    h.cuts_age = d.reuse_cuts ? h.cuts_age + 1 : 0;
    h.recorded = false; h.ordered = true; h.age = 0;
  } else if (h.ordered) {
    ++h.age;
  }
  d.hand_order = h.ordered;
  d.hand_cuts = h.ordered && !t.equal_bands;
  const bool still = h.ordered && h.view == view && !t.force_moving;
  if (!still) h.refresh = kOrderRefresh;
  // A view that moves: tile costs shift by a fraction of a tile per frame, so the order of a few frames ago is still a good one -- it is
  // re-measured (and the next launch re-ordered) every kMovingRefresh launches, not every launch: the sorter is a launch of its own
  // between two frames (~10 us of a 230 us frame). The first launch after a standstill (a cut, a teleport) is measured at once.
  const bool jumped = !still && !h.moving;
  const uint32_t period = still ? std::min(h.refresh, t.still_refresh_max) : t.moving_refresh;
  if (!h.ordered || jumped || h.age + 1 >= period) {  // measure this launch (each traced tile overwrites its cost): the next one re-orders
    d.measure = true;
    h.recorded = true; h.measured = true;
    if (still) h.refresh = std::min(kOrderRefreshMax, h.refresh * 2u);
  }
  h.moving = !still && h.measured && h.view != 0 && (h.view != view || t.force_moving);  // (the first launch of a view that stands still is not a moving one;
                                                                                         //  DUST_HIP_FORCE_MOVING: a still view on a moving view's schedule)
  h.view = view;
  return d;
}

// ---- a sharded surfel trace (DustHipFrameParams::surfel_world >= 1): rank's share of the ordered pool, in groups of 64 slots
struct ShardRange {
  uint32_t groups, per;   // groups of the pool, groups per rank
  size_t cap;             // staging slots: room for any world up to 64 (a rank's share ends on a group boundary)
  uint32_t group_begin, group_count, slots_per_rank;   // (a rank past the end of the pool traces nothing)
};
inline ShardRange shard_range(uint32_t pool_size, uint32_t rank, uint32_t world) {
  ShardRange r;
  r.groups = (pool_size + 63u) / 64u; r.per = (r.groups + world - 1u) / world;
  r.cap = size_t(r.groups + 64u) * 64u;
  r.group_begin = std::min(r.groups, rank * r.per);
  r.group_count = std::min(r.per, r.groups - r.group_begin);
  r.slots_per_rank = r.per * 64u;
  return r;
}
// key bits of the ordered apply's sort by hash location: locations 0 .. capacity (capacity itself = "no insert")
inline uint32_t apply_key_bits(uint32_t capacity) {
  uint32_t bits = 1;
  while ((1ull << bits) <= uint64_t(capacity)) ++bits;
  return bits;
}

}  // namespace dust
