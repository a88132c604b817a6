// kernels.hip -- CDNA4 (gfx950) kernels of the primary and ambient-occlusion passes, the frame post-passes (accumulate, auto
// exposure, tone map), the cost-ordered work distribution's sorter and the device-function evaluator. The traversal code
// they are made of is traverse.hpp; the final gather and surfel passes are gi.hip.
#include "traverse.hpp"

namespace dust {

// ==================================================================== primary visibility
// primary.rgen:8-22 + hit.rint + hit.rchit:16-95 + miss.rmiss:7-17 for one packet. Returns, per lane, what the later
// passes read back from the G-buffer: the hit distance (INFINITY on a miss) and the packed normal texel.
// (primary_shade -- hit.rchit + miss.rmiss for one packet -- lives in traverse.hpp)
template <int MODE>
__device__ __forceinline__ void primary_packet(ArgsRef a, const Packet& p, uint32_t* cand, LaneStats& st,
                                               bool store_illuminance, float& hitT, uint32_t& normal_packed) {
  const V3 o = mk(a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]);
  const V3 d = camera_ray_dir(a, p.px, p.py);
  const uint32_t ncand = (a.debug & 2u) ? 0u : cull_instances<MODE>(a, __any(p.valid), point_range(o), wave_range(p.valid, d), a.cam.far_, cand);
  Hit h;
  h.found = false;
  if (!(a.debug & 1u)) trace_ray<0, MODE>(a, p.valid, o, d, a.cam.near_, a.cam.far_, false, cand, ncand, h, st);
  __builtin_amdgcn_wave_barrier();
  PROF_ENTER(P_PRIMARY_SHADE);
  primary_shade<MODE>(reload_args(a), p, o, d, h, store_illuminance, hitT, normal_packed);
  PROF_LEAVE(P_PRIMARY_SHADE);
}
// ==================================================================== sun shadow + ambient occlusion
// ambient_occlusion.rgen:14-66 + .rint + .rchit + .rmiss + nee.rmiss:11-22 for one packet.
// hitT / normal_packed / payload are what the raygen shader loads from img_depth / img_normal / img_illuminance.
template <int MODE>
__device__ __forceinline__ void ao_packet(ArgsRef a, const Packet& p, uint32_t* cand, LaneStats& st_sun, LaneStats& st_ao,
                                          float hitT, uint32_t normal_packed, V3 payload) {
  PROF_ENTER(P_AO_SETUP);
  const V3 sun = mk(a.sky[48], a.sky[49], a.sky[50]);
  const size_t pix = p.valid ? (size_t)p.py * a.width + p.px : 0;
  const bool live = p.valid && !(hitT == INFINITY);
  V3 n = mk(0, 0, 1), loc = mk(0, 0, 0), ad = mk(0, 0, 1);
  if (live) {
    n = nrd_unpack_normal(normal_packed);
    const V3 d = camera_ray_dir(a, p.px, p.py);
    loc = mk((hitT * d.x + a.cam.pos[0]) + n.x * 0.01f, (hitT * d.y + a.cam.pos[1]) + n.y * 0.01f,
             (hitT * d.z + a.cam.pos[2]) + n.z * 0.01f);
    const uint32_t nx = (p.px + 7u + a.rand) % 128u, ny = (p.py + 183u + a.rand) % 128u;
    const uint32_t tex = ((DUST_RO(uint32_t))a.noise5)[ny * 128u + nx];
    V3 ns = mk(div_const((float)(tex & 255u), 255.0f) * 2.0f - 1.0f, div_const((float)((tex >> 8) & 255u), 255.0f) * 2.0f - 1.0f,
               div_const((float)((tex >> 16) & 255u), 255.0f) * 2.0f - 1.0f);
    ad = normalize3(rotate_by_normal(n, ns));
  }
  // two rays per pixel through the same code: k = 0 the sun shadow ray (any-hit, ambient_occlusion.rgen:33-50),
  // k = 1 the ambient occlusion ray (closest hit within 8 units, ambient_occlusion.rgen:52-65)
  const bool sun_live = live && dot3(sun, n) > 0.0f;
  const V3 sd = mk(a.sun_dir[0], a.sun_dir[1], a.sun_dir[2]);  // normalize(sun)
  const Range3 org = wave_range(live, loc);  // both rays leave from the same points (sun_live is a subset of live)
  PROF_LEAVE(P_AO_SETUP);
  Hit h;
#pragma unroll 1
  for (int k = 0; k < 2; ++k) {
#ifdef DUST_SKIP_SUN   // (never shipped: timing builds that leave a ray kind out -- make VARIANT=nosun EXTRA=-DDUST_SKIP_SUN, tools/diag/kinds.py)
    if (k == 0) continue;
#endif
#ifdef DUST_SKIP_AO
    if (k == 1) { h.found = false; h.t = 0.0f; continue; }
#endif
    ArgsRef b = reload_args(a);
    const bool act = k == 0 ? sun_live : live;
    const V3 dir = k == 0 ? sd : ad;
    const float tmax = k == 0 ? 10000.0f : 8.0f;
    const uint32_t ncand = cull_instances<MODE>(b, __any(act), org, k == 0 ? point_range(sd) : wave_range(live, ad), tmax, cand);
    LaneStats cur = {0, 0, 0, 0, 0, 0};
    trace_ray<1, MODE>(b, act, loc, dir, 0.1f, tmax, k == 0, cand, ncand, h, cur);
    if (COUNT) add_stats(k == 0 ? st_sun : st_ao, cur);
    __builtin_amdgcn_wave_barrier();
    if (k == 0 && sun_live && !h.found) {  // final_gather/nee.rmiss:11-22; sun_term = sun radiance x (1 - cos(solar radius))
      const float dn = dot3(n, sd);
      payload.x += b.sun_term[0] * dn; payload.y += b.sun_term[1] * dn; payload.z += b.sun_term[2] * dn;
    }
  }
  if (live) store_radiance(reload_args(a).g.illuminance, pix, payload, h.found ? h.t : 0.0f);
}

#ifdef DUST_WALK_PROBE
// (never shipped: the walk-only kernel the round-4 review asked to have MEASURED -- make VARIANT=wp5 EXTRA="-DDUST_WALK_PROBE -DDUST_WP_T=640
// -DDUST_WP_W=5 -DDUST_MAX_BLOCK=1024u", tools/diag/walk_probe.py. k_primary without its shading: cull + trace of the camera rays, a 16-byte hit
// record per pixel into the accumulation plane (which a primary-only frame does not touch), at the launch bounds given; DUST_WALK_PROBE=2
// adds k_shade_probe, a thread per pixel at full occupancy that turns the records into the G-buffer planes with primary_shade.)
#ifndef DUST_WP_T
#define DUST_WP_T 512
#define DUST_WP_W 4
#endif
template <int MODE>
__global__ void __launch_bounds__(DUST_WP_T, DUST_WP_W) k_primary(const FrameArgs) {
  ArgsRef a0 = launch_args();
  stage_roots(a0);
  uint32_t* cand = wave_cand_list(a0);
  LaneStats st = {0, 0, 0, 0, 0, 0};
  WorkCursor wc = cursor_begin();
  Packet p;
  while (next_packet(a0, wc, p)) {
    ArgsRef a = reload_args(a0);
    const V3 o = mk(a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]);
    const V3 d = camera_ray_dir(a, p.px, p.py);
    const uint32_t ncand = cull_instances<MODE>(a, __any(p.valid), point_range(o), wave_range(p.valid, d), a.cam.far_, cand);
    Hit h;
    h.found = false;
    trace_ray<0, MODE>(a, p.valid, o, d, a.cam.near_, a.cam.far_, false, cand, ncand, h, st);
    if (p.valid) {
      ArgsRef b = reload_args(a0);
      u32x4 r;
      r.x = h.found ? __float_as_uint(h.t) : 0x7F800000u; r.y = h.inst | (h.voxel << 16); r.z = h.block; r.w = h.found ? 1u : 0u;
      DUST_NT_STORE(r, (DUST_GLOBAL_AS u32x4*)b.g.accum + ((size_t)p.py * b.width + p.px));
    }
  }
  prof_end();
  flush_stats<MODE>(a0, 0, st);
}
template <int MODE>
__global__ void __launch_bounds__(256) k_shade_probe(const FrameArgs) {
  ArgsRef a = launch_args();
  // 8x8 pixel blocks per wave, like the packets (the hit-lane waterfall of primary_shade wants few distinct instances per wave)
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
  if (wave >= a.tiles_x * a.tiles_y) return;
  const uint32_t ty = wave / a.tiles_x, tx = wave - ty * a.tiles_x;
  Packet p;
  p.px = tx * kTileW + (lane % kTileW); p.py = a.row_begin + ty * kTileH + (lane / kTileW);
  p.valid = p.px < a.width && p.py < a.row_end;
  Hit h;
  h.found = false; h.t = 0.0f; h.inst = 0; h.block = 0; h.voxel = 0;
  if (p.valid) {
    const u32x4 r = *((const DUST_GLOBAL_AS u32x4*)a.g.accum + ((size_t)p.py * a.width + p.px));
    h.t = __uint_as_float(r.x); h.inst = r.y & 0xFFFFu; h.voxel = r.y >> 16; h.block = r.z; h.found = r.w != 0u;
  }
  float hitT;
  uint32_t npk;
  primary_shade<MODE>(a, p, mk(a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]), camera_ray_dir(a, p.px, p.py), h, true, hitT, npk);
}
#else
template <int MODE>
__global__ void __launch_bounds__(512, 4) k_primary(const FrameArgs) {
  ArgsRef a0 = launch_args();
  stage_roots(a0);
  uint32_t* cand = wave_cand_list(a0);
  LaneStats st = {0, 0, 0, 0, 0, 0};
  WorkCursor wc = cursor_begin();
  Packet p;
  while (next_packet(a0, wc, p)) {
    ArgsRef a = reload_args(a0);  // per packet: nothing of the descriptor rides in SGPRs from one packet to the next
    float hitT;
    uint32_t npk;
    primary_packet<MODE>(a, p, cand, st, true, hitT, npk);
  }
  prof_end();
  flush_stats<MODE>(a0, 0, st);
}
#endif

template <int MODE>
__global__ void __launch_bounds__(512, 4) k_ambient_occlusion(const FrameArgs) {
  ArgsRef a0 = launch_args();
  stage_roots(a0);
  uint32_t* cand = wave_cand_list(a0);
  LaneStats st_sun = {0, 0, 0, 0, 0, 0}, st_ao = {0, 0, 0, 0, 0, 0};
  WorkCursor wc = cursor_begin();
  Packet p;
  while (next_packet(a0, wc, p)) {
    ArgsRef a = reload_args(a0);  // per packet: nothing of the descriptor rides in SGPRs from one packet to the next
    const size_t pix = p.valid ? (size_t)p.py * a.width + p.px : 0;
    const float hitT = p.valid ? a.g.depth[pix] : INFINITY;
    uint32_t npk = 0;
    V3 payload = mk(0, 0, 0);
    if (p.valid && !(hitT == INFINITY)) {
      npk = a.g.normal[pix];
      float w;
      payload = load_radiance(a.g.illuminance, pix, w);
    }
    ao_packet<MODE>(a, p, cand, st_sun, st_ao, hitT, npk, payload);
  }
  prof_end();
  flush_stats<MODE>(a0, 0, st_sun);
  flush_stats<MODE>(a0, 1, st_ao);
}

// Fused primary + ambient occlusion passes: a pixel's AO pass reads only that pixel's own primary outputs, so the
// wave that traced a packet's primary rays goes straight on to its shadow and AO rays with depth and normal still
// in registers (as the quantised values the separate pass would load back). One launch, one LDS staging and one
// work queue instead of two; the G-buffer contents are bit-identical to running the two kernels.
// The fused kernel may be launched as ONE 1024-thread workgroup per CU instead of two of 512 (capi.cpp, render_frame): the same
// 4 waves per SIMD, but the roots are staged once per CU instead of twice and sixteen waves share a tile queue (-1 %).
#ifndef DUST_PAO_THREADS
#define DUST_PAO_THREADS 1024
#define DUST_PAO_WAVES 4
#endif
template <int MODE>
__global__ void __launch_bounds__(DUST_PAO_THREADS, DUST_PAO_WAVES) k_primary_ao(const FrameArgs) {
  ArgsRef a0 = launch_args();
#ifdef DUST_WAVE_TIMES
  const unsigned long long wt0 = __builtin_amdgcn_s_memtime(), ww0 = wall_clock64();
  unsigned long long wt_tiles = 0, wt_last_tile = 0, wt_last_start = 0, wt_prev_tile = 0, wt_prev_start = 0;
#endif
  stage_roots(a0);
#ifdef DUST_WAVE_TIMES
  const unsigned long long wt1 = __builtin_amdgcn_s_memtime();
#endif
  uint32_t* cand = wave_cand_list(a0);
  LaneStats st = {0, 0, 0, 0, 0, 0}, st_sun = {0, 0, 0, 0, 0, 0}, st_ao = {0, 0, 0, 0, 0, 0};
  WorkCursor wc = cursor_begin();
  Packet p;
  while (next_packet(a0, wc, p)) {
    float hitT;
    uint32_t npk;
#ifdef DUST_WAVE_TIMES
    wt_tiles += 1;
    wt_prev_tile = wt_last_tile; wt_prev_start = wt_last_start;
    wt_last_tile = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)p.py) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)p.px);
    wt_last_start = wall_clock64();
#endif
    primary_packet<MODE>(reload_args(a0), p, cand, st, false, hitT, npk);
    ao_packet<MODE>(reload_args(a0), p, cand, st_sun, st_ao, hitT, npk, mk(0, 0, 0));  // unpack(0,0,0,0) == (0,0,0)
  }
#ifdef DUST_WAVE_TIMES
  if ((threadIdx.x & 63u) == 0) {
    const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w < 8192u) {
      g_wave_times[w][0] = wt0; g_wave_times[w][1] = wt1; g_wave_times[w][2] = __builtin_amdgcn_s_memtime();
      g_wave_times[w][3] = ww0; g_wave_times[w][4] = wall_clock64(); g_wave_times[w][5] = wt_tiles;
      g_wave_times[w][6] = wt_last_tile; g_wave_times[w][7] = wt_last_start; g_wave_times[w][8] = wt_prev_tile; g_wave_times[w][9] = wt_prev_start;
      if (w == 0u) {
        const uint32_t slot = a0.frame_index & 255u;
        g_launch_clock[slot][0] = g_wave_times[w][2] - wt0; g_launch_clock[slot][1] = g_wave_times[w][4] - ww0; g_launch_clock[slot][2] = a0.frame_index;
      }
    }
  }
#endif
  prof_end();
  flush_stats<MODE>(a0, 0, st);
  flush_stats<MODE>(a0, 1, st_sun);
  flush_stats<MODE>(a0, 2, st_ao);
}

// Several frames in ONE persistent launch (dust_hip_render_frames): the kernel argument is a BatchArgs, `batch_frames` whole launch
// descriptors side by side. The frames share what is staged in LDS (one scene) and the launch geometry; a wave that finds frame f without
// tiles -- its own band's; in the last frame the others' too -- takes the next frame's descriptor and queue and goes on, so the launch has ONE tail (waves idle
// behind the last long tiles), one staging of the roots and one inter-launch gap for all of its frames: the per-launch costs that are what
// is left of the 1080p frame (4 % + 1 % + 1.9 %). Each frame writes the planes of ITS pipeline with the bits the single-frame
// kernel writes (same packets, same arithmetic; tests/test_gpu_batch.py). The reference keeps up to three frames in flight
// (rhyolite_bevy/src/lib.rs:58); the GI passes cannot ride along: a frame's gather reads the hash its predecessor's surfel pass wrote.
// Frames after the first are not dealt a first round (launch_primary_ao_batch): their waves arrive one by one and take the most expensive
// tiles left, in order. The frames may read different images of the scene's ring (an instance moved between them): what is staged in LDS
// is frame 0's, and a frame of another image has n_lds_boxes = 0 (its boxes come from memory).
template <int MODE>
__global__ void __launch_bounds__(DUST_PAO_THREADS, DUST_PAO_WAVES) k_primary_ao_batch(const BatchArgs) {
  ArgsRef lead = launch_args();
#ifdef DUST_WAVE_TIMES   // (tools/wave_times.py --frames-per-launch: when the launch's waves start, get past staging and run out of tiles)
  const unsigned long long wt0 = __builtin_amdgcn_s_memtime(), ww0 = wall_clock64();
  unsigned long long wt_tiles = 0;
#endif
  stage_roots_of<true>(lead);
#ifdef DUST_WAVE_TIMES
  const unsigned long long wt1 = __builtin_amdgcn_s_memtime();
#endif
  uint32_t* cand = wave_cand_list(lead);
  LaneStats st = {0, 0, 0, 0, 0, 0}, st_sun = {0, 0, 0, 0, 0, 0}, st_ao = {0, 0, 0, 0, 0, 0};  // (never a counting build: dead)
  const uint32_t n_frames = lead.batch_frames;
#pragma unroll 1
  for (uint32_t f = 0; f < n_frames; ++f) {
    const DUST_CONST_AS FrameArgs* fq = &launch_args() + f;
    asm volatile("" : "+s"(fq));
    ArgsRef a0 = *fq;
    // (frame 0's set was zeroed by stage_roots; nobody reads these before the next launch of that pipeline, stream-ordered behind this one)
    if (f != 0u && blockIdx.x == 0 && threadIdx.x < kRegions) a0.next_work_counters[threadIdx.x * kCounterStride] = 0u;
    WorkCursor wc = cursor_begin();
    wc.frame = f;
    wc.grab = a0.batch_grab;
    // Before the launch's last frame a workgroup stays on its OWN band -- its XCD's L2 -- and goes on to the next frame when that is handed out:
    // the band's last tiles are its own workgroups' business, nobody waits for a frame in the middle of a launch, and the up to seven refused
    // atomics on the other bands' counters per workgroup and frame are not paid (8 frames per launch: 1.6653 -> 1.6574 ms). The last frame is
    // finished by whoever is free, as a single frame is.
    wc.tries = f + 1u == n_frames ? kRegions : 1u;
    Packet p;
    while (next_packet_of<true>(a0, wc, p)) {
      float hitT;
      uint32_t npk;
#ifdef DUST_WAVE_TIMES
      wt_tiles += 1;
#endif
      primary_packet<MODE>(reload_args(a0), p, cand, st, false, hitT, npk);
      ao_packet<MODE>(reload_args(a0), p, cand, st_sun, st_ao, hitT, npk, mk(0, 0, 0));
    }
  }
#ifdef DUST_WAVE_TIMES
  if ((threadIdx.x & 63u) == 0) {
    const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w < 8192u) {
      g_wave_times[w][0] = wt0; g_wave_times[w][1] = wt1; g_wave_times[w][2] = __builtin_amdgcn_s_memtime();
      g_wave_times[w][3] = ww0; g_wave_times[w][4] = wall_clock64(); g_wave_times[w][5] = wt_tiles;
      for (int k = 6; k < 12; ++k) g_wave_times[w][k] = 0;
    }
  }
#endif
  prof_end();
}

// View runs (dust_dev.h, FrameArgs::view_run): consecutive frames of a launch with the same camera, sky and scene image. Everything but the AO ray
// is the same for all of them, bit for bit -- the camera ray's cull, walk and shading, the sun ray's cull and walk and what it adds to the payload --, so
// a tile is ONE work item for the whole run: the leader's descriptor traces the camera and sun rays once, every member's planes get the texels, and
// only the AO ray (its direction reads the member's rand and noise slice) is traced per member. primary_packet + ao_packet, regrouped:
//   camera ray, primary_shade<KEEP>  ->  for each member: its G-buffer texels  ->  sun ray  ->  for each member: AO ray, its illuminance texel.
// The static texels wait in registers only from primary_shade to the member loop right behind it (six VGPRs, nothing of a trace is live there): the
// stores stand outside primary_shade's one-instance-at-a-time loop, and no trace carries them.
// The sun ray and the members' AO rays go through ONE trace_ray<1> (k = 0: sun, k = 1 + m: member m), as ao_packet's two rays do.
template <int MODE>
__device__ __forceinline__ void view_run_packet(ArgsRef a, const DUST_CONST_AS FrameArgs* members, uint32_t run, const Packet& p, uint32_t* cand, LaneStats& st) {
  float hitT;
  uint32_t normal_packed;
  {
    const V3 o = mk(a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]);
    const V3 d = camera_ray_dir(a, p.px, p.py);
    const uint32_t ncand = (a.debug & 2u) ? 0u : cull_instances<MODE>(a, __any(p.valid), point_range(o), wave_range(p.valid, d), a.cam.far_, cand);
    Hit h;
    h.found = false;
    if (!(a.debug & 1u)) trace_ray<0, MODE>(a, p.valid, o, d, a.cam.near_, a.cam.far_, false, cand, ncand, h, st);
    __builtin_amdgcn_wave_barrier();
    PROF_ENTER(P_PRIMARY_SHADE);
    PrimaryTexels tx;
    primary_shade<MODE, true>(reload_args(a), p, o, d, h, false, hitT, normal_packed, &tx);
#pragma unroll 1
    for (uint32_t m = 0; m < run; ++m) {
      const DUST_CONST_AS FrameArgs* mq = members + (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
      asm volatile("" : "+s"(mq));
      store_primary_texels(*mq, p, hitT, normal_packed, tx);
    }
    PROF_LEAVE(P_PRIMARY_SHADE);
  }
  PROF_ENTER(P_AO_SETUP);
  ArgsRef a1 = reload_args(a);
  const V3 sun = mk(a1.sky[48], a1.sky[49], a1.sky[50]);
  const size_t pix = p.valid ? (size_t)p.py * a1.width + p.px : 0;
  const bool live = p.valid && !(hitT == INFINITY);
  V3 n = mk(0, 0, 1), loc = mk(0, 0, 0);
  if (live) {
    n = nrd_unpack_normal(normal_packed);
    const V3 d = camera_ray_dir(a1, p.px, p.py);
    loc = mk((hitT * d.x + a1.cam.pos[0]) + n.x * 0.01f, (hitT * d.y + a1.cam.pos[1]) + n.y * 0.01f,
             (hitT * d.z + a1.cam.pos[2]) + n.z * 0.01f);
  }
  const bool sun_live = live && dot3(sun, n) > 0.0f;
  const V3 sd = mk(a1.sun_dir[0], a1.sun_dir[1], a1.sun_dir[2]);
  const Range3 org = wave_range(live, loc);
  V3 payload = mk(0, 0, 0);
  PROF_LEAVE(P_AO_SETUP);
  // ONE AO cull per tile and run. The members' AO rays leave from the same points (org) with the same reach (8) and differ only in direction, so the
  // list is built once, at k = 1, for EVERY unit direction: the cube [-1, 1]^3 widened by a hair (normalize3's components end within 3 ulp of
  // [-1, 1]: three roundings in the dot product, halved by the root, one in the root, one in the division; 1.000001f is 1 + 8 ulp), which leaves of
  // cull_instances' test "the box lies within Chebyshev distance 8 of the box of the tile's hit points". A superset of every member's own list with
  // entry times no later than the member's own, so trace_ray's walk and its early exit stay conservative and the texels are what they were (the order
  // of a list decides the work, not the hit). 64 cosine directions already fill most of the cube: the lists are hardly longer than a member's own.
  // Nothing between two members' traces writes the wave's list, the sort staging or a LARGE scene's group mask behind it: cull_instances is their
  // only writer, trace_ray takes them as const, and the wave takes no new tile (next_packet, the tile accounts) before the loop is done.
  Range3 cube;
#pragma unroll
  for (int q = 0; q < 3; ++q) { cube.lo[q] = -1.000001f; cube.hi[q] = 1.000001f; }
  // ONE set-up per tile when that list holds one candidate -- the common tile: the instance its pixels hit. Which instance that is and where its
  // record lies are the same for every member, so they are worked out here, once, and trace_run_ray takes them instead of reading the list: per
  // member that leaves the direction, its reciprocals, the object-space ray, the world-box slab with the entry-time limit -- the tests that decide
  // WHICH lanes enter stay per ray, bit for bit -- and trace_instance. Lists of two or more, lists that overflow and debug bit 4 walk the list as
  // before; debug bit 64 sends every tile that way (tests, A/B in one binary). (The origins in object space, xform_point(w2o, loc), are the same
  // for every member too; kept across the members' walks they cost 3 to 11 VGPR spills per variant and measured +1 %: they are worked out per member.)
  TileVisit tv;
  tv.v = nullptr; tv.inst = 0;
  Hit h;
  uint32_t ncand = 0;
#pragma unroll 1
  for (uint32_t k = 0; k <= run; ++k) {
    ArgsRef b = reload_args(a);
    const DUST_CONST_AS FrameArgs* mq = members + (uint32_t)__builtin_amdgcn_readfirstlane((int)(k ? k - 1u : 0u));   // the member whose AO ray this is (k = 0, the sun ray: nobody's)
    asm volatile("" : "+s"(mq));
    const bool act = k == 0u ? sun_live : live;
    const float tmax = k == 0u ? 10000.0f : 8.0f;
    if (k <= 1u) ncand = cull_instances<MODE>(b, __any(act), org, k == 0u ? point_range(sd) : cube, tmax, cand);   // k >= 2: member 0's list
    if (k == 1u && (uint32_t)__builtin_amdgcn_readfirstlane((int)ncand) == 1u && !(b.debug & (4u | 64u))) {   // (the cull ends behind a fence and a wave barrier: cand[0] is there)
      tv.inst = (uint32_t)__builtin_amdgcn_readfirstlane((int)cand[0]) & 0xFFFFu;
      tv.v = &b.visits[tv.inst];
    }
    V3 ad = mk(0, 0, 1);
    PROF_ENTER_IF(k != 0u, P_M_DIR);
    if (k != 0u && live) {  // ambient_occlusion.rgen:52-58 with the member's frame index: its noise slice and rand
      const uint32_t nx = (p.px + 7u + mq->rand) % 128u, ny = (p.py + 183u + mq->rand) % 128u;
      const uint32_t tex = ((DUST_RO(uint32_t))mq->noise5)[ny * 128u + nx];
      V3 ns = mk(div_const((float)(tex & 255u), 255.0f) * 2.0f - 1.0f, div_const((float)((tex >> 8) & 255u), 255.0f) * 2.0f - 1.0f,
                 div_const((float)((tex >> 16) & 255u), 255.0f) * 2.0f - 1.0f);
      ad = normalize3(rotate_by_normal(n, ns));
    }
    PROF_LEAVE_IF(k != 0u, P_M_DIR);
    const V3 dir = k == 0u ? sd : ad;
    LaneStats cur = {0, 0, 0, 0, 0, 0};
    trace_run_ray<MODE>(b, act, loc, dir, 0.1f, tmax, k == 0u, cand, ncand, tv, h, cur);
    __builtin_amdgcn_wave_barrier();
    if (k == 0u && sun_live && !h.found) {
      const float dn = dot3(n, sd);
      payload.x += b.sun_term[0] * dn; payload.y += b.sun_term[1] * dn; payload.z += b.sun_term[2] * dn;
    }
    PROF_ENTER_IF(k != 0u, P_M_STORE);
    if (k != 0u && live) store_radiance(mq->g.illuminance, pix, payload, h.found ? h.t : 0.0f);
    PROF_LEAVE_IF(k != 0u, P_M_STORE);
  }
}
// k_primary_ao_batch over view runs instead of frames (launch_primary_ao_batch launches it when a run of the launch is longer than one frame). A run
// takes its LEADER's tile queue, tile order, band cuts, cost buffer and work counters -- the followers' are not read --; the next launch's counters
// are zeroed for every member, as k_primary_ao_batch does for every frame. A run of one frame is what a frame is there; the rules of the launch's
// last frame (every band, refills of kGrabBatch) are those of its last RUN.
template <int MODE>
__global__ void __launch_bounds__(DUST_PAO_THREADS, DUST_PAO_WAVES) k_primary_ao_runs(const BatchArgs) {
  ArgsRef lead = launch_args();
#ifdef DUST_WAVE_TIMES
  const unsigned long long wt0 = __builtin_amdgcn_s_memtime(), ww0 = wall_clock64();
  unsigned long long wt_tiles = 0;
#endif
  stage_roots_of<true>(lead);
#ifdef DUST_WAVE_TIMES
  const unsigned long long wt1 = __builtin_amdgcn_s_memtime();
#endif
  uint32_t* cand = wave_cand_list(lead);
  LaneStats st = {0, 0, 0, 0, 0, 0};  // (never a counting build: dead)
  const uint32_t n_frames = lead.batch_frames;
#pragma unroll 1
  for (uint32_t f = 0; f < n_frames;) {
    const DUST_CONST_AS FrameArgs* fq = &launch_args() + f;
    asm volatile("" : "+s"(fq));
    ArgsRef a0 = *fq;
    uint32_t run = a0.view_run ? a0.view_run : 1u;
    if (run > n_frames - f) run = n_frames - f;   // (the launcher checks the runs against the frame count: a run never leaves the BatchArgs)
    if (blockIdx.x == 0 && threadIdx.x < kRegions)
      for (uint32_t m = f ? 0u : 1u; m < run; ++m) fq[m].next_work_counters[threadIdx.x * kCounterStride] = 0u;   // (frame 0's: stage_roots)
    WorkCursor wc = cursor_begin();
    wc.frame = f;
    wc.grab = a0.batch_grab;
    wc.tries = f + run == n_frames ? kRegions : 1u;
    Packet p;
    while (next_packet_of<true>(a0, wc, p)) {
#ifdef DUST_WAVE_TIMES
      wt_tiles += 1;
#endif
      view_run_packet<MODE>(reload_args(a0), fq, run, p, cand, st);
    }
    f += run;
  }
#ifdef DUST_WAVE_TIMES
  if ((threadIdx.x & 63u) == 0) {
    const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w < 8192u) {
      g_wave_times[w][0] = wt0; g_wave_times[w][1] = wt1; g_wave_times[w][2] = __builtin_amdgcn_s_memtime();
      g_wave_times[w][3] = ww0; g_wave_times[w][4] = wall_clock64(); g_wave_times[w][5] = wt_tiles;
      for (int k = 6; k < 12; ++k) g_wave_times[w][k] = 0;
    }
  }
#endif
  prof_end();
}

// ==================================================================== N-frame mean (stands in for NRD)
__global__ void k_accumulate(const FrameArgs) {
  ArgsRef a = launch_args();
  const uint32_t rows = a.row_end - a.row_begin;
  const size_t n = (size_t)rows * a.width;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = (size_t)a.row_begin * a.width + i;
    float w;
    const bool miss = a.g.depth[pix] == INFINITY;
    const V3 r = load_radiance(miss ? a.g.denoised : a.g.illuminance, pix, w);  // miss.rmiss writes the denoised target
    f32x4 acc = ((DUST_GLOBAL_AS f32x4*)a.g.accum)[pix];
    const float k = 1.0f / (float)(a.accum_count + 1u);
    if (a.accum_count == 0u) acc = f32x4{0.f, 0.f, 0.f, 0.f};
    acc.x += (r.x - acc.x) * k; acc.y += (r.y - acc.y) * k; acc.z += (r.z - acc.z) * k;
    acc.w = (float)(a.accum_count + 1u);
    ((DUST_GLOBAL_AS f32x4*)a.g.accum)[pix] = acc;
    // what the denoiser would hand to auto exposure / tone mapping (img_illuminance_denoised, packed YCoCg);
    // miss pixels already carry the sky there (miss.rmiss:13)
    if (!miss) store_radiance(a.g.denoised, pix, mk(acc.x, acc.y, acc.z), w);
  }
}

// ==================================================================== auto exposure + tone map
// auto_exposure.comp:20-74: 256-bin log2-luminance histogram of the (packed YCoCg) radiance image
__global__ void __launch_bounds__(256) k_exposure_histogram(const uint16_t* __restrict__ src, uint32_t n_pixels, float min_log,
                                                            float log_range, uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[256];
  bins[threadIdx.x] = 0;
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pixels; i += (size_t)gridDim.x * blockDim.x) {
    float w;
    const V3 c = load_radiance(src, i, w);
    const float lum = (c.x * 0.299f + c.y * 0.587f) + c.z * 0.114f;
    uint32_t bin = 0;
    if (!(lum < 0.005f)) {
      const float logLum = gclamp((log2f(lum) - min_log) * (1.0f / log_range), 0.0f, 1.0f);
      bin = (uint32_t)(logLum * 254.0f + 1.0f);
    }
    atomicAdd(&bins[bin], 1u);
  }
  __syncthreads();
  if (bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
}
// auto_exposure_avg.comp:19-53: weighted bin average -> luminance -> exponential adaptation; clears the histogram
__global__ void __launch_bounds__(256) k_exposure_average(uint32_t* __restrict__ hist, float* __restrict__ avg, uint32_t n_pixels,
                                                          float min_log, float log_range, float time_coeff) {
  __shared__ uint32_t s[256];
  s[threadIdx.x] = hist[threadIdx.x] * threadIdx.x;
  __syncthreads();
  hist[threadIdx.x] = 0;
  for (uint32_t cutoff = 128; cutoff > 0; cutoff >>= 1) {
    if (threadIdx.x < cutoff) s[threadIdx.x] += s[threadIdx.x + cutoff];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float num = fmaxf((float)n_pixels, 1.0f);
    const float weighted_log_avg = ((float)s[0] / num) - 1.0f;
    const float weighted_avg_lum = exp2f(((weighted_log_avg / 254.0f) * log_range) + min_log);
    const float last = *avg;
    *avg = last + (weighted_avg_lum - last) * time_coeff;
  }
}
namespace {
__device__ __forceinline__ float rrt_odt_fit(float v) {  // tone_map.comp:39-43
  return (v * (v + 0.0245786f) - 0.000090537f) / (v * (0.983729f * v + 0.4329510f) + 0.238081f);
}
__device__ float oetf(uint32_t tf, float c) {  // tone_map.comp:72-181
  switch (tf) {
    case 1: return c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f;
    case 2: return c <= -0.0031308f ? -1.055f * powf(-c, 1.0f / 2.4f) + 0.055f
                                    : (c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f);
    case 3: return powf(c / 52.37f, 1.0f / 2.6f);
    case 4: return c < 0.0030186f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f;
    case 5: return c < 0.0181f ? 4.5f * c : 1.0993f * powf(c, 0.45f) - (1.0993f - 1.0f);
    case 6: {
      const float m1 = 2610.0f / 16384.0f, m2 = (2523.0f / 4096.0f) * 128.0f, c2 = (2413.0f / 4096.0f) * 32.0f,
                  c3 = (2392.0f / 4096.0f) * 32.0f;
      const float c1 = c3 - c2 + 1.0f;
      const float Lm = powf(c, m1);
      return powf((c1 + c2 * Lm) / (1.0f + c3 * Lm), m2);
    }
    case 7: return c < (1.0f / 12.0f) ? sqrtf(3.0f * c) : 0.17883277f * logf(12.0f * c - (1.0f - 4.0f * 0.17883277f)) + 0.55991073f;
    case 8: return powf(c, 256.0f / 563.0f);
    default: return c;
  }
}
}  // namespace
struct ToneMapArgs {
  const uint16_t* src;
  const uint32_t* albedo;
  uint16_t* dst;
  const float* avg;
  uint32_t n_pixels, transfer_function;
  float conv[9];
};
// tone_map.comp:184-220: radiance x albedo x exposure -> display primaries -> ACES fit -> OETF
__global__ void __launch_bounds__(256) k_tone_map(ToneMapArgs t) {
  const float avg = *t.avg;
  float exposure = 1.0f / (9.6f * avg);
  exposure *= 9.6f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.n_pixels; i += (size_t)gridDim.x * blockDim.x) {
    float w;
    const V3 c = load_radiance(t.src, i, w);
    const uint32_t ap = t.albedo[i];
    V3 m = modulate_by_avg_albedo(c, ((ap & 1023u) << 22) | (((ap >> 10) & 1023u) << 12) | (((ap >> 20) & 1023u) << 2));
    m = mk(m.x * exposure, m.y * exposure, m.z * exposure);
    m = mk((t.conv[0] * m.x + t.conv[3] * m.y) + t.conv[6] * m.z, (t.conv[1] * m.x + t.conv[4] * m.y) + t.conv[7] * m.z,
           (t.conv[2] * m.x + t.conv[5] * m.y) + t.conv[8] * m.z);
    V3 r = mk((m.x * 0.59719f + m.y * 0.35458f) + m.z * 0.04823f, (m.x * 0.07600f + m.y * 0.90834f) + m.z * 0.01566f,
              (m.x * 0.02840f + m.y * 0.13383f) + m.z * 0.83777f);
    r = mk(rrt_odt_fit(r.x), rrt_odt_fit(r.y), rrt_odt_fit(r.z));
    const V3 o = mk((r.x * 1.60475f + r.y * -0.53108f) + r.z * -0.07367f, (r.x * -0.10208f + r.y * 1.10813f) + r.z * -0.00605f,
                    (r.x * -0.00327f + r.y * -0.07276f) + r.z * 1.07602f);
    store_half4((DUST_RW(uint16_t))t.dst, i, oetf(t.transfer_function, o.x), oetf(t.transfer_function, o.y), oetf(t.transfer_function, o.z), 1.0f);
  }
}
hipError_t launch_tone_map(const uint16_t* src, const uint32_t* albedo, uint16_t* dst, uint32_t n_pixels, uint32_t* hist, float* avg,
                           float min_log, float log_range, float time_coeff, const float conv[9], uint32_t tf, hipStream_t s) {
  hipLaunchKernelGGL(k_exposure_histogram, dim3(1024), dim3(256), 0, s, src, n_pixels, min_log, log_range, hist);
  hipLaunchKernelGGL(k_exposure_average, dim3(1), dim3(256), 0, s, hist, avg, n_pixels, min_log, log_range, time_coeff);
  ToneMapArgs t;
  t.src = src; t.albedo = albedo; t.dst = dst; t.avg = avg; t.n_pixels = n_pixels; t.transfer_function = tf;
  for (int i = 0; i < 9; ++i) t.conv[i] = conv[i];
  hipLaunchKernelGGL(k_tone_map, dim3(2048), dim3(256), 0, s, t);
  return hipGetLastError();
}

// ==================================================================== device function evaluation (dust_hip_device_eval)
// Runs ONE of the device functions the traversal and shading kernels are made of on n independent inputs, so that the
// arithmetic that otherwise only shows through whole frames can be checked against vectors directly (tests/golden/*.npz:
// an independent restatement of the shaders). The functions are the same inlined bodies the frame kernels use.
struct EvalArgs {
  const uint32_t* in;
  uint32_t* out;
  uint32_t fn, in_words, out_words, n;
  float sky[56];  // fns 15, 16: the sky state of the call (the leading rows of its input), read as the frame kernels read theirs
};
constexpr uint32_t kEvalSkyRows = 19;  // 56 floats in rows of 3 words, the last word padding
__global__ void __launch_bounds__(256) k_device_eval(EvalArgs e) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= e.n) return;
  if ((e.fn == 15 || e.fn == 16) && i < kEvalSkyRows) return;  // the state's rows: their output stays zero
  const uint32_t* in = e.in + (size_t)i * e.in_words;
  uint32_t* out = e.out + (size_t)i * e.out_words;
  auto f = [&](int k) { return __uint_as_float(in[k]); };
  auto put3 = [&](V3 v) { out[0] = __float_as_uint(v.x); out[1] = __float_as_uint(v.y); out[2] = __float_as_uint(v.z); };
  switch (e.fn) {
    case 0: case 1: case 2: {  // in: o[3] d[3] tmin mask_lo mask_hi -> reported, t, voxel
      const V3 o = mk(f(0), f(1), f(2)), d = mk(f(3), f(4), f(5));
      const V3 tc = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);  // trace_instance's reciprocals: hit.rint:88 `1.0 / dir`
      float t = 0.0f;
      uint32_t vox = 0;
      bool rep;
      if (e.fn == 0) rep = brick_intersect<0>(o, d, tc, in[7], in[8], f(6), t, vox);
      else if (e.fn == 1) rep = brick_intersect<1>(o, d, tc, in[7], in[8], f(6), t, vox);
      else rep = brick_intersect<2>(o, d, tc, in[7], in[8], f(6), t, vox);
      out[0] = rep ? 1u : 0u; out[1] = rep ? __float_as_uint(t) : 0u; out[2] = rep ? vox : 0u;
      break;
    }
    case 3: out[0] = logluv_encode(mk(f(0), f(1), f(2))); break;
    case 4: put3(logluv_decode(in[0])); break;
    case 5: out[0] = nrd_pack_normal(mk(f(0), f(1), f(2)), 1.0f, f(3)); break;
    case 6: put3(nrd_unpack_normal(in[0])); break;
    case 7: {  // in: rgb[3] hitdist -> the four fp16 values store_radiance writes
      const u32x2 v = pack_radiance(mk(f(0), f(1), f(2)), f(3));
      out[0] = v.x; out[1] = v.y;
      break;
    }
    case 8: {
      u32x2 v;
      v.x = in[0]; v.y = in[1];
      float w;
      put3(decode_radiance(v, w));
      out[3] = __float_as_uint(w);
      break;
    }
    case 9: out[0] = pack_rgb10a2(f(0), f(1), f(2), f(3)); break;
    case 10: {
      const V3 c = cubed_normalize(mk(f(0), f(1), f(2)));
      put3(c);
      out[3] = normal2faceid(c);
      break;
    }
    case 11: put3(rotate_by_normal(mk(f(0), f(1), f(2)), mk(f(3), f(4), f(5)))); break;
    case 15: case 16: {  // in: dir[3] -> rgb[3], the state through the constant address space off the kernel argument
      const DUST_CONST_AS EvalArgs& ka = *(const DUST_CONST_AS EvalArgs*)__builtin_amdgcn_kernarg_segment_ptr();
      const V3 dir = mk(f(0), f(1), f(2));
      V3 c;  // (inlined here as in the frame kernels: no out-of-line copy of either body joins the code object)
      if (e.fn == 15) { [[clang::always_inline]] c = sky_radiance(ka.sky, dir); }
      else { [[clang::always_inline]] c = sun_radiance(ka.sky, dir); }
      put3(c);
      break;
    }
    case 17: {  // in: r[3], packed avg_albedo -> the three srgb_to_linear results, then the modulated colour
      const uint32_t p = in[3];
      put3(mk(srgb_to_linear(div_const((float)((p >> 22) & 1023u), 1023.0f)), srgb_to_linear(div_const((float)((p >> 12) & 1023u), 1023.0f)),
              srgb_to_linear(div_const((float)((p >> 2) & 1023u), 1023.0f))));
      const V3 m = modulate_by_avg_albedo(mk(f(0), f(1), f(2)), p);
      out[3] = __float_as_uint(m.x); out[4] = __float_as_uint(m.y); out[5] = __float_as_uint(m.z);
      break;
    }
    case 18: {  // in: x y z (int32) dir capacity -> fingerprint, location (0 for a capacity of 0)
      HashKey k;
      k.x = (int)in[0]; k.y = (int)in[1]; k.z = (int)in[2]; k.dir = in[3];
      out[0] = key_fingerprint(k);
      out[1] = in[4] ? key_location(k, in[4]) : 0u;
      break;
    }
    case 19: {  // in: the 9 words of a probe window, fingerprint, value[3], frame_index -> the window after the insert
      HashWindow win;
#pragma unroll
      for (int k = 0; k < 9; ++k) win.w[k] = in[k];
      hash_insert_window(win, in[9], mk(f(10), f(11), f(12)), in[13]);
#pragma unroll
      for (int k = 0; k < 9; ++k) out[k] = win.w[k];
      break;
    }
    default: break;
  }
}
hipError_t launch_device_eval(uint32_t fn, const uint32_t* in, uint32_t in_words, uint32_t* out, uint32_t out_words, uint32_t n, const float* sky,
                              hipStream_t s) {
  EvalArgs e;
  for (int i = 0; i < 56; ++i) e.sky[i] = sky ? sky[i] : 0.0f;
  e.in = in; e.out = out; e.fn = fn; e.in_words = in_words; e.out_words = out_words; e.n = n;
  hipLaunchKernelGGL(k_device_eval, dim3((n + 255) / 256), dim3(256), 0, s, e);
  return hipGetLastError();
}

// ==================================================================== launchers (called from capi.cpp)
// `a` is the launch descriptor, passed to the kernels by value.
// ==================================================================== cost-ordered work distribution
// A persistent launch ends when its LAST tile does, and tile costs are far from equal (a packet whose rays graze a dozen
// instances takes several times the median): with tiles handed out in screen order the expensive ones that happen to be drawn
// late leave most of the GPU idle while a few waves finish them -- a quarter of the fused kernel's time on the castle. Costs
// barely change from one frame to the next (same view, or a slowly moving one), so each launch records per-tile cycles and the
// next launch of the same pass hands its tiles out longest first: per band (the XCD affinity stays), a stable counting sort of
// the band's tiles into 32 cost classes a quarter octave apart, most expensive class first. One workgroup per band, wave
// ballots for the ranks (as radix.hip), ~5 us. The order only decides which wave traces which tile when -- never a result.
constexpr uint32_t kTileOrderMaxBand = 65536;  // tiles per band the sorter stages in LDS (an 8K frame has 64 800)
__global__ void __launch_bounds__(1024) k_tile_order(const uint32_t* __restrict__ cost, uint32_t* __restrict__ order, uint32_t* cuts,
                                                       uint32_t total, uint32_t per, uint32_t reuse_cuts) {
  __shared__ uint32_t cnt[16][32];
  __shared__ uint32_t wave_part[16];
  __shared__ unsigned long long wave_sum[16];
  __shared__ uint32_t s_cuts[kRegions + 1], cut_chunk[kRegions + 1];
  __shared__ unsigned long long cut_need[kRegions + 1];
  __shared__ uint8_t octave[kTileOrderMaxBand];  // quarter octaves of each tile's cost: the only pass over global memory
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  // Bands of equal COST, not of equal tile count. With equal counts the bands of a frame differ by tens of percent in work (sky
  // above, a courtyard full of detail below): the waves of the light bands then end up stealing the heavy band's remaining tiles,
  // which are its cheapest but still mid-sized, at a time when only small tiles should be left -- 8 % of the fused kernel's wave
  // time idled behind them at 1080p (tools/wave_times.py). Every workgroup works the cuts out for itself (a scan over the cost
  // map: thread t sums a contiguous run, the runs are prefix-summed through shuffles and LDS, and the thread whose run holds
  // the k/8 point of the total walks it); a cut is a tile index in screen order, so a band is still contiguous (one XCD's L2).
  if (cuts && !reuse_cuts) {
    // chunk c = tiles [512 c, 512 c + 512) as eight rows of 64: load j of a wave is row j, one coalesced 256-byte access (a lane reading
    // eight CONSECUTIVE tiles made every load touch 64 different sectors: 13 us of address processing per workgroup). A lane adds up its
    // column, a wave the 64 columns (values are capped at 2^22 cycles, so a chunk fits 32 bits; the chunk sums live where the sorter's
    // quarter octaves will)
    uint32_t* chunk_sum = reinterpret_cast<uint32_t*>(octave);
    constexpr uint32_t kChunk = 512u, kCap = 1u << 22;
    const uint32_t nc = (total + kChunk - 1u) / kChunk;   // <= 1024: total <= kRegions * kTileOrderMaxBand (the host checks `per`)
    for (uint32_t c = wave; c < nc; c += 64u) {  // four chunks' 32 loads in flight before the first reduction: this loop is memory latency and nothing else
      uint32_t v[4], raw[4][8];
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {  // clamped indices, so that no load needs a guard ...
        const uint32_t i0 = (c + 16u * q) * kChunk + lane;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) raw[q][j] = cost[min(i0 + 64u * j, total - 1u)];
      }
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)  // ... and the values pinned here, so that the compiler does not sink each load behind its use again (a wait per load: 13 us)
        asm volatile("" ::"v"(raw[q][0]), "v"(raw[q][1]), "v"(raw[q][2]), "v"(raw[q][3]), "v"(raw[q][4]), "v"(raw[q][5]), "v"(raw[q][6]), "v"(raw[q][7]));
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t i0 = (c + 16u * q) * kChunk + lane;
        uint32_t t = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) t += i0 + 64u * j < total ? min(max(raw[q][j], 1u), kCap) : 0u;  // (a tile nobody has timed yet counts as cheap)
        v[q] = t;
      }
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        uint32_t t = v[q];
#pragma unroll
        for (uint32_t d = 32; d > 0; d >>= 1) t += (uint32_t)__shfl_xor((int)t, (int)d);
        if (lane == 0 && c + 16u * q < nc) chunk_sum[c + 16u * q] = t;
      }
    }
    if (threadIdx.x <= kRegions) { s_cuts[threadIdx.x] = threadIdx.x == kRegions ? total : 0u; cut_chunk[threadIdx.x] = 0xFFFFFFFFu; }
    __syncthreads();
    // thread t owns chunk t: exclusive prefix over the chunk sums through shuffles and 16 wave totals
    const unsigned long long mine = threadIdx.x < nc ? chunk_sum[threadIdx.x] : 0u;
    unsigned long long inc = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const unsigned long long up = (unsigned long long)__shfl_up((long long)inc, (int)d);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (uint32_t w = 0; w < 16; ++w) { if (w < wave) before += wave_sum[w]; all += wave_sum[w]; }
    const unsigned long long excl = before + inc - mine;
    for (uint32_t k = 1; k < kRegions; ++k) {  // the thread whose chunk holds the k/8 point of the total says so ...
      const unsigned long long target = all / kRegions * k;
      if (mine != 0 && excl < target && target <= excl + mine) { cut_chunk[k] = threadIdx.x; cut_need[k] = target - excl; }
    }
    __syncthreads();
    if (wave >= 1u && wave < kRegions && cut_chunk[wave] != 0xFFFFFFFFu) {  // ... and wave k finds the tile inside it: the row of 64, then the lane
      const uint32_t i0 = cut_chunk[wave] * kChunk + lane;
      uint32_t t8[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) t8[j] = cost[min(i0 + 64u * j, total - 1u)];
      asm volatile("" ::"v"(t8[0]), "v"(t8[1]), "v"(t8[2]), "v"(t8[3]), "v"(t8[4]), "v"(t8[5]), "v"(t8[6]), "v"(t8[7]));
      unsigned long long need = cut_need[wave];
      uint32_t cut = min(cut_chunk[wave] * kChunk + kChunk, total);  // (the chunk's last tile, should rounding leave the point behind it)
      bool found = false;
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t mine_j = i0 + 64u * j < total ? min(max(t8[j], 1u), kCap) : 0u;
        uint32_t incl = mine_j;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
          const uint32_t up = (uint32_t)__shfl_up((int)incl, (int)d);
          if (lane >= d) incl += up;
        }
        const uint32_t row = (uint32_t)__shfl((int)incl, 63);
        const unsigned long long reached = __ballot((unsigned long long)incl >= need);
        if (!found && reached) { cut = min(cut_chunk[wave] * kChunk + 64u * j + (uint32_t)__builtin_ctzll(reached) + 1u, total); found = true; }
        if (!found) need -= row;
      }
      if (lane == 0) s_cuts[wave] = cut;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // (a band the sorter cannot stage -- frames beyond 8K with most of their cost in one corner: the equal split)
      bool ok = true;
      for (uint32_t k = 0; k < kRegions; ++k) ok = ok && s_cuts[k] <= s_cuts[k + 1] && s_cuts[k + 1] - s_cuts[k] <= kTileOrderMaxBand;
      if (!ok) for (uint32_t k = 0; k <= kRegions; ++k) s_cuts[k] = min(k * per, total);
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x <= kRegions) cuts[threadIdx.x] = s_cuts[threadIdx.x];
    __syncthreads();  // (the chunk sums are dead: `octave` is the sorter's from here)
  } else if (cuts) {  // the cuts of an earlier launch on the same grid: a view that moves keeps them for a few frames
    if (threadIdx.x <= kRegions) s_cuts[threadIdx.x] = min(cuts[threadIdx.x], total);
    __syncthreads();
  } else {
    if (threadIdx.x <= kRegions) s_cuts[threadIdx.x] = min(threadIdx.x * per, total);
    __syncthreads();
  }
  const uint32_t lo = s_cuts[blockIdx.x], hi = s_cuts[blockIdx.x + 1u];
  const uint32_t n = hi - lo;
  uint32_t top = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 1024u) {
    const uint32_t c = cost[lo + i];  // (stays: a launch that measures overwrites the tiles it traces, and the map can be read back)
    const uint32_t q = c ? 1u + (uint32_t)(4.0f * __log2f((float)c)) : 0u;  // 0 = never timed, else 1 + floor(4 log2 c) <= 129
    octave[i] = (uint8_t)q;
    top = max(top, q);
  }
#pragma unroll
  for (uint32_t d = 32; d > 0; d >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, (int)d));
  if (lane == 0) wave_part[wave] = top;
  if (threadIdx.x < 512) (&cnt[0][0])[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t w = 0; w < 16; ++w) top = max(top, wave_part[w]);
  __syncthreads();
  const uint32_t chunk = ((n + 15u) / 16u + 63u) & ~63u;  // a wave owns a contiguous run: (wave, round, lane) order is index order
  const uint32_t begin = wave * chunk;
  const uint64_t lower = (1ull << lane) - 1ull;
  for (int pass = 0; pass < 2; ++pass) {  // pass 0 counts, pass 1 places
    for (uint32_t r = 0; r < chunk; r += 64u) {
      const uint32_t i = begin + r + lane;
      const bool valid = i < n;
      const uint32_t q = valid ? octave[i] : 0u;
      // class 0 = within a quarter octave of the band's most expensive tile, ..., 31 = 1/256 of it or less (or never timed)
      const uint32_t digit = q ? min(top - q, 31u) : 31u;
      uint64_t peers = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        const bool bit = (digit >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
      }
      const uint32_t before = cnt[wave][digit];
      const uint32_t rank = before + (uint32_t)__popcll(peers & lower);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (valid && (peers & lower) == 0) cnt[wave][digit] = before + (uint32_t)__popcll(peers);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (pass == 1 && valid) order[lo + rank] = lo + i;
    }
    __syncthreads();
    if (pass == 0) {  // 512 counters -> exclusive prefix in class-major, wave-minor order: shuffles inside a wave, wave sums through LDS
      uint32_t v = 0, inc = 0;
      if (threadIdx.x < 512) {
        v = cnt[threadIdx.x & 15u][threadIdx.x >> 4];
        inc = v;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
          const uint32_t up = (uint32_t)__shfl_up((int)inc, (int)d);
          if (lane >= d) inc += up;
        }
        if (lane == 63) wave_part[wave] = inc;
      }
      __syncthreads();
      if (threadIdx.x < 512) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < wave; ++w) before += wave_part[w];
        cnt[threadIdx.x & 15u][threadIdx.x >> 4] = before + inc - v;
      }
      __syncthreads();
    }
  }
}
// Tile costs are noisy: the same tile of the same view, timed in two launches, differs by tens of percent (it depends on which waves
// shared its SIMD), and the 300 most expensive tiles of one launch cost 0.76 of that in the next. The order is therefore made from
// a running mean of the measurements -- half the new one, half what was known -- which a tile nobody has timed yet starts at once.
__global__ void __launch_bounds__(256) k_cost_blend(const uint32_t* __restrict__ raw, uint32_t* __restrict__ smooth, uint32_t total, uint32_t keep_shift) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const uint32_t r = raw[i], o = smooth[i];
    // keep_shift k: new = old + (raw - old) / 2^k (k = 1: the mean of the two); old == 0: nothing known, take the measurement
    smooth[i] = (o == 0u || r == 0u || keep_shift == 0u) ? (r ? r : o) : (uint32_t)((long long)o + (((long long)r - (long long)o) >> keep_shift));
  }
}
// A view that moves: what made a tile expensive is, a few frames on, partly in the tile next to it. The order of such a view is made
// from each tile's cost or its most expensive neighbour's, whichever is more (3 x 3 tiles): a tile beside an expensive one starts early too.
__global__ void __launch_bounds__(256) k_cost_dilate(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t tiles_x, uint32_t tiles_y) {
  const uint32_t total = tiles_x * tiles_y;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const uint32_t y = i / tiles_x, x = i - y * tiles_x;
    uint32_t m = 0;
    for (uint32_t yy = y ? y - 1u : 0u; yy <= min(y + 1u, tiles_y - 1u); ++yy)
      for (uint32_t xx = x ? x - 1u : 0u; xx <= min(x + 1u, tiles_x - 1u); ++xx) m = max(m, in[yy * tiles_x + xx]);
    out[i] = m;
  }
}
hipError_t launch_cost_blend(const uint32_t* raw, uint32_t* smooth, uint32_t total, uint32_t keep_shift, hipStream_t s) {
  hipLaunchKernelGGL(k_cost_blend, dim3((total + 255u) / 256u < 64u ? (total + 255u) / 256u : 64u), dim3(256), 0, s, raw, smooth, total, keep_shift);
  return hipGetLastError();
}
hipError_t launch_cost_dilate(const uint32_t* in, uint32_t* out, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s) {
  const uint32_t total = tiles_x * tiles_y;
  hipLaunchKernelGGL(k_cost_dilate, dim3((total + 255u) / 256u < 64u ? (total + 255u) / 256u : 64u), dim3(256), 0, s, in, out, tiles_x, tiles_y);
  return hipGetLastError();
}
// cuts: kRegions + 1 tile indices the kernel fills in (the cost-balanced bands the order is made for), or null = equal bands of `per`
// reuse_cuts: keep the cuts an earlier launch on this grid left there (the order is then made for those bands)
hipError_t launch_tile_order(const uint32_t* cost, uint32_t* order, uint32_t* cuts, bool reuse_cuts, uint32_t total, uint32_t per, hipStream_t s) {
  if (per > kTileOrderMaxBand) return hipErrorInvalidValue;  // (the caller keeps screen order for frames beyond 8K)
  hipLaunchKernelGGL(k_tile_order, dim3(kRegions), dim3(1024), 0, s, cost, order, cuts, total, per, reuse_cuts ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_primary(const FrameArgs& a_in, uint32_t grid, uint32_t block, bool count, hipStream_t s) {
  const size_t lds = lds_bytes(a_in, block);
  DUST_LAUNCH_MODE(k_primary, count, a_in);
#if defined(DUST_WALK_PROBE) && DUST_WALK_PROBE >= 2
  {
    const uint32_t waves = a_in.tiles_x * a_in.tiles_y;
    if (a_in.deep) hipLaunchKernelGGL(k_shade_probe<2>, dim3((waves + 3u) / 4u), dim3(256), 0, s, a_in);
    else hipLaunchKernelGGL(k_shade_probe<0>, dim3((waves + 3u) / 4u), dim3(256), 0, s, a_in);
  }
#endif
  return hipGetLastError();
}
hipError_t launch_primary_ao(const FrameArgs& a_in, uint32_t grid, uint32_t block, bool count, hipStream_t s) {
  const size_t lds = lds_bytes(a_in, block);
  DUST_LAUNCH_MODE(k_primary_ao, count, a_in);
  return hipGetLastError();
}
// n frames (2 .. kMaxBatch) in one launch; frames[0] decides the kernel variant and the geometry. Frames after the first: no dealt round.
// A frame whose view_run is above 1 leads a view run (dust_dev.h): the launch then goes to k_primary_ao_runs, which hands out tiles per run.
hipError_t launch_primary_ao_batch(const FrameArgs* frames, uint32_t n, uint32_t grid, uint32_t block, hipStream_t s) {
  if (n < 1u || n > kMaxBatch) return hipErrorInvalidValue;
  bool runs = false;
  for (uint32_t i = 0; i < n; ++i) runs = runs || frames[i].view_run > 1u;
  uint32_t last_lead = n - 1u;   // first frame of the launch's last run (no runs: its last frame)
  if (runs)
    for (uint32_t i = 0; i < n;) {
      const uint32_t run = frames[i].view_run;
      if (run < 1u || run > n - i) return hipErrorInvalidValue;   // every run starts at a leader and ends inside the launch
      for (uint32_t m = 1; m < run; ++m)
        if (frames[i + m].view_run != 0u) return hipErrorInvalidValue;
      last_lead = i;
      i += run;
    }
  const size_t lds = lds_bytes(frames[0], block) + 16u * (n - 1u);   // + a tile queue per further frame (frame_queue)
  BatchArgs b;
  for (uint32_t i = 0; i < n; ++i) {
    b.f[i] = with_schedule(frames[i], grid, block);
    // (a dealt tile is BOUND to its wave: a wave held up by a long tile of frame i would sit on the most expensive tiles of every later frame --
    //  measured on 1/8 row bands: 0.095 ms per band frame against 0.039)
    // (... and for whole frames, several rounds of tiles per wave, dealing every frame's first round changes nothing: 1.6653 -> 1.6635 ms)
    if (i) b.f[i].static_rounds = 0u;
    b.f[i].batch_frames = i ? 0u : n;
    {  // tickets per refill: a quarter of what a workgroup's share of a band comes to, between kGrabBatch and kBatchGrabMax; the last frame: kGrabBatch
      const uint32_t groups_per_band = (grid + kRegions - 1u) / kRegions;
      const uint32_t share = b.f[i].tiles_per_band / (4u * (groups_per_band ? groups_per_band : 1u));
      b.f[i].batch_grab = i >= last_lead ? kGrabBatch : (share < kGrabBatch ? kGrabBatch : (share > kBatchGrabMax ? kBatchGrabMax : share));
    }
    b.f[i].batch_queue_base = (uint32_t)lds_bytes(frames[0], block);
  }
  for (uint32_t i = n; i < kMaxBatch; ++i) b.f[i] = b.f[0];   // (never read)
  if (runs) switch ((b.f[0].deep ? 2 : 0) | (b.f[0].n_groups ? 4 : 0)) {
    case 0: hipLaunchKernelGGL(k_primary_ao_runs<0>, dim3(grid), dim3(block), lds, s, b); break;
    case 2: hipLaunchKernelGGL(k_primary_ao_runs<2>, dim3(grid), dim3(block), lds, s, b); break;
    case 4: hipLaunchKernelGGL(k_primary_ao_runs<4>, dim3(grid), dim3(block), lds, s, b); break;
    default: hipLaunchKernelGGL(k_primary_ao_runs<6>, dim3(grid), dim3(block), lds, s, b); break;
  }
  else switch ((b.f[0].deep ? 2 : 0) | (b.f[0].n_groups ? 4 : 0)) {
    case 0: hipLaunchKernelGGL(k_primary_ao_batch<0>, dim3(grid), dim3(block), lds, s, b); break;
    case 2: hipLaunchKernelGGL(k_primary_ao_batch<2>, dim3(grid), dim3(block), lds, s, b); break;
    case 4: hipLaunchKernelGGL(k_primary_ao_batch<4>, dim3(grid), dim3(block), lds, s, b); break;
    default: hipLaunchKernelGGL(k_primary_ao_batch<6>, dim3(grid), dim3(block), lds, s, b); break;
  }
  return hipGetLastError();
}
hipError_t launch_ambient_occlusion(const FrameArgs& a_in, uint32_t grid, uint32_t block, bool count, hipStream_t s) {
  const size_t lds = lds_bytes(a_in, block);
  DUST_LAUNCH_MODE(k_ambient_occlusion, count, a_in);
  return hipGetLastError();
}
hipError_t launch_accumulate(const FrameArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_accumulate, dim3(2048), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t configure_gi_kernels(size_t max_lds);  // gi.hip
hipError_t configure_kernels(size_t max_lds) {
  hipError_t e;
#ifdef DUST_PROFILE
  max_lds -= sizeof(g_prof);  // the profiling build's static buckets come out of the same 160 KB
#endif
#ifdef DUST_TRACE_DEBUG
  max_lds -= 1024;
#endif
  const void* fns[] = {
      (const void*)k_primary<0>, (const void*)k_primary<1>, (const void*)k_primary<2>, (const void*)k_primary<3>, (const void*)k_primary<4>, (const void*)k_primary<5>, (const void*)k_primary<6>, (const void*)k_primary<7>,
      (const void*)k_ambient_occlusion<0>, (const void*)k_ambient_occlusion<1>, (const void*)k_ambient_occlusion<2>, (const void*)k_ambient_occlusion<3>, (const void*)k_ambient_occlusion<4>, (const void*)k_ambient_occlusion<5>, (const void*)k_ambient_occlusion<6>, (const void*)k_ambient_occlusion<7>,
      (const void*)k_primary_ao<0>, (const void*)k_primary_ao<1>, (const void*)k_primary_ao<2>, (const void*)k_primary_ao<3>, (const void*)k_primary_ao<4>, (const void*)k_primary_ao<5>, (const void*)k_primary_ao<6>, (const void*)k_primary_ao<7>,
      (const void*)k_primary_ao_batch<0>, (const void*)k_primary_ao_batch<2>, (const void*)k_primary_ao_batch<4>, (const void*)k_primary_ao_batch<6>,
      (const void*)k_primary_ao_runs<0>, (const void*)k_primary_ao_runs<2>, (const void*)k_primary_ao_runs<4>, (const void*)k_primary_ao_runs<6>};
  for (const void* f : fns) {
    e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds);
    if (e != hipSuccess) return e;
  }
  return configure_gi_kernels(max_lds);
}

}  // namespace dust

#ifdef DUST_WAVE_TIMES
extern "C" int dust_hip_launch_clocks(unsigned long long* out) {  // 256 x 3
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(dust::g_launch_clock), sizeof(unsigned long long) * 256 * 3) == hipSuccess ? 0 : -1;
}
extern "C" int dust_hip_wave_times(unsigned long long* out) {  // 8192 x 6, of the last fused launch
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(dust::g_wave_times), sizeof(unsigned long long) * 8192 * 12) == hipSuccess ? 0 : -1;
}
#endif
#ifdef DUST_PROFILE
// profiling build only (tools/kernel_sections.py): read and clear the section cycle counters
extern "C" int dust_gi_profile_read(unsigned long long* out, int n);  // gi.hip's copy of the buckets
extern "C" int dust_hip_profile_read(unsigned long long* out, int n) {
  unsigned long long h[dust::kProfBuckets] = {}, g[dust::kProfBuckets] = {};
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(dust::g_prof_out), sizeof h) != hipSuccess) return -1;
  if (dust_gi_profile_read(g, dust::kProfBuckets) != 0) return -1;
  for (int i = 0; i < n && i < dust::kProfBuckets; ++i) out[i] = h[i] + g[i];
  unsigned long long z[dust::kProfBuckets] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(dust::g_prof_out), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
