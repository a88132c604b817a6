// query.hip -- caller-supplied rays against the committed scene (dust_hip_scene_trace_rays / _async): what a game's own ray-tracing
// pipeline traces against the reference's TLAS (render/src/pipeline/mod.rs:64-98) -- picking, where an edit lands, line of sight, probes.
//
// One ray per LANE, as k_ray_walk carries the GI passes' rays (gi.hip): a lane takes the next ray of the launch, walks the top-level grid
// (top_begin / top_next, top.hpp) to the next instance whose box the ray meets in front of its hit so far, enters it (walk_begin) and
// walks it cell by cell (walk_step: trace_instance's cell steps, walk_cell.hpp), until the grid has nothing more in front of the hit; then the
// 32-byte hit record is written and the lane takes another ray. A trip of the wave's loop advances every lane by one phase, whatever
// phase its neighbours are in. Every ray is a primary-type ray (RT 0, hit.rint): the same brick tests on a superset of the bricks that
// can be accepted and the same tie rule as the frame's camera rays and the CPU oracle's single-ray trace -- results are bit-identical by
// construction. A scene whose grid could not be built (DustHipScene::grid_valid) has its instance boxes tested one by one instead
// (large scenes: behind their group's box, as the packet cull does).
//
// Work distribution: persistent workgroups (about one per CU) take chunks of kQueryChunk rays from a device counter -- the workgroup
// stages the scene's root nodes in LDS once (walk_step reads them through lds_slot), so the launch must not be n / 256 short-lived
// workgroups. A picking query of a few rays is one workgroup.
#include "box_query.hpp"  // palette_index, next_chunk, launch_by_mode

namespace dust {
namespace {

constexpr uint32_t kQueryChunk = 64;   // rays a wave takes from the counter at a time
constexpr uint32_t kQueryTopIters = 16;  // grid steps + box tests per trip of a lane on the top-level walk
constexpr uint32_t kQueryScanIters = 32; // box tests per trip without a grid
enum : uint32_t { Q_EMPTY = 0, Q_FETCH, Q_TOP, Q_SCAN, Q_BEGIN, Q_WALK, Q_DONE };

__device__ __forceinline__ bool finite3(V3 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }

// The hit record: t, instance, block (gl_PrimitiveID), voxel, the voxel's tree coordinates, and what hit.rchit:16-95 derives from the hit
// (primary_shade, traverse.hpp): the model-space normal -- CubedNormalize of the hit point minus the voxel's centre -- as normal2FaceID,
// and the palette index, the popcount into the brick's material stream.
__device__ __forceinline__ void put_hit(ArgsRef a, const QueryArgs& q, uint32_t rid, V3 o, V3 d, float tmax, const Hit& h) {
  u32x4 r0, r1;
  r1.x = r1.y = r1.z = r1.w = 0u;
  if (!h.found) {
    r0.x = __float_as_uint(tmax); r0.y = DUST_HIP_NO_HIT; r0.z = 0u; r0.w = 0u;
  } else {
    InstanceRef in = a.instances[h.inst];
    ModelRef m = a.visits[h.inst].m;
    const uint32_t block = resolve_block(m, h.block);
    const DustHipBlock b = load_block(m.blocks + block);
    const V3 oo = xform_point(in.w2o, o), od = xform_dir(in.w2o, d);
    const V3 hpo = mk(h.t * od.x + oo.x, h.t * od.y + oo.y, h.t * od.z + oo.z);
    const uint32_t vx = h.voxel >> 4, vy = (h.voxel >> 2) & 3u, vz = h.voxel & 3u;
    const V3 ctr = mk(((float)b.x + (float)vx) + 0.5f, ((float)b.y + (float)vy) + 0.5f, ((float)b.z + (float)vz) + 0.5f);
    const uint32_t face = normal2faceid(cubed_normalize(mk(hpo.x - ctr.x, hpo.y - ctr.y, hpo.z - ctr.z)));
    const uint32_t pal = palette_index(b, m.materials, h.voxel);
    r0.x = __float_as_uint(h.t); r0.y = h.inst; r0.z = block; r0.w = h.voxel;
    r1.x = (uint32_t)b.x + vx; r1.y = (uint32_t)b.y + vy; r1.z = (uint32_t)b.z + vz; r1.w = (face & 0xFFu) | ((pal & 0xFFu) << 8);
  }
  u32x4* out = reinterpret_cast<u32x4*>(q.hits) + (size_t)rid * 2u;
  out[0] = r0;
  out[1] = r1;
}

}  // namespace

// MODE: launch_by_mode (box_query.hpp)
template <int MODE>
__global__ void __launch_bounds__(1024, 4) k_ray_query(const FrameArgs, const QueryArgs q) {
  ArgsRef a0 = launch_args();
  if (blockIdx.x == 0 && threadIdx.x == 0) *q.next_counter = 0ull;
  copy16(g_lds, a0.root_table, a0.n_lds_models * kN16LdsBytes);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t lower = (1ull << lane) - 1ull;
  const bool any_hit = q.any_hit != 0u;
  const bool use_grid = a0.grid.cells != nullptr && a0.n_instances != 0u;
  uint32_t win_next = 0, win_end = 0;
  bool dry = false;
  uint32_t state = Q_EMPTY, rid = 0, pend = 0, ci = 0;
  V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
  float tmin = 0.0f, tmax = 0.0f;
  Hit best;
  best.found = false; best.t = 0.0f; best.inst = 0; best.block = 0; best.voxel = 0;
  TopState ts;
  ts.cell = 0; ts.prev = kNoCell; ts.cur = ts.end = 0; ts.t_end = 0.0f;
  WalkState w;
  w.o = w.d = w.inv = mk(0, 0, 0); w.t = w.tx_stop = w.near_tol = 0.0f; w.ijk[0] = w.ijk[1] = w.ijk[2] = 0;
  w.stepped = 0; w.cl_main = 2; w.steps = 0; w.screen = false; w.prev_whole = false; midcache_reset(w.mc); w.inst = 0;
  w.lds_slot = -1; w.extent = 0; w.root = nullptr; w.dense_mask = nullptr;
  LaneStats st = {0, 0, 0, 0, 0, 0};
  TopSource memsrc;  // (the grid is read from memory: the roots take the LDS)
  memsrc.base = g_lds; memsrc.cells = memsrc.items = memsrc.boxes = 0xFFFFFFFFu;
  for (uint32_t trip = 0; trip < (1u << 30); ++trip) {  // (the bound is a fuse: every phase below makes progress)
    // ---- empty lanes take the launch's next rays, in lane order
    {
      const uint64_t b_empty = __ballot(state == Q_EMPTY);
      if (b_empty != 0ull && !dry) {
        if (win_next == win_end) {  // the wave's chunk is used up
          const unsigned long long k = next_chunk(q.counter, kQueryChunk, lane);
          if (k >= q.n) dry = true;
          else { win_next = (uint32_t)k; win_end = (uint32_t)min((unsigned long long)q.n, k + kQueryChunk); }
        }
        if (!dry) {
          const uint32_t rank = (uint32_t)__popcll(b_empty & lower);
          if (state == Q_EMPTY && win_next + rank < win_end) { rid = win_next + rank; state = Q_FETCH; }
          win_next = min(win_end, win_next + (uint32_t)__popcll(b_empty));
        }
      }
    }
    if (state == Q_FETCH) {  // the ray: degenerate ones (zero or non-finite direction, non-finite origin or window, tmin > tmax) miss
      const f32x4* r = reinterpret_cast<const f32x4*>(q.rays) + (size_t)rid * 2u;
      const f32x4 r0 = r[0], r1 = r[1];
      o = mk(r0.x, r0.y, r0.z); tmin = r0.w;
      d = mk(r1.x, r1.y, r1.z); tmax = r1.w;
      best.found = false; best.t = tmax; best.inst = 0; best.block = 0; best.voxel = 0;
      const bool ok = finite3(o) && finite3(d) && __builtin_isfinite(tmin) && __builtin_isfinite(tmax) && tmin <= tmax &&
                      !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
      if (!ok) state = Q_DONE;
      else if (use_grid) {
        const V3 inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));  // (conservative box tests)
        // (from t = 0, not tmin: hit.rint starts its DDA at max(entry, tmin) and clamps the position into the brick, so a brick the ray
        //  has left before tmin still reports a solid voxel AT tmin -- the oracle's trace meets such an instance, and so must the grid walk)
        state = top_begin(a0, memsrc, o, d, inv, 0.0f, tmax, ts) ? Q_TOP : Q_DONE;
      } else {
        ci = 0;
        state = Q_SCAN;
      }
    }
    if (state == Q_WALK) {
      const DUST_CONST_AS DevVisit& v = a0.visits[w.inst];
      if (walk_step<0, MODE>(w, &v.m, tmin, tmax, any_hit, best, st)) state = (any_hit && best.found) ? Q_DONE : (use_grid ? Q_TOP : Q_SCAN);
    }
    if (state == Q_TOP) {  // the grid's next instance in front of the hit so far
      const V3 inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
      const bool zero_axis = __any(d.x == 0.0f || d.y == 0.0f || d.z == 0.0f);  // (of the lanes in this phase)
      const uint32_t r = top_next(a0, memsrc, o, d, inv, best.found ? best.t : tmax, best.found, ts, pend, kQueryTopIters, zero_axis);
      state = r == RS_BEGIN ? Q_BEGIN : (r == RS_DONE ? Q_DONE : Q_TOP);
    }
    if (state == Q_SCAN) {  // no grid: every instance box (LARGE: behind its group's box), in index (slot) order
      const V3 inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
      const float limit = best.found ? best.t : tmax;
      uint32_t next = Q_DONE;
      for (uint32_t it = 0; ci < a0.n_instances; ++it) {
        if (it == kQueryScanIters) { next = Q_SCAN; break; }
        float te, tx;
        if (LARGE && (ci & 63u) == 0u) {
          const DUST_CONST_AS DevBox& g = a0.gboxes[ci >> 6];
          if (!slab_box(o, d, inv, g.lo, g.hi, te, tx) || te * (1.0f - 2e-6f) > limit) { ci += 64u; continue; }
        }
        const DUST_CONST_AS DevBox& b = LARGE ? a0.sboxes[ci] : a0.boxes[ci];
        const uint32_t id = LARGE ? __float_as_uint(b.pad0) : ci;
        ci += 1u;
        if (slab_box(o, d, inv, b.lo, b.hi, te, tx) && !(te * (1.0f - 2e-6f) > limit)) { pend = id; next = Q_BEGIN; break; }
      }
      state = next;
    }
    if (state == Q_BEGIN) {  // enter the instance
      const DUST_CONST_AS DevVisit& v = a0.visits[pend];
      const V3 oo = xform_point(v.w2o, o), od = xform_dir(v.w2o, d);
      state = walk_begin<0, MODE>(w, v.m, pend, oo, od, tmin) ? Q_WALK : (use_grid ? Q_TOP : Q_SCAN);
    }
    if (state == Q_DONE) {  // the ray's hit record; the lane is free
      put_hit(a0, q, rid, o, d, tmax, best);
      state = Q_EMPTY;
    }
    if (dry && !__any(state != Q_EMPTY)) break;
  }
}

// grid, block: the host's choice (capi_scene.cpp trace_rays_impl); the dynamic LDS is the staged roots
hipError_t launch_ray_query(const FrameArgs& a, const QueryArgs& q, uint32_t grid, uint32_t block, hipStream_t s) {
  const size_t lds = (size_t)a.n_lds_models * kN16LdsBytes;
  return launch_by_mode(a, [&](auto mode) { hipLaunchKernelGGL(k_ray_query<decltype(mode)::value>, dim3(grid), dim3(block), lds, s, a, q); });
}
hipError_t configure_query_kernels(size_t max_lds) {  // (as configure_gi_kernels: dynamic LDS beyond 64 KiB must be asked for)
  const void* fns[] = {(const void*)k_ray_query<0>, (const void*)k_ray_query<2>, (const void*)k_ray_query<4>, (const void*)k_ray_query<6>};
#ifdef DUST_PROFILE
  max_lds -= sizeof(g_prof);  // (as configure_kernels: the profiling build's static buckets come out of the same 160 KB)
#endif
  for (const void* f : fns) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace dust
