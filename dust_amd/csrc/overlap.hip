// overlap.hip -- caller-supplied world-space boxes against the committed scene (dust_hip_scene_overlap_boxes / _async): every solid
// voxel inside a region -- collision, placement, area edits, trigger volumes. The region counterpart of query.hip's rays.
//
// One query per WAVE. Persistent workgroups of kOverlapWaves waves take kOverlapChunk queries at a time from the ray queries' device
// counter (same stream, same protocol). The listing of instances, the per-instance voxel range, the separating axes, the float32
// formulas and the tree steps are box_query.hpp's, shared with sweep.hip. What this file owns:
//  1. the order of the visit: ascending instance id. A listed query's candidates are ranked by id in LDS; one that could not be
//     listed tests every instance box in id order, 64 per step.
//  2. per instance: the root (-> l2 for 4096^3 trees) cells in the voxel range are looked up a lane per 16-cell, the occupied ones taken
//     in ascending child order -- depth-first storage makes that ascending block order (dust_dev.h) -- and each mid node is tested a
//     lane per BRICK: the lane loads its DustHipBlock and makes the mask of its voxels that overlap the box.
//       Axis-aligned instances: the voxel's world box on world axis r depends on ONE model coordinate, so the test is separable --
//       4 voxel slabs per axis, exactly the header's float32 formula (no contraction: -ffp-contract=off), and the 64-bit mask is
//       their outer product.
//       Other instances: a separating-axis test of the voxel's world parallelepiped against the box grown by tau / 2 (the 15 axes
//       are the instance's, kept in LDS per wave), a brick first, then its voxels.
//  3. slots come from a wave-wide exclusive prefix of the lanes' counts plus the query's running total: records leave in (instance,
//     block, voxel bit) order without atomics, the first `capacity` of them kept, nothing at or beyond n_records written.
#include "box_query.hpp"

namespace dust {
namespace {

struct OverlapLds {
  uint32_t cand[2 * kBoxCand];  // [0, kBoxCand): as found; [kBoxCand, 2 kBoxCand): ranked by id
  f32x4 axis[16];               // the 15 separating axes of the instance being tested: {L, R = support of voxel + box}
  float axis_s[16];             // ... and |L.x| + |L.y| + |L.z| (what the tolerance grows R by per unit)
};
__shared__ OverlapLds g_overlap[kOverlapWaves];

// one query, as the wave works on it
struct Query {
  float lo[3], hi[3];
  float big;                        // max |coordinate| of the box
  uint64_t first, cap, n_records;
  uint64_t total;                   // overlapping voxels so far
  bool any_hit;
};

// axis-aligned instance: the mask of a brick's voxels at (bx, by, bz) whose world box overlaps the query. col[r]: the model axis world
// axis r takes
__device__ __forceinline__ uint64_t aligned_mask(DUST_RO(float) o2w, const int col[3], int bx, int by, int bz, const Query& q) {
  uint32_t m4x = 0u, m4y = 0u, m4z = 0u;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int c = col[r];
    const int b = c == 0 ? bx : (c == 1 ? by : bz);
    float w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = plane(o2w, r, c, (float)(b + i));
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) bits |= slab_overlap(fminf(w[i], w[i + 1]), fmaxf(w[i], w[i + 1]), q.lo[r], q.hi[r]) ? (1u << i) : 0u;
    m4x |= c == 0 ? bits : 0u; m4y |= c == 1 ? bits : 0u; m4z |= c == 2 ? bits : 0u;
  }
  uint32_t yz = 0;  // bit iy << 2 | iz
#pragma unroll
  for (int iy = 0; iy < 4; ++iy) yz |= ((m4y >> iy) & 1u) ? (m4z << (4 * iy)) : 0u;
  uint64_t all = 0;
#pragma unroll
  for (int ix = 0; ix < 4; ++ix) all |= ((m4x >> ix) & 1u) ? ((uint64_t)yz << (16 * ix)) : 0ull;
  return all;
}

// general instance: does the parallelepiped o2w([x, x + size]^3) overlap the box grown by tau / 2? (the axes and their supports for
// a UNIT voxel are in the wave's LDS; a brick of 4 scales the parallelepiped's part of R by 4)
__device__ __forceinline__ bool sat_overlap(const OverlapLds& L, DUST_RO(float) o2w, float x, float y, float z, float size, const Query& q,
                                            const float half[3], const float ctr[3], const float ext[3]) {
  const float hx = x + 0.5f * size, hy = y + 0.5f * size, hz = z + 0.5f * size;
  float c[3], big = q.big;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    c[r] = ((o2w[r * 4] * hx + o2w[r * 4 + 1] * hy) + o2w[r * 4 + 2] * hz) + o2w[r * 4 + 3];
    big = fmaxf(big, fabsf(c[r]) + ext[r] * size);   // the voxel's largest corner coordinate
  }
  const float slack = 0.5e-5f * (1.0f + big);
  const float d[3] = {c[0] - ctr[0], c[1] - ctr[1], c[2] - ctr[2]};
  bool ok = true;
  for (int k = 0; k < 15; ++k) {
    const f32x4 a = L.axis[k];
    const float dist = fabsf((a.x * d[0] + a.y * d[1]) + a.z * d[2]);
    // a.w = sum_k |L.e_k| (unit voxel) ; the box's support is added here (the same for every voxel)
    const float rq = (half[0] * fabsf(a.x) + half[1] * fabsf(a.y)) + half[2] * fabsf(a.z);
    ok = ok && !(dist > a.w * size + rq + slack * L.axis_s[k]);
  }
  return ok;
}

// the instance's 15 axes into the wave's LDS (lane k < 15 makes axis k)
__device__ __forceinline__ void make_axes(OverlapLds& L, DUST_RO(float) o2w, uint32_t lane) {
  if (lane < 15u) {
    const f32x4 a = box_axis(o2w, lane);
    L.axis[lane] = a;
    L.axis_s[lane] = (fabsf(a.x) + fabsf(a.y)) + fabsf(a.z);
  }
  wave_sync_lds();
}

// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// a voxel record: {instance, block, x | y << 16, z | palette << 16 | voxel << 24}
__device__ __forceinline__ void put_ref(const OverlapArgs& o, uint64_t at, uint32_t inst, uint32_t block, const DustHipBlock& b,
                                        DUST_RO(uint8_t) materials, uint32_t v) {
  uint32_t w2, w3;
  voxel_words(b, materials, v, w2, w3);
  u32x4 r;
  r.x = inst; r.y = block; r.z = w2; r.w = w3;
  reinterpret_cast<u32x4*>(o.records)[at] = r;
}

// one mid node (16-cell idx of the node at base): a lane per brick. Returns true when the query is over (any-hit with a hit)
template <int MODE>
__device__ __forceinline__ bool visit_mid(const OverlapArgs& o, Query& q, const BoxInst& in, ModelRef m, const OverlapLds& L, uint32_t mid,
                                          const int base[3], uint32_t idx, uint32_t lane) {
  int bx, by, bz;
  uint64_t pass = 0;
  uint32_t block;
  DustHipBlock b;
  b.x = b.y = b.z = b.w = 0; b.mask = 0; b.material_ptr = 0; b.avg_albedo = 0;
  if (lane_brick(m, in, mid, base, idx, lane, bx, by, bz, block)) {
    b = load_block(m.blocks + block);
    if (in.aligned) {
      pass = aligned_mask(in.o2w, in.col, bx, by, bz, q) & b.mask;
    } else if (sat_overlap(L, in.o2w, (float)bx, (float)by, (float)bz, 4.0f, q, in.half, in.ctr, in.ext)) {
      uint64_t rest = b.mask;
      while (rest) {
        const uint32_t v = (uint32_t)__builtin_ctzll(rest);
        rest &= rest - 1ull;
        if (sat_overlap(L, in.o2w, (float)(bx + (int)(v >> 4)), (float)(by + (int)((v >> 2) & 3u)), (float)(bz + (int)(v & 3u)), 1.0f, q, in.half,
                        in.ctr, in.ext))
          pass |= 1ull << v;
      }
    }
  }
  const uint32_t cnt = (uint32_t)__popcll(pass);
  const uint64_t some = __ballot(cnt != 0u);
  if (some == 0ull) return false;
  if (q.any_hit) {  // one voxel of the first lane that has one
    if (lane == (uint32_t)__builtin_ctzll(some) && q.cap >= 1u && q.first < q.n_records)
      put_ref(o, q.first, in.id, block, b, m.materials, (uint32_t)__builtin_ctzll(pass));
    q.total = 1;
    return true;
  }
  const uint32_t incl = wave_scan(cnt, lane);
  const uint32_t sum = uniform((uint32_t)__shfl((int)incl, 63, 64));
  uint64_t slot = q.total + (incl - cnt);
  uint64_t rest = pass;
  while (rest != 0ull && slot < q.cap && q.first + slot < q.n_records) {
    const uint32_t v = (uint32_t)__builtin_ctzll(rest);
    rest &= rest - 1ull;
    put_ref(o, q.first + slot, in.id, block, b, m.materials, v);
    slot += 1u;
  }
  q.total += sum;
  return false;
}

// the occupied 16-cells in [c0, c1] of one node (box_query.hpp, visit_nodes), in ascending child order
template <int MODE>
__device__ __forceinline__ bool visit_cells(const OverlapArgs& o, Query& q, const BoxInst& in, ModelRef m, const OverlapLds& L, int l2, const int base[3],
                                            const int c0[3], const int c1[3], uint32_t lane) {
  const CellRange range(base, c0, c1);
  for (uint32_t s = 0; s < range.cells; s += 64u) {
    const uint32_t j = s + lane;
    uint32_t mid = kNoMid, idx = 0;
    if (j < range.cells) {
      int x, y, z;
      idx = range.index(j, x, y, z);
      mid = cell_mid<MODE>(m, l2, idx);
    }
    uint64_t occ = __ballot(mid != kNoMid);
    while (occ != 0ull) {
      const uint32_t src = (uint32_t)__builtin_ctzll(occ);
      occ &= occ - 1ull;
      const uint32_t mu = uniform((uint32_t)__shfl((int)mid, (int)src, 64));
      const uint32_t iu = uniform((uint32_t)__shfl((int)idx, (int)src, 64));
      if (visit_mid<MODE>(o, q, in, m, L, mu, base, iu, lane)) return true;
    }
  }
  return false;
}

// one instance whose world box meets the query. Returns true when the query is over (any-hit with a hit)
template <int MODE>
__device__ bool visit_instance(ArgsRef a, const OverlapArgs& o, Query& q, uint32_t id, uint32_t lane, OverlapLds& L) {
  ModelRef m = a.visits[id].m;
  BoxInst in;
  if (!box_instance(in, a, id, q.lo, q.hi, q.lo, q.hi, q.big)) return false;
  if (!in.aligned) make_axes(L, in.o2w, lane);
  return visit_nodes<MODE>(
      m, in, [](int, int, int, float) { return true; },
      [&](int l2, const int base[3], const int c0[3], const int c1[3]) { return visit_cells<MODE>(o, q, in, m, L, l2, base, c0, c1, lane); });
}

// the candidates a wave listed in LDS (unique ids), ranked into ascending order and visited
template <int MODE>
__device__ bool visit_listed(ArgsRef a, const OverlapArgs& o, Query& q, uint32_t n_cand, uint32_t lane, OverlapLds& L) {
  wave_sync_lds();
  for (uint32_t j = lane; j < n_cand; j += 64u) {
    const uint32_t v = L.cand[j];
    uint32_t rank = 0;
    for (uint32_t i = 0; i < n_cand; ++i) rank += L.cand[i] < v ? 1u : 0u;
    L.cand[kBoxCand + rank] = v;
  }
  wave_sync_lds();
  for (uint32_t i = 0; i < n_cand; ++i)
    if (visit_instance<MODE>(a, o, q, uniform(L.cand[kBoxCand + i]), lane, L)) return true;
  return false;
}

template <int MODE>
__device__ void overlap_query(ArgsRef a, const OverlapArgs& o, uint32_t qi, uint32_t lane, OverlapLds& L) {
  const f32x4* bq = reinterpret_cast<const f32x4*>(o.boxes) + (size_t)qi * 2u;
  const f32x4 b0 = bq[0], b1 = bq[1];
  Query q;
  q.lo[0] = b0.x; q.lo[1] = b0.y; q.lo[2] = b0.z;
  q.hi[0] = b1.x; q.hi[1] = b1.y; q.hi[2] = b1.z;
  q.first = uniform(__float_as_uint(b0.w));
  q.cap = uniform(__float_as_uint(b1.w));
  q.n_records = o.n_records;
  q.total = 0;
  q.any_hit = o.any_hit != 0u;
  q.big = 0.0f;
  bool ok = a.n_instances != 0u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ok = ok && finite(q.lo[k]) && finite(q.hi[k]) && q.lo[k] <= q.hi[k];
    q.big = fmaxf(q.big, fmaxf(fabsf(q.lo[k]), fabsf(q.hi[k])));
  }
  if (ok) {
    const uint32_t n_cand = list_instances<MODE>(a, q.lo, q.hi, L.cand, lane);
    if (n_cand <= kBoxCand) {
      visit_listed<MODE>(a, o, q, n_cand, lane, L);
    } else {
      // not listed: every instance box in id order, 64 per step
      bool done = false;
      for (uint32_t s = 0; !done && s < a.n_instances; s += 64u) {
        uint64_t bal = __ballot(s + lane < a.n_instances && instance_meets(a, s + lane, q.lo, q.hi));
        while (bal != 0ull && !done) {
          const uint32_t id = s + (uint32_t)__builtin_ctzll(bal);
          bal &= bal - 1ull;
          done = visit_instance<MODE>(a, o, q, id, lane, L);
        }
      }
    }
  }
  if (lane == 0u) o.counts[qi] = q.total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)q.total;
}

}  // namespace

// MODE: launch_by_mode (box_query.hpp)
template <int MODE>
__global__ void __launch_bounds__(kOverlapWaves * 64) k_overlap_boxes(const FrameArgs, const OverlapArgs o) {
  ArgsRef a = launch_args();
  if (blockIdx.x == 0 && threadIdx.x == 0) *o.next_counter = 0ull;
  const uint32_t lane = threadIdx.x & 63u;
  OverlapLds& L = g_overlap[threadIdx.x >> 6];
  for (;;) {  // the wave's next chunk of queries
    const unsigned long long k = next_chunk(o.counter, kOverlapChunk, lane);
    if (k >= o.n) break;
    const uint32_t end = (uint32_t)min((unsigned long long)o.n, k + kOverlapChunk);
    for (uint32_t qi = (uint32_t)k; qi < end; ++qi) overlap_query<MODE>(a, o, qi, lane, L);
  }
}

// grid, block: the host's choice (capi_scene.cpp overlap_boxes_impl); no dynamic LDS
hipError_t launch_overlap_boxes(const FrameArgs& a, const OverlapArgs& o, uint32_t grid, uint32_t block, hipStream_t s) {
  return launch_by_mode(a, [&](auto mode) { hipLaunchKernelGGL(k_overlap_boxes<decltype(mode)::value>, dim3(grid), dim3(block), 0, s, a, o); });
}

}  // namespace dust

