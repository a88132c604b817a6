// body.hip -- model bodies (dust_hip_model_bodies): mass, first and second moments, voxel count and bounds per GROUP of voxels -- the
// whole model, a palette index, an island of the standing labelling or a cell of the standing fracture -- for a rigid-body solver. The
// model is only read. The arithmetic is body_rule.hpp's; this file decides which voxels go into which record.
//
// k_bodies has the shape of k_surface_count, k_census and k_fracture_records: a workgroup per root cell of the region's CellBox, four
// waves of 16 bricks, lane = voxel bit. Per brick the counted voxels are one wave-uniform word (the brick mask, the region's mask, a
// ballot of the palette filter). The distinct groups of a brick are taken as k_fracture_records takes them: the first open lane's group
// word, the ballot of its equals, clear. Per (brick, group) the ten LOCAL moments are popcounts of that word (no weights: scalar work
// only, and under ALL without a filter no grid byte is loaded) or ten 32-bit sums across the wave (weights: 255 uint16 in 512 bytes of
// LDS, looked up by the lane's grid byte); body_shift moves them to the brick's origin in 64 bits, wave-uniform. Each wave keeps ONE
// running record for the group it is looking at (Held in k_island_stats) and sends it off only when the group changes or its bricks
// end; when the four waves end holding the same group -- always under ALL, and inside any large piece -- they fold through LDS and one
// wave sends the sum. A solid terrain block then sends at most seventeen ordinary vector atomics per root cell, not per brick: ten
// 64-bit adds, one 32-bit add and six 32-bit maxima for the bounds (a byte-packed maximum would not be a maximum per axis), fields that
// hold the neutral element skipped. (Integer atomic rates on this chip are unmeasured: their number is kept small rather than
// budgeted.) All integer adds and maxima: no order shows, two runs give the same bytes. No fences, spins or waits
// BETWEEN workgroups; the one barrier is reached by every wave of a workgroup.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "body.hpp"
#include "fracture_rule.hpp"  // kFractureNoCell
#include "island.hpp"         // kNoIsland, kIslandRows
#include "surface_rule.hpp"   // surface_region_mask

namespace dust {

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return uniform(v);
}

// where group `group` of kind kGroup is accumulated: an island by its rank in key order, exactly as flush in island.hip ranks it
template <uint32_t kGroup>
__device__ __forceinline__ uint32_t group_index(const BodyArgs& a, uint32_t group) {
  if constexpr (kGroup == kBodiesIslands) {
    const uint32_t row = group >> 6;  // < kIslandRows: a label is a key below 2^24
    return a.root_count[row] + a.scan_tmp[row >> 10] + (uint32_t)__popcll(a.root_mask[row] & ((1ull << (group & 63u)) - 1ull));
  } else {
    return group;
  }
}
// one wave sends a part (wave-uniform) to its group's accumulator, as flush in island.hip does: one lane, an atomic per field that is
// not neutral
template <uint32_t kGroup>
__device__ __forceinline__ void flush(const BodyArgs& a, uint32_t group, const BodyPart& h, uint32_t lane) {
  if (h.voxels == 0u || lane != 0u) return;
  const uint32_t index = group_index<kGroup>(a, group);
  if (index >= a.capacity) return;
  BodyAcc* acc = a.acc + index;
  atomicAdd(&acc->voxels, h.voxels);
#pragma unroll
  for (uint32_t k = 0; k < kBodySums; ++k)
    if (h.s.v[k] != 0ull) atomicAdd(&acc->sums[k], (unsigned long long)h.s.v[k]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (h.inv_lo[r] != 0u) atomicMax(&acc->bounds[r], h.inv_lo[r]);
    if (h.hi[r] != 0u) atomicMax(&acc->bounds[3 + r], h.hi[r]);
  }
}

}  // namespace

template <uint32_t kGroup, bool kWeighted>
__global__ void __launch_bounds__(256) k_bodies(BodyArgs a) {
  __shared__ uint16_t weight[256];  // by grid byte: [0] unused, [1 + p] the weight of palette index p
  __shared__ unsigned long long fold_sums[4][kBodySums];
  __shared__ uint32_t fold_words[4][8];  // the wave's group, voxels, 255 - lo[3], hi[3]
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  if constexpr (kWeighted) {
    weight[threadIdx.x] = threadIdx.x == 0u ? (uint16_t)0 : a.weights[threadIdx.x - 1u];  // (256 threads; weights has 255 entries)
    __syncthreads();
  }
  const uint32_t cell = a.box.cell(blockIdx.x);
  const bool need_grid = kWeighted || kGroup == kBodiesMaterials || a.byte != 0u;  // uniform
  BodyPart h = body_neutral();  // what this wave holds for `held` (every member wave-uniform)
  uint32_t held = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t c = wave * 16u + k, code = cell * 64u + c;  // < kLattice: the box's cells are below 4096
    const uint64_t own = uniform64(a.brick_mask[code]);
    if (own == 0ull) continue;
    uint32_t bx, by, bz;
    cell_brick(cell, c, bx, by, bz);
    uint64_t m = own & surface_region_mask(bx, by, bz, a.lo, a.hi);
    if (m == 0ull) continue;
    uint32_t g = 0;
    if (need_grid) {
      g = a.grid[(size_t)code * 64u + lane];
      m &= __ballot(g != 0u && (a.byte == 0u || g == a.byte));
      if (m == 0ull) continue;
    }
    uint32_t word = 0;  // the voxel's group
    if constexpr (kGroup == kBodiesMaterials) word = g - 1u;
    if constexpr (kGroup == kBodiesIslands) {
      word = a.label[voxel_key(bx, by, bz, lane)];
      m &= __ballot(word != kNoIsland);
    }
    if constexpr (kGroup == kBodiesCells) {
      word = a.field[(size_t)code * 64u + lane];
      m &= __ballot(word != kFractureNoCell);  // voxels that answer NO_CELL belong to no group
    }
    if (m == 0ull) continue;
    const bool counted = ((m >> lane) & 1ull) != 0ull;
    BodyLocal mine{};
    if constexpr (kWeighted) mine = body_local_voxel(weight[g & 255u], lane);
    for (uint64_t open = m; open != 0ull;) {
      uint32_t group = 0;
      uint64_t mg = open;
      if constexpr (kGroup != kBodiesAll) {
        group = (uint32_t)__builtin_amdgcn_readlane((int)word, (int)__builtin_ctzll(open));
        mg = __ballot(counted && word == group);  // holds the first open lane
      }
      open &= ~mg;
      BodyLocal l;
      if constexpr (kWeighted) {
        const bool in = ((mg >> lane) & 1ull) != 0ull;
#pragma unroll
        for (uint32_t j = 0; j < kBodySums; ++j) l.v[j] = wave_sum(in ? mine.v[j] : 0u);
      } else {
        l = body_local_unweighted(mg);
      }
      const BodyPart p = body_brick_part(mg, l, bx, by, bz);
      if (h.voxels != 0u && group != held) {
        flush<kGroup>(a, held, h, lane);
        h = body_neutral();
      }
      held = group;
      body_fold(h, p);
    }
  }
  // the end of the wave's bricks: when every wave that holds something holds the same group, one wave sends their sum
  if (lane == 0u) {
    fold_words[wave][0] = held; fold_words[wave][1] = h.voxels;
#pragma unroll
    for (int r = 0; r < 3; ++r) { fold_words[wave][2 + r] = h.inv_lo[r]; fold_words[wave][5 + r] = h.hi[r]; }
#pragma unroll
    for (uint32_t j = 0; j < kBodySums; ++j) fold_sums[wave][j] = h.s.v[j];
  }
  __syncthreads();  // (no wave has left: the loop above only continues)
  uint32_t live = 0, first = 0;
  bool same = true;
#pragma unroll
  for (uint32_t w = 0; w < 4u; ++w) {
    const uint32_t group = uniform(fold_words[w][0]), voxels = uniform(fold_words[w][1]);
    if (voxels == 0u) continue;
    if (live == 0u) first = group;
    else same = same && group == first;
    live += 1u;
  }
  if (live == 0u) return;
  if (!same) {
    flush<kGroup>(a, held, h, lane);
    return;
  }
  if (wave != 0u) return;
  BodyPart t = body_neutral();
#pragma unroll
  for (uint32_t w = 0; w < 4u; ++w) {  // (a wave that holds nothing wrote the neutral element)
    BodyPart p;
    p.voxels = uniform(fold_words[w][1]);
#pragma unroll
    for (int r = 0; r < 3; ++r) { p.inv_lo[r] = uniform(fold_words[w][2 + r]); p.hi[r] = uniform(fold_words[w][5 + r]); }
#pragma unroll
    for (uint32_t j = 0; j < kBodySums; ++j) p.s.v[j] = uniform64(fold_sums[w][j]);
    body_fold(t, p);
  }
  flush<kGroup>(a, first, t, lane);
}

// a thread per row of 64 keys: the islands it names, in key order, give their accumulators their keys
__global__ void __launch_bounds__(256) k_bodies_keys(BodyArgs a) {
  const uint32_t row = blockIdx.x * 256u + threadIdx.x;  // < kIslandRows: the grid is kIslandRows / 256 workgroups
  uint64_t m = a.root_mask[row];
  if (m == 0ull) return;
  uint32_t rank = a.root_count[row] + a.scan_tmp[row >> 10];
  for (; m != 0ull && rank < a.capacity; m &= m - 1ull, ++rank) a.acc[rank].key = row * 64u + (uint32_t)__builtin_ctzll(m);
}

// a thread per record: accumulator -> the 96-byte record
__global__ void __launch_bounds__(256) k_bodies_emit(BodyArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.capacity) return;
  const BodyAcc s = a.acc[i];
  BodyPart p;
  p.voxels = s.voxels;
#pragma unroll
  for (int r = 0; r < 3; ++r) { p.inv_lo[r] = s.bounds[r]; p.hi[r] = s.bounds[3 + r]; }
#pragma unroll
  for (uint32_t j = 0; j < kBodySums; ++j) p.s.v[j] = s.sums[j];
  a.records[i] = body_emit(a.group == kBodiesIslands ? s.key : i, p);
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_body_keys(const BodyArgs& a, hipStream_t s) {
  static_assert(kIslandRows % 256u == 0u, "a thread per row");
  if (a.capacity) hipLaunchKernelGGL(k_bodies_keys, dim3(kIslandRows / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}
namespace {
template <uint32_t kGroup>
void launch_group(const BodyArgs& a, hipStream_t s) {
  if (a.weights) hipLaunchKernelGGL((k_bodies<kGroup, true>), dim3(a.box.count()), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_bodies<kGroup, false>), dim3(a.box.count()), dim3(256), 0, s, a);
}
}  // namespace
hipError_t launch_bodies(const BodyArgs& a, hipStream_t s) {
  if (a.capacity == 0u) return hipSuccess;
  switch (a.group) {
    case kBodiesAll: launch_group<kBodiesAll>(a, s); break;
    case kBodiesMaterials: launch_group<kBodiesMaterials>(a, s); break;
    case kBodiesIslands: launch_group<kBodiesIslands>(a, s); break;
    case kBodiesCells: launch_group<kBodiesCells>(a, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_bodies_emit(const BodyArgs& a, hipStream_t s) {
  if (a.capacity) hipLaunchKernelGGL(k_bodies_emit, dim3((a.capacity + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
