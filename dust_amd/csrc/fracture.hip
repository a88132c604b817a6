// fracture.hip -- model fracture (dust_hip_model_fracture, _fracture_detach, _fracture_apply): every counted voxel of a region takes
// the index of its nearest seed under fracture_rule.hpp's integer metric (k_fracture_label), the cells are described from the labels
// (k_fracture_records, k_fracture_emit), whole cells move into a model of their own (k_fracture_detach) and the seams or the labelled
// voxels take a grid byte (k_fracture_apply). The labels are a brick-major uint16 field (field.hpp looks them up). Everything is
// integer work; what crosses workgroups are ordinary integer atomic adds and maxima, so two runs give the same bytes. No workgroup
// waits for another.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fracture.hpp"

namespace dust {

namespace {

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = umin(v, (uint32_t)__shfl_xor((int)v, d));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = umax(v, (uint32_t)__shfl_xor((int)v, d));
  return v;
}
// sum over the lanes of m of a per-lane count c < 8
__device__ __forceinline__ uint32_t wave_sum3(uint32_t c, uint64_t m) {
  return (uint32_t)__popcll(__ballot(c & 1u) & m) + 2u * (uint32_t)__popcll(__ballot(c & 2u) & m) + 4u * (uint32_t)__popcll(__ballot(c & 4u) & m);
}

// the label of voxel (x, y, z), kFractureNoCell outside the tree
__device__ __forceinline__ uint32_t label_at(const uint16_t* field, int32_t x, int32_t y, int32_t z) {
  if (((uint32_t)x | (uint32_t)y | (uint32_t)z) > 255u) return kFractureNoCell;
  return field[voxel_index((uint32_t)x, (uint32_t)y, (uint32_t)z)];
}
// of a labelled voxel's six face-neighbours: how many are labelled with another cell, and how many with a higher one
__device__ __forceinline__ void face_counts(const uint16_t* field, const Voxel& v, uint32_t label, uint32_t& other, uint32_t& higher) {
  other = higher = 0;
  const int32_t x = (int32_t)v.x, y = (int32_t)v.y, z = (int32_t)v.z;
  const uint32_t n[6] = {label_at(field, x - 1, y, z), label_at(field, x + 1, y, z), label_at(field, x, y - 1, z),
                         label_at(field, x, y + 1, z), label_at(field, x, y, z - 1), label_at(field, x, y, z + 1)};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    other += (n[k] != kFractureNoCell && n[k] != label) ? 1u : 0u;
    higher += (n[k] != kFractureNoCell && n[k] > label) ? 1u : 0u;
  }
}

// what a set of voxels of one brick (a wave-uniform word, not 0) adds to a record: all scalar work
struct BrickStats {
  uint32_t n, lo[3], hi[3];
  unsigned long long sum[3];
};
// one axis of it: the voxels of m in the four planes c = 0..3 (plane0 moved by `shift` bits per plane), from coordinate `base`
__device__ __forceinline__ void axis_stats(uint64_t m, uint64_t plane0, uint32_t shift, uint32_t base, uint32_t n, uint32_t& lo, uint32_t& hi,
                                           unsigned long long& sum) {
  const uint32_t c0 = (uint32_t)__popcll(m & plane0), c1 = (uint32_t)__popcll(m & (plane0 << shift)), c2 = (uint32_t)__popcll(m & (plane0 << (2u * shift))),
                 c3 = (uint32_t)__popcll(m & (plane0 << (3u * shift)));
  lo = base + (c0 ? 0u : (c1 ? 1u : (c2 ? 2u : 3u)));
  hi = base + (c3 ? 3u : (c2 ? 2u : (c1 ? 1u : 0u)));
  sum = (unsigned long long)n * base + c1 + 2u * c2 + 3u * c3;
}
__device__ __forceinline__ BrickStats brick_stats(uint64_t m, uint32_t bx, uint32_t by, uint32_t bz) {
  BrickStats s;
  s.n = (uint32_t)__popcll(m);
  axis_stats(m, kSurfaceX0, 16u, bx * 4u, s.n, s.lo[0], s.hi[0], s.sum[0]);
  axis_stats(m, kSurfaceY0, 4u, by * 4u, s.n, s.lo[1], s.hi[1], s.sum[1]);
  axis_stats(m, kSurfaceZ0, 1u, bz * 4u, s.n, s.lo[2], s.hi[2], s.sum[2]);
  return s;
}

}  // namespace

// One workgroup per root cell of the region's box, four waves of 16 bricks (cell_records.hpp's ownership: wave w owns child bits
// 16 w .. 16 w + 15, lane = voxel bit). The workgroup finds U, the smallest max_d2 of any seed to the cell's part of the region, keeps
// the seeds that pass fracture_candidate in an LDS list of 8-byte entries (int16 x, y, z and the uint16 index: 32 KiB for 4096 seeds)
// -- each wave compacts its quarter of the seeds into its own segment with ballots and popcount prefixes, so no barrier stands inside
// the loop -- and then every wave walks the whole list ONCE with its lane's 16 voxels in registers: the x term is shared by the 16
// bricks, the y and z terms by four each. The order of the list does not show: (d2, index) has one minimum.
__global__ void __launch_bounds__(256) k_fracture_label(FractureArgs a) {
  __shared__ uint2 list[kFractureMaxSeeds];
  __shared__ uint32_t wave_u[4], wave_n[4], wave_live[4];
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  uint32_t bx, by0, bz0;
  cell_brick(cell, wave * 16u, bx, by0, bz0);
  const uint32_t first_code = cell * 64u + wave * 16u;
  // the counted voxels: solid, inside the region, of the filter's material
  uint32_t live = 0, mine = 0, solid = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16u; ++k) {
    uint64_t m = uniform64(a.brick_mask[first_code + k]) & surface_region_mask(bx, by0 + (k >> 2), bz0 + (k & 3u), a.lo, a.hi);
    if (a.byte != 0u && m != 0ull) m &= __ballot(a.grid[(size_t)(first_code + k) * 64u + lane] == a.byte);
    live |= (m != 0ull ? 1u : 0u) << k;
    mine |= (uint32_t)((m >> lane) & 1ull) << k;
    solid += (uint32_t)__popcll(m);
  }
  if (lane == 0u) wave_live[wave] = live;
  __syncthreads();
  if ((wave_live[0] | wave_live[1] | wave_live[2] | wave_live[3]) == 0u) return;  // (the same in every wave: the field is cleared already)

  // U over all seeds, against the cell's box clipped to the region
  FractureBox box;
  const uint32_t c0[3] = {(cell >> 8) * 16u, ((cell >> 4) & 15u) * 16u, (cell & 15u) * 16u};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    box.lo[r] = (int32_t)umax(c0[r], a.lo[r]);
    box.hi[r] = (int32_t)umin(c0[r] + 15u, a.hi[r]);
  }
  uint32_t u = kFractureNoLimit;
  if (a.cull) {
    for (uint32_t i = threadIdx.x; i < a.n_seeds; i += 256u) {
      const DevFractureSeed s = a.seeds[i];
      u = umin(u, fracture_max_d2(a.scale, s.x, s.y, s.z, box));
    }
    u = wave_min(u);
    if (lane == 0u) wave_u[wave] = u;
    __syncthreads();
    u = umin(umin(wave_u[0], wave_u[1]), umin(wave_u[2], wave_u[3]));
  }
  // the candidates: wave w compacts seeds w q .. w q + q - 1 into list[w q ..]
  const uint32_t q = ((a.n_seeds + 255u) / 256u) * 64u;  // 4 q <= kFractureMaxSeeds
  uint32_t kept = 0;
  for (uint32_t base = wave * q; base < wave * q + q; base += 64u) {
    const uint32_t i = base + lane;
    bool pass = false;
    DevFractureSeed s{};
    if (i < a.n_seeds) {
      s = a.seeds[i];
      pass = !a.cull || fracture_candidate(fracture_min_d2(a.scale, s.x, s.y, s.z, box), u, a.limit);
    }
    const uint64_t passed = __ballot(pass);
    if (pass) {
      const uint32_t slot = wave * q + kept + (uint32_t)__popcll(passed & ((1ull << lane) - 1ull));  // < wave q + q <= kFractureMaxSeeds
      list[slot] = make_uint2(((uint32_t)s.x & 0xFFFFu) | ((uint32_t)s.y << 16), ((uint32_t)s.z & 0xFFFFu) | (i << 16));
    }
    kept += (uint32_t)__popcll(passed);
  }
  if (lane == 0u) wave_n[wave] = kept;
  __syncthreads();
  if (live == 0u) return;  // (no barrier below)

  // the walk
  const int32_t vx = (int32_t)(bx * 4u + (lane >> 4));
  int32_t vy[4], vz[4];
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    vy[j] = (int32_t)((by0 + j) * 4u + ((lane >> 2) & 3u));
    vz[j] = (int32_t)((bz0 + j) * 4u + (lane & 3u));
  }
  uint32_t best[16], best_i[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) { best[k] = kFractureNoLimit; best_i[k] = kFractureNoCell; }
  for (uint32_t w = 0; w < 4u; ++w) {
    const uint32_t n = uniform(wave_n[w]);
    for (uint32_t j = 0; j < n; ++j) {
      const uint2 e = list[w * q + j];
      const uint32_t ex = uniform(e.x), ey = uniform(e.y);
      const int32_t sx = (int32_t)(ex << 16) >> 16, sy = (int32_t)ex >> 16, sz = (int32_t)(ey << 16) >> 16;
      const uint32_t index = ey >> 16;
      const uint32_t tx = fracture_term(a.scale[0], vx - sx);
      uint32_t ty[4], tz[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        ty[c] = fracture_term(a.scale[1], vy[c] - sy);
        tz[c] = fracture_term(a.scale[2], vz[c] - sz);
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t d2 = tx + ty[k >> 2] + tz[k & 3];
        const bool better = fracture_before(d2, index, best[k], best_i[k]);
        best[k] = better ? d2 : best[k];
        best_i[k] = better ? index : best_i[k];
      }
    }
  }
  // one coalesced 128-byte row per brick that holds a counted voxel (the others are cleared already)
  uint32_t labelled = 0, far = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16u; ++k) {
    if (((live >> k) & 1u) == 0u) continue;
    const uint32_t label = ((mine >> k) & 1u) ? fracture_label(best[k], best_i[k], a.limit) : kFractureNoCell;
    a.field[(size_t)(first_code + k) * 64u + lane] = (uint16_t)label;
    labelled += (uint32_t)__popcll(__ballot(label != kFractureNoCell));
    if (label != kFractureNoCell) far = umax(far, best[k]);
  }
  far = wave_max(far);
  if (lane == 0u) {
    atomicAdd(&a.acc[kFractureSolid], solid);
    if (labelled) {
      atomicAdd(&a.acc[kFractureLabelled], labelled);
      atomicMax(&a.acc[kFractureMaxD2], far);
    }
  }
}

// The second pass, a workgroup per root cell of the region's box and a wave per 16 bricks: a lane reads its label and its six
// face-neighbours' (across a brick face from the neighbour brick's row; outside the tree there is none), and per distinct label of the
// brick -- the first open lane's label, the ballot of its equals, reduce, clear -- the wave sends one set of vector atomics to that
// cell's accumulator: lanes 0 and 1 the adds, lanes 2..7 the maxima, lanes 8..10 the 64-bit sums. Their number per brick follows the
// distinct labels, not the voxels.
__global__ void __launch_bounds__(256) k_fracture_records(FractureArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  uint32_t bx, by0, bz0;
  cell_brick(cell, wave * 16u, bx, by0, bz0);
  uint32_t cut_once = 0, any = 0;
  uint32_t inv_lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t code = cell * 64u + wave * 16u + k;
    const uint32_t by = by0 + (k >> 2), bz = bz0 + (k & 3u);
    const uint32_t label = a.field[(size_t)code * 64u + lane];
    uint64_t open = __ballot(label != kFractureNoCell);
    if (open == 0ull) continue;
    uint32_t other = 0, higher = 0;
    if (label != kFractureNoCell) face_counts(a.field, brick_voxel(bx, by, bz, lane), label, other, higher);
    cut_once += wave_sum3(higher, open);
    const BrickStats all = brick_stats(open, bx, by, bz);
    any = 1u;
#pragma unroll
    for (int r = 0; r < 3; ++r) { inv_lo[r] = umax(inv_lo[r], 255u - all.lo[r]); hi[r] = umax(hi[r], all.hi[r]); }
    const uint64_t b0 = __ballot(other & 1u), b1 = __ballot(other & 2u), b2 = __ballot(other & 4u);
    while (open != 0ull) {
      const uint32_t cell_index = (uint32_t)__shfl((int)label, (int)__builtin_ctzll(open));  // < n_seeds: written by k_fracture_label
      const uint64_t m = __ballot(label == cell_index);
      open &= ~m;
      const BrickStats s = brick_stats(m, bx, by, bz);
      const uint32_t cut = (uint32_t)__popcll(b0 & m) + 2u * (uint32_t)__popcll(b1 & m) + 4u * (uint32_t)__popcll(b2 & m);
      uint32_t* words = reinterpret_cast<uint32_t*>(a.cells + cell_index);  // voxels, cut_faces, inv_lo[3], hi[3], pad[2], sum[3]
      if (lane < 2u) {
        atomicAdd(words + lane, lane == 0u ? s.n : cut);
      } else if (lane < 8u) {
        const uint32_t v = lane == 2u ? 255u - s.lo[0] : lane == 3u ? 255u - s.lo[1] : lane == 4u ? 255u - s.lo[2] : lane == 5u ? s.hi[0] : lane == 6u ? s.hi[1] : s.hi[2];
        atomicMax(words + lane, v);
      } else if (lane < 11u) {
        const unsigned long long v = lane == 8u ? s.sum[0] : lane == 9u ? s.sum[1] : s.sum[2];
        atomicAdd(reinterpret_cast<unsigned long long*>(words + 10) + (lane - 8u), v);
      }
    }
  }
  if (any && lane == 0u) {
    if (cut_once) atomicAdd(&a.acc[kFractureCut], cut_once);
    for (int r = 0; r < 3; ++r) {
      atomicMax(&a.acc[kFractureLo + r], inv_lo[r]);
      atomicMax(&a.acc[kFractureHi + r], hi[r]);
    }
  }
}

// a thread per cell: the 40-byte record, the number of cells that hold a voxel, and the largest cell as one 64-bit maximum
__global__ void __launch_bounds__(256) k_fracture_emit(FractureArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  uint32_t voxels = 0;
  if (i < a.n_seeds) {
    const FractureAcc s = a.cells[i];
    DevFractureCell r;
    r.voxels = voxels = s.voxels;
    r.cut_faces = s.cut_faces;
    r.lo = (255u - s.inv_lo[0]) | ((255u - s.inv_lo[1]) << 8) | ((255u - s.inv_lo[2]) << 16);
    r.hi = s.hi[0] | (s.hi[1] << 8) | (s.hi[2] << 16);
    for (int k = 0; k < 3; ++k) { r.sum[2 * k] = (uint32_t)s.sum[k]; r.sum[2 * k + 1] = (uint32_t)(s.sum[k] >> 32); }
    a.records[i] = r;
  }
  const uint32_t filled = (uint32_t)__popcll(__ballot(voxels != 0u));
  // the wave's largest (voxels, ~index): first the voxels, then the lowest index among the lanes that hold them
  const uint32_t most = wave_max(voxels);
  const uint32_t rank = wave_max(voxels == most && voxels != 0u ? 0xFFFFFFFFu - i : 0u);
  if (lane == 0u && filled) {
    atomicAdd(&a.acc[kFractureCells], filled);
    atomicMax(reinterpret_cast<unsigned long long*>(a.acc + kFractureLargest), ((unsigned long long)most << 32) | rank);
  }
}

// a wavefront per brick, launch_island_detach's copy and carve with the test selected[label]: the voxels of the selected cells go to dst
// (every other byte of dst is cleared) and, with `carve`, leave the source and its labelling
__global__ void __launch_bounds__(256) k_fracture_detach(FractureDetachArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t code = blockIdx.x * 4u + (threadIdx.x >> 6);  // < kLattice: the grid is kLattice / 4 workgroups
  const size_t at = (size_t)code * 64u + lane;
  const uint8_t g = a.src[at];
  const uint32_t label = a.field[at];  // < kFractureMaxSeeds or kFractureNoCell
  const bool moves = g != 0 && label != kFractureNoCell && ((a.selected[label >> 6] >> (label & 63u)) & 1ull) != 0ull;
  if (a.dst) a.dst[at] = moves ? g : (uint8_t)0;
  if (a.carve && moves) {
    a.src[at] = 0;
    a.field[at] = (uint16_t)kFractureNoCell;
  }
}

// a workgroup per root cell of the box, a wave per 16 bricks; only the grid is written, so every decision sees the labelling as it stands
__global__ void __launch_bounds__(256) k_fracture_apply(FractureApplyArgs a) {
  const uint32_t cell = a.box.cell(blockIdx.x);
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  uint32_t bx, by0, bz0;
  cell_brick(cell, wave * 16u, bx, by0, bz0);
  uint32_t n = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    const size_t at = ((size_t)cell * 64u + wave * 16u + k) * 64u + lane;
    const uint32_t label = a.field[at];
    if (__ballot(label != kFractureNoCell) == 0ull) continue;
    bool chosen = label != kFractureNoCell;
    if (chosen && a.seams) {
      uint32_t other, higher;
      face_counts(a.field, brick_voxel(bx, by0 + (k >> 2), bz0 + (k & 3u), lane), label, other, higher);
      chosen = higher != 0u;
    }
    const bool differs = chosen && a.grid[at] != a.byte;
    if (differs) a.grid[at] = (uint8_t)a.byte;
    n += (uint32_t)__popcll(__ballot(differs));
  }
  if (n && lane == 0u) atomicAdd(a.changed, n);
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_fracture_label(const FractureArgs& a, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(a.field, 0xFF, (size_t)kLattice * 64u * sizeof(uint16_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_fracture_label, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_fracture_records(const FractureArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fracture_records, dim3(a.box.count()), dim3(256), 0, s, a);
  if (a.n_seeds) hipLaunchKernelGGL(k_fracture_emit, dim3((a.n_seeds + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_fracture_detach(const FractureDetachArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fracture_detach, dim3(kLattice / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_fracture_apply(const FractureApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fracture_apply, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
