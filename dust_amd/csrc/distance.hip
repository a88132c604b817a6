// distance.hip -- exact distance from every voxel of an editable hierarchy!(4,2,2) model to the nearest solid or empty voxel
// (dust_hip_model_distance, dust_hip_model_distance_at, dust_hip_model_distance_apply; the contract is in include/dust_hip.h).
//
// The field is a uint16 per voxel, brick-major like the grid (edit.hpp EditArgs::grid): a 4^3 brick is 128 contiguous bytes, the value
// of voxel bit x << 4 | y << 2 | z at leaf_code(bx, by, bz) * 64 + bit. The transform is integer and separable: three in-place passes,
// x then y then z, and in each pass every line of 256 voxels along the pass axis is independent of every other. A BRICK COLUMN along
// the axis is 64 bricks = 16 lines = 4096 values; one workgroup of four waves owns one column (4096 workgroups per pass), loads it into
// LDS a brick row (one coalesced 128-byte wave access) at a time, works on it and writes the same rows back:
//   k_distance_bits    pass x. No field is read: a brick's targets are its 64-bit occupancy (EditArgs::brick_mask, complemented under
//                      TO_EMPTY; under TO_MATERIAL a ballot over the brick's grid bytes). A line's 256 target bits are four ballots, a
//                      lane's value the distance to the nearest set bit by count-leading / count-trailing zeros on the 64-bit words
//   k_distance_scan    passes y and z. lane = one output voxel, a wave takes 64 consecutive positions of a line. Each lane computes
//                      min over |k| <= R of combine(line[i + k], k), combine = g + k^2 (EUCLIDEAN) or max(g, |k|) (CHEBYSHEV), walking k
//                      outward from 0 and stopping once k^2 (k) is no smaller than every lane's current best: no candidate further out
//                      can lower any lane, so the bytes are those of the full window. A line without a finite value is skipped by one
//                      wave vote. Values above the limit become FAR after every pass (a nearest target within R has every per-axis
//                      offset within R). The last pass folds WALLS into its store
//   k_distance_result  a wave per 16 bricks: ballots for the counts, one 64-bit maximum of value << 32 | (0xFFFFFF - key) per wave
// (dust_hip_model_distance_at and _distance_apply: field.hip)
// A workgroup reads and writes only its own column, so nothing is ordered between workgroups: no fences, no spins, and everything is
// integer -- two runs give the same bytes.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "distance.hpp"
#include "edit.hpp"
#include "field.hpp"

namespace dust {

namespace {

constexpr uint32_t kPad = 256;                 // FAR values on either side of a line in LDS: line[i +- k] needs no bounds check (k <= 255)
constexpr uint32_t kStride = 256 + 2 * kPad + 4;  // uint16 per line; 386 dwords: the 16 lines of a brick row fall into 32 different banks
constexpr uint32_t kNoBit = 1024;              // farther than any bit of a line

// brick b of the column (u, v) along `axis`: u, v are the brick coordinates on the other two axes, in x, y, z order
__device__ __forceinline__ uint32_t column_brick(uint32_t axis, uint32_t b, uint32_t u, uint32_t v) {
  return axis == 0u ? leaf_code(b, u, v) : axis == 1u ? leaf_code(u, b, v) : leaf_code(u, v, b);
}
// a voxel bit's coordinate along the axis, and its line: the two other coordinates, (p << 2) | q in x, y, z order
__device__ __forceinline__ uint32_t bit_along(uint32_t axis, uint32_t bit) { return (bit >> (4u - 2u * axis)) & 3u; }
__device__ __forceinline__ uint32_t bit_line(uint32_t axis, uint32_t bit) {
  const uint32_t s = 4u - 2u * axis;
  return ((bit >> (s + 2u)) << s) | (bit & ((1u << s) - 1u));
}

// the column's 64 brick rows, LDS -> field: wave w takes bricks w, w + 4, ...; lane = voxel bit
__device__ __forceinline__ void store_column(uint16_t* field, const uint16_t* col, uint32_t axis, uint32_t u, uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t at = bit_line(axis, lane) * kStride + kPad + bit_along(axis, lane);
  for (uint32_t j = 0; j < 16u; ++j) {
    const uint32_t b = j * 4u + wave;
    field[(size_t)column_brick(axis, b, u, v) * 64u + lane] = col[at + b * 4u];
  }
}

}  // namespace

__global__ void __launch_bounds__(256) k_distance_bits(DistanceArgs a) {
  __shared__ uint16_t col[16 * kStride];
  __shared__ uint64_t mask[64];  // per brick of the column: its target voxels
  const uint32_t u = blockIdx.x >> 6, v = blockIdx.x & 63u;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (a.target == kDistanceToMaterial) {
    for (uint32_t j = 0; j < 16u; ++j) {
      const uint32_t b = j * 4u + wave;
      const uint64_t m = __ballot((uint32_t)a.grid[(size_t)leaf_code(b, u, v) * 64u + lane] == a.byte);
      if (lane == 0u) mask[b] = m;
    }
  } else if (threadIdx.x < 64u) {
    const uint64_t m = a.brick_mask[leaf_code(threadIdx.x, u, v)];
    mask[threadIdx.x] = a.target == kDistanceToEmpty ? ~m : m;
  }
  __syncthreads();
  for (uint32_t n = 0; n < 4u; ++n) {
    const uint32_t line = wave * 4u + n;  // y << 2 | z inside the brick: the low four bits of a voxel bit
    uint64_t w[4];                         // the line's 256 target bits (wave-uniform)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t i = (uint32_t)p * 64u + lane;
      w[p] = __ballot(((mask[i >> 2] >> (((i & 3u) << 4) | line)) & 1ull) != 0ull);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      // the nearest set bit at or below position i = p * 64 + lane, and at or above it
      uint32_t d_lo = kNoBit, d_hi = kNoBit;
#pragma unroll
      for (int pp = 0; pp < p; ++pp)  // (the last word that holds a bit is the nearest)
        if (w[pp] != 0ull) d_lo = lane + (uint32_t)(p - pp) * 64u - 63u + (uint32_t)__builtin_clzll(w[pp]);
#pragma unroll
      for (int pp = 3; pp > p; --pp)
        if (w[pp] != 0ull) d_hi = (uint32_t)(pp - p) * 64u + (uint32_t)__builtin_ctzll(w[pp]) - lane;
      const uint64_t below = w[p] & (~0ull >> (63u - lane)), above = w[p] >> lane;
      if (below != 0ull) d_lo = lane - 63u + (uint32_t)__builtin_clzll(below);
      if (above != 0ull) d_hi = (uint32_t)__builtin_ctzll(above);
      const uint32_t d = umin(d_lo, d_hi);
      const uint32_t value = d > a.radius ? kFieldNone : a.metric == kDistanceEuclidean ? d * d : d;
      col[line * kStride + kPad + (uint32_t)p * 64u + lane] = (uint16_t)value;
    }
  }
  __syncthreads();
  store_column(a.field, col, 0u, u, v);
}

// axis 1 or 2; last: the pass whose store folds WALLS
__global__ void __launch_bounds__(256) k_distance_scan(DistanceArgs a, uint32_t axis, uint32_t last) {
  __shared__ uint16_t col[16 * kStride];
  const uint32_t u = blockIdx.x >> 6, v = blockIdx.x & 63u;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t t = threadIdx.x; t < 16u * 2u * kPad; t += 256u) {  // the pads of the 16 lines
    const uint32_t r = t & (2u * kPad - 1u);
    col[(t / (2u * kPad)) * kStride + (r < kPad ? r : r + 256u)] = (uint16_t)kFieldNone;
  }
  {
    const uint32_t at = bit_line(axis, lane) * kStride + kPad + bit_along(axis, lane);
    for (uint32_t j = 0; j < 16u; ++j) {
      const uint32_t b = j * 4u + wave;
      col[at + b * 4u] = a.field[(size_t)column_brick(axis, b, u, v) * 64u + lane];
    }
  }
  __syncthreads();
  const uint32_t radius = a.radius, limit = a.limit;
  for (uint32_t n = 0; n < 4u; ++n) {
    const uint32_t l = wave * 4u + n;  // this wave alone reads and writes the line
    uint16_t* line = col + l * kStride + kPad;
    uint32_t out[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) out[p] = line[(uint32_t)p * 64u + lane];
    const bool finite = out[0] != kFieldNone || out[1] != kFieldNone || out[2] != kFieldNone || out[3] != kFieldNone;
    if (__any(finite)) {  // (a line of FAR stays FAR)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint16_t* at = line + (uint32_t)p * 64u + lane;
        uint32_t best = out[p];
        if (a.metric == kDistanceEuclidean) {
          for (uint32_t k = 1; k <= radius; ++k) {
            const uint32_t kk = k * k;
            if (!__any(kk < best)) break;  // no lane of the wave can still be lowered
            best = umin(best, umin(at[-(int)k], at[k]) + kk);  // (FAR + k^2 is above every value)
          }
        } else {
          for (uint32_t k = 1; k <= radius; ++k) {
            if (!__any(k < best)) break;
            best = umin(best, umax(umin(at[-(int)k], at[k]), k));
          }
        }
        out[p] = best > limit ? kFieldNone : best;
      }
    }
    if (last != 0u && a.walls != 0u) {
      // the nearest voxel outside the tree lies straight across the nearest face, w voxels away
      const uint32_t c1 = u * 4u + (l >> 2), c2 = v * 4u + (l & 3u);
      const uint32_t w12 = umin(umin(c1 + 1u, 256u - c1), umin(c2 + 1u, 256u - c2));
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t i = (uint32_t)p * 64u + lane;
        const uint32_t w = umin(w12, umin(i + 1u, 256u - i));
        const uint32_t value = w > radius ? kFieldNone : a.metric == kDistanceEuclidean ? w * w : w;
        out[p] = umin(out[p], value);
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) line[(uint32_t)p * 64u + lane] = (uint16_t)out[p];
  }
  __syncthreads();
  store_column(a.field, col, axis, u, v);
}

// a workgroup per root cell (64 bricks contiguous in the field), a wave per 16 bricks
__global__ void __launch_bounds__(256) k_distance_result(DistanceArgs a) {
  __shared__ DistanceAcc sum;
  if (threadIdx.x == 0u) { sum.best = 0ull; sum.targets = 0u; sum.far = 0u; }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t targets = 0, far = 0;
  unsigned long long best = 0ull;
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t code = blockIdx.x * 64u + wave * 16u + k;
    const uint32_t value = a.field[(size_t)code * 64u + lane];
    targets += (uint32_t)__popcll(__ballot(value == 0u));
    far += (uint32_t)__popcll(__ballot(value == kFieldNone));
    if (value != kFieldNone) {
      const uint32_t key = code_voxel(code, lane).key();
      const unsigned long long packed = ((unsigned long long)value << 32) | (unsigned long long)(0xFFFFFFu - key);
      best = packed > best ? packed : best;
    }
  }
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) {
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), step), lo = (uint32_t)__shfl_xor((int)(uint32_t)best, step);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    best = other > best ? other : best;
  }
  if (lane == 0u) {  // integer sums and maxima: the order does not matter
    if (targets) atomicAdd(&sum.targets, targets);
    if (far) atomicAdd(&sum.far, far);
    if (best) atomicMax(&sum.best, best);
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    if (sum.targets) atomicAdd(&a.acc->targets, sum.targets);
    if (sum.far) atomicAdd(&a.acc->far, sum.far);
    if (sum.best) atomicMax(&a.acc->best, sum.best);
  }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_distance_field(const DistanceArgs& a, hipStream_t s) {
  const dim3 columns(64 * 64), cells(kLattice / 64), block(256);
  hipLaunchKernelGGL(k_distance_bits, columns, block, 0, s, a);
  hipLaunchKernelGGL(k_distance_scan, columns, block, 0, s, a, 1u, 0u);
  hipLaunchKernelGGL(k_distance_scan, columns, block, 0, s, a, 2u, 1u);
  hipLaunchKernelGGL(k_distance_result, cells, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
