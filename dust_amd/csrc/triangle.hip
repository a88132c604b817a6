// triangle.hip -- model voxelisation (dust_hip_model_edit_triangles, _fill_mesh): triangles to voxels on the device, the inverse of
// mesh.hip. Every decision is triangle_rule.hpp, sign tests on int64 values: no float anywhere in this file.
//   k_edit_triangles  the surface rule on k_edit_shapes' skeleton (cell_records.hpp): a workgroup per root cell some triangle's bounds
//                     reach, a wave per 16 bricks, lane = voxel bit, the cell's triangle ids walked once in call order. A triangle's
//                     record and its setup are wave-uniform; a brick is rejected by its brick bounds and then by the same 13-axis test
//                     on the brick's box (wave-uniform too: a branch, no divergence) before any lane tests its voxel.
//   k_fill_columns    the solid rule without atomics: a workgroup per 16 x 16 tile of voxel columns walks the tile's triangle list
//                     (the same binning with z collapsed), a lane per column. A crossing toggles the centres below it, so a lane XORs
//                     one marker bit per crossing into its column's 256 bits -- eight words in registers, the word chosen by
//                     compares -- and the inside bits are the suffix XOR. The tile's columns go through 8 KiB of LDS into brick-mask
//                     layout, and every non-zero brick word is XORed into the context's bit volume with a plain load and store: a
//                     tile has one workgroup per launch and the launches of a call are ordered on the stream, so a word has one owner.
//   k_fill_apply      a workgroup per root cell of the region, a wave per brick: one volume word (wave-uniform), one coalesced 64-byte
//                     read of the brick and, where something changes, one write; covered, changed and the bounds are folded per wave
//                     and leave as at most 8 ordinary vector atomics (integer adds and maxima: no order shows in the result).
// No fences, spins or waits between workgroups.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cell_records.hpp"
#include "triangle.hpp"

namespace dust {

namespace {

__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v = umax(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

// bit z of the result: the XOR of the bits z .. 31 of m
__device__ __forceinline__ uint32_t suffix_xor(uint32_t m) {
  m ^= m >> 1; m ^= m >> 2; m ^= m >> 4; m ^= m >> 8; m ^= m >> 16;
  return m;
}

}  // namespace

__global__ void __launch_bounds__(256) k_edit_triangles(EditTriangleArgs a) {
  walk_cell_records(a, [&](CellBricks& c, uint32_t id) -> uint32_t {
    const DevTriangle s = a.triangles[id];
    const uint32_t lo_x = (s.lo & 255u) >> 2, lo_y = ((s.lo >> 8) & 255u) >> 2, lo_z = (s.lo >> 16) >> 2;
    const uint32_t hi_x = (s.hi & 255u) >> 2, hi_y = ((s.hi >> 8) & 255u) >> 2, hi_z = (s.hi >> 16) >> 2;
    if (c.bx < lo_x || c.bx > hi_x) return 0u;
    const TriangleSetup t = triangle_setup(s.v);
    const Voxel p = brick_voxel(c.bx, c.by0, c.bz0, c.lane);
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t by = c.by0 + (uint32_t)(k >> 2), bz = c.bz0 + (uint32_t)(k & 3);
      if (by < lo_y || by > hi_y || bz < lo_z || bz > hi_z) continue;
      if (!triangle_touches_brick(t, (int32_t)c.bx, (int32_t)by, (int32_t)bz)) continue;  // wave-uniform
      const bool in = triangle_covers(t, (int32_t)p.x, (int32_t)(p.y + (uint32_t)((k >> 2) * 4)), (int32_t)(p.z + (uint32_t)((k & 3) * 4)));
      const uint32_t g = c.v[k];
      const uint32_t to = g ? (s.solid_to == kEditKeep ? g : s.solid_to) : s.empty_to;
      n += c.set(k, in && to != g, to);
    }
    return n;
  });
}

__global__ void __launch_bounds__(256) k_fill_columns(FillColumnsArgs a) {
  __shared__ uint32_t columns[8][257];  // [word][column x << 4 | y of the tile]; a row is padded by a word: the eight words of one
                                        // column, which the lanes of a wave read together below, lie in eight banks
  const uint32_t cell = a.cells[blockIdx.x];  // (x >> 4) << 8 | (y >> 4) << 4
  const uint32_t first = a.cell_start[blockIdx.x], last = a.cell_start[blockIdx.x + 1];
  const uint32_t tx = cell >> 8, ty = (cell >> 4) & 15u;
  const int32_t px = (int32_t)(tx * 16u + (threadIdx.x >> 4)) * kTriangleUnit + kTriangleUnit / 2;
  const int32_t py = (int32_t)(ty * 16u + (threadIdx.x & 15u)) * kTriangleUnit + kTriangleUnit / 2;
  uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0, m6 = 0, m7 = 0;  // marker bit k: a crossing with k + 1 centres below it
  for (uint32_t j = first; j < last; ++j) {
    const uint32_t id = uniform(a.ids[j]);
    const TriangleColumn t = triangle_column(a.triangles[id].v);
    if (!column_crossed(t, px, py)) continue;
    const uint32_t below = crossing_count(t, px, py);
    if (below == 0u) continue;
    const uint32_t w = (below - 1u) >> 5, bit = 1u << ((below - 1u) & 31u);
    m0 ^= w == 0u ? bit : 0u; m1 ^= w == 1u ? bit : 0u; m2 ^= w == 2u ? bit : 0u; m3 ^= w == 3u ? bit : 0u;
    m4 ^= w == 4u ? bit : 0u; m5 ^= w == 5u ? bit : 0u; m6 ^= w == 6u ? bit : 0u; m7 ^= w == 7u ? bit : 0u;
  }
  // centre z is inside iff an odd number of crossings has more than z centres below it: the suffix XOR, from the top word down
  uint32_t odd = 0;
#define DUST_FILL_WORD(W, M)                                   \
  columns[W][threadIdx.x] = suffix_xor(M) ^ (odd ? ~0u : 0u);  \
  odd ^= (uint32_t)__popc(M) & 1u;
  DUST_FILL_WORD(7, m7) DUST_FILL_WORD(6, m6) DUST_FILL_WORD(5, m5) DUST_FILL_WORD(4, m4)
  DUST_FILL_WORD(3, m3) DUST_FILL_WORD(2, m2) DUST_FILL_WORD(1, m1) DUST_FILL_WORD(0, m0)
#undef DUST_FILL_WORD
  __syncthreads();
  // the tile's 4 x 4 x 64 bricks, four per thread: bit x << 4 | y << 2 | z of a brick word from the 16 columns of the brick
#pragma unroll
  for (uint32_t q = 0; q < 4u; ++q) {
    const uint32_t i = q * 256u + threadIdx.x, bz = i & 63u, byl = (i >> 6) & 3u, bxl = i >> 8;
    uint64_t word = 0ull;
#pragma unroll
    for (uint32_t xi = 0; xi < 4u; ++xi)
#pragma unroll
      for (uint32_t yi = 0; yi < 4u; ++yi) {
        const uint32_t column = ((bxl * 4u + xi) << 4) | (byl * 4u + yi);
        const uint32_t nibble = (columns[bz >> 3][column] >> ((bz & 7u) * 4u)) & 15u;
        word |= (uint64_t)nibble << (xi * 16u + yi * 4u);
      }
    if (word != 0ull) a.volume[leaf_code(tx * 4u + bxl, ty * 4u + byl, bz)] ^= word;
  }
}

__global__ void __launch_bounds__(256) k_fill_apply(FillApplyArgs a) {
  __shared__ uint32_t part[4][kFillAccWords];
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  uint32_t covered = 0, changed = 0, lo_x = 0, lo_y = 0, lo_z = 0, hi_x = 0, hi_y = 0, hi_z = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t code = cell * 64u + wave * 16u + k;
    const uint64_t word = uniform64(a.volume[code]);
    if (word == 0ull) continue;
    const Voxel p = code_voxel(code, lane);
    const bool in = ((word >> lane) & 1ull) != 0ull && p.x >= a.lo[0] && p.x <= a.hi[0] && p.y >= a.lo[1] && p.y <= a.hi[1] && p.z >= a.lo[2] && p.z <= a.hi[2];
    if (__ballot(in) == 0ull) continue;
    uint8_t* at = a.grid + (size_t)code * 64u + lane;
    const uint32_t g = *at;
    const uint32_t to = g ? (a.solid_to == kEditKeep ? g : a.solid_to) : a.empty_to;
    if (in) {
      covered += 1u;
      lo_x = umax(lo_x, 255u - p.x); lo_y = umax(lo_y, 255u - p.y); lo_z = umax(lo_z, 255u - p.z);
      hi_x = umax(hi_x, p.x); hi_y = umax(hi_y, p.y); hi_z = umax(hi_z, p.z);
      if (to != g) {
        *at = (uint8_t)to;
        changed += 1u;
      }
    }
  }
  covered = wave_add(covered); changed = wave_add(changed);
  lo_x = wave_umax(lo_x); lo_y = wave_umax(lo_y); lo_z = wave_umax(lo_z);
  hi_x = wave_umax(hi_x); hi_y = wave_umax(hi_y); hi_z = wave_umax(hi_z);
  if (lane == 0u) {
    uint32_t* p = part[wave];
    p[0] = covered; p[1] = changed; p[2] = lo_x; p[3] = lo_y; p[4] = lo_z; p[5] = hi_x; p[6] = hi_y; p[7] = hi_z;
  }
  __syncthreads();
  if (wave == 0u && lane < kFillAccWords) {  // the four partials into one, and one atomic per field that has something to say
    const uint32_t p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
    if (lane < 2u) {
      const uint32_t sum = p0 + p1 + p2 + p3;
      if (sum != 0u) atomicAdd(&a.acc[lane], sum);
    } else {
      const uint32_t most = umax(umax(p0, p1), umax(p2, p3));
      if (most != 0u) atomicMax(&a.acc[lane], most);
    }
  }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_edit_triangles(const EditTriangleArgs& a, hipStream_t s) {
  if (a.n_cells) hipLaunchKernelGGL(k_edit_triangles, dim3(a.n_cells), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_fill_columns(const FillColumnsArgs& a, hipStream_t s) {
  if (a.n_cells) hipLaunchKernelGGL(k_fill_columns, dim3(a.n_cells), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_fill_apply(const FillApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fill_apply, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
