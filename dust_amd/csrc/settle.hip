// settle.hip -- model settling (dust_hip_model_settle, _settle_apply): the loose voxels of a region fall along an axis until they rest
// on a fixed voxel, on each other or on the region's floor, and slide one step sideways and down where a 45 degree slope is free.
// What is loose is a second set of brick masks beside EditArgs::brick_mask (2 MiB, the loose voxels of every brick), made from the grid
// bytes by k_settle_masks -- or the brick masks themselves when every palette index is loose. With it every decision is made from
// masks alone; grid bytes are touched only to move them.
//   k_settle         counts what one fall would do, in k_columns' shape: a workgroup per root-cell column of the (u, v) plane, a lane per
//                    voxel column, the column's 256 solid and 256 loose bits gathered four at a time from the bricks it crosses and
//                    handed to settle_rule.hpp. Every wave folds its 14-word record with cross-lane sums and maxima, the four waves
//                    fold theirs through LDS at one barrier, and at most 14 ordinary vector atomics leave per workgroup.
//   k_settle_fall    the same walk and the same record, then the move: a lane visits its column's voxels in ascending order and
//                    carries each loose byte down to its destination, which is never above a voxel not yet visited -- in place, no
//                    copy. A lane reads and writes only its own column. It leaves the masks stale: k_settle_masks runs behind it.
//   k_settle_slide   a workgroup per root cell, a wave per brick, lane = voxel bit. The brick's and its eight neighbours' words in the
//                    plane of the slide and the fall (solid, loose, region: 27 wave-uniform words) go through settle_slide and come
//                    back as two words: who leaves, who arrives. A voxel that arrives fetches its source's byte from the grid that is
//                    read; a voxel that leaves writes 0; the brick's 64 bytes and its two words go to the OTHER grid and masks. No
//                    atomics on voxels.
//   k_settle_masks   a wave per brick: two ballots over the brick's 64 bytes.
// Everything is integer: no order shows in any result. No fences, spins or waits BETWEEN workgroups; no kernel uses scratch.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "settle.hpp"
#include "settle_rule.hpp"
#include "surface.hpp"  // surface_axis_bounds

namespace dust {

namespace {

// coordinate c on the axis, u and v in the plane -> x, y, z (column_u_axis, column_v_axis)
__device__ __forceinline__ void place(uint32_t axis, uint32_t c, uint32_t u, uint32_t v, uint32_t& x, uint32_t& y, uint32_t& z) {
  x = axis == 0u ? c : v;
  y = axis == 1u ? c : (axis == 0u ? v : u);
  z = axis == 2u ? c : u;
}
__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v = umax(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}
// the leaf_code bits of brick coordinate b on the axis alone
__device__ __forceinline__ uint32_t axis_code(uint32_t axis, uint32_t b) {
  uint32_t bx, by, bz;
  place(axis, b, 0u, 0u, bx, by, bz);
  return leaf_code(bx, by, bz);
}

// the four partial records of a workgroup into one, and one atomic per word that has something to say
__device__ __forceinline__ void flush_records(const uint32_t (*part)[kSettleAccWords], uint32_t* acc, uint32_t wave, uint32_t lane) {
  __syncthreads();
  if (wave == 0u && lane < kSettleAccWords) {
    const uint32_t p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
    if (lane < kSettleAccSums) {
      const uint32_t sum = p0 + p1 + p2 + p3;
      if (sum != 0u) atomicAdd(&acc[lane], sum);
    } else {
      const uint32_t most = umax(umax(p0, p1), umax(p2, p3));
      if (most != 0u) atomicMax(&acc[lane], most);
    }
  }
}

// One voxel column per lane: gathered, turned so that position 0 is the end things fall toward, handed to settle_fall; with kMove the
// bytes are moved too. A lane outside the region loads nothing and has the empty column.
template <bool kMove>
__device__ __forceinline__ void settle_columns(const SettleArgs& a, uint32_t (*part)[kSettleAccWords]) {
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t u = (a.cell_u + blockIdx.x % a.cells_u) * 16u + (threadIdx.x & 15u);
  const uint32_t v = (a.cell_v + blockIdx.x / a.cells_u) * 16u + (threadIdx.x >> 4);
  const bool inside = u >= a.lo_u && u <= a.hi_u && v >= a.lo_v && v <= a.hi_v;
  uint32_t x, y, z;
  place(a.axis, 0u, u >> 2, v >> 2, x, y, z);
  const uint32_t code = leaf_code(x, y, z);  // of the column's brick with brick coordinate 0 on the axis
  place(a.axis, 0u, u & 3u, v & 3u, x, y, z);
  const uint32_t off = voxel_bit(x, y, z);   // of its voxel with coordinate 0 (mod 4) on the axis
  const uint32_t stride = 16u >> (2u * a.axis);
  const bool all_loose = a.loose_mask == a.brick_mask;  // uniform: kernel arguments
  const uint32_t b_lo = a.lo_n >> 2, b_hi = a.hi_n >> 2;
  Column raw_solid, raw_loose;
#pragma unroll
  for (uint32_t w = 0; w < 4u; ++w) {
    uint64_t solid = 0ull, loose = 0ull;
    const uint32_t first = umax(b_lo, 16u * w), last = umin(b_hi, 16u * w + 15u);
    if (inside) {
      for (uint32_t b = first; b <= last; ++b) {  // (uniform bounds; empty where the region does not reach this word)
        const uint32_t at = code | axis_code(a.axis, b);
        const uint32_t nib = column_nibble(a.brick_mask[at], off, stride);
        if (nib == 0u) continue;
        solid |= (uint64_t)nib << (4u * (b & 15u));
        loose |= (uint64_t)(all_loose ? nib : column_nibble(a.loose_mask[at], off, stride)) << (4u * (b & 15u));
      }
    }
    raw_solid.w[w] = solid;
    raw_loose.w[w] = loose;
  }
  const bool from_high = a.from_high != 0u;
  const Column loose = column_turn(raw_loose, a.lo_n, a.hi_n, from_high);
  const Column solid = column_turn(raw_solid, a.lo_n, a.hi_n, from_high);
  const Column fixed = column_xor(solid, loose);  // (loose is a subset of solid)
  const SettleFall f = settle_fall(loose, fixed);
  const Column turned = column_xor(loose, f.now);  // the positions that turn solid or empty
  const uint32_t changed = column_count(turned);
  uint32_t lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};  // (lo as 255 - the bound)
  if (changed != 0u) {
    const uint32_t c0 = column_coord(column_first(turned), a.lo_n, a.hi_n, from_high), c1 = column_coord(column_last(turned), a.lo_n, a.hi_n, from_high);
    place(a.axis, umin(c0, c1), u, v, x, y, z);
    lo[0] = 255u - x; lo[1] = 255u - y; lo[2] = 255u - z;
    place(a.axis, umax(c0, c1), u, v, hi[0], hi[1], hi[2]);
  }
  if (kMove) {
    settle_walk(loose, fixed, [&](uint32_t from, uint32_t to) {
      const uint32_t cf = column_coord(from, a.lo_n, a.hi_n, from_high), ct = column_coord(to, a.lo_n, a.hi_n, from_high);
      const size_t at_from = (size_t)(code | axis_code(a.axis, cf >> 2)) * 64u + off + (cf & 3u) * stride;
      const size_t at_to = (size_t)(code | axis_code(a.axis, ct >> 2)) * 64u + off + (ct & 3u) * stride;
      a.grid[at_to] = a.grid[at_from];
      a.grid[at_from] = 0;
    });
  }
  // the wave's partial record (a lane outside the region adds nothing: its column is empty)
  const uint32_t columns = (uint32_t)__popcll(__ballot(f.moved != 0u));
  const uint32_t s_loose = wave_add(f.loose), s_fixed = wave_add(f.fixed), s_moved = wave_add(f.moved), s_changed = wave_add(changed);
  const uint32_t s_fall = wave_add(f.fall_sum), m_fall = wave_umax(f.fall_max);
  const uint32_t lo_x = wave_umax(lo[0]), lo_y = wave_umax(lo[1]), lo_z = wave_umax(lo[2]);
  const uint32_t hi_x = wave_umax(hi[0]), hi_y = wave_umax(hi[1]), hi_z = wave_umax(hi[2]);
  if (lane == 0u) {
    uint32_t* p = part[wave];
    p[0] = s_loose; p[1] = s_fixed; p[2] = s_moved; p[3] = s_changed; p[4] = s_fall; p[5] = columns; p[kSettleSlid] = 0u;
    p[kSettleFallMax] = m_fall;
    p[kSettleLo] = lo_x; p[kSettleLo + 1] = lo_y; p[kSettleLo + 2] = lo_z;
    p[kSettleHi] = hi_x; p[kSettleHi + 1] = hi_y; p[kSettleHi + 2] = hi_z;
  }
  flush_records(part, a.acc, wave, lane);
}

__device__ __forceinline__ uint64_t lane_word(uint64_t v, int lane) {  // lane `lane`'s value, wave-uniform (lane is a constant)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

}  // namespace

__global__ void __launch_bounds__(256) k_settle(SettleArgs a) {
  __shared__ uint32_t part[4][kSettleAccWords];
  settle_columns<false>(a, part);
}

__global__ void __launch_bounds__(256) k_settle_fall(SettleArgs a) {
  __shared__ uint32_t part[4][kSettleAccWords];
  settle_columns<true>(a, part);
}

__global__ void __launch_bounds__(256) k_settle_slide(SettleSlideArgs a) {
  __shared__ uint32_t part[4][kSettleAccWords];
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  SettleDirs dirs;
  dirs.d = settle_axis(a.d_axis); dirs.g = settle_axis(a.g_axis);
  dirs.d_up = a.d_up != 0u; dirs.g_up = a.g_up != 0u;
  // this lane's word of the 27: lane = 9 * kind + 3 * (i + 1) + (j + 1), kind 0 solid, 1 loose, 2 region; the brick i bricks along d and
  // j bricks along g
  const uint32_t kind = lane / 9u;
  const int step_d = ((int)(lane % 9u) / 3 - 1) * (dirs.d_up ? 1 : -1), step_g = ((int)(lane % 3u) - 1) * (dirs.g_up ? 1 : -1);
  const int off_x = (a.d_axis == 0u ? step_d : 0) + (a.g_axis == 0u ? step_g : 0);
  const int off_y = (a.d_axis == 1u ? step_d : 0) + (a.g_axis == 1u ? step_g : 0);
  const int off_z = (a.d_axis == 2u ? step_d : 0) + (a.g_axis == 2u ? step_g : 0);
  // the source of a voxel that arrives: v - d - g
  const int src_x = (a.d_axis == 0u ? (dirs.d_up ? -1 : 1) : 0) + (a.g_axis == 0u ? (dirs.g_up ? -1 : 1) : 0);
  const int src_y = (a.d_axis == 1u ? (dirs.d_up ? -1 : 1) : 0) + (a.g_axis == 1u ? (dirs.g_up ? -1 : 1) : 0);
  const int src_z = (a.d_axis == 2u ? (dirs.d_up ? -1 : 1) : 0) + (a.g_axis == 2u ? (dirs.g_up ? -1 : 1) : 0);
  uint32_t slid = 0;   // of the wave (uniform)
  bool turned_any = false;  // a brick may only lose voxels to bricks of other waves: its bounds count all the same
  uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u};
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t c = wave * 16u + k, code = cell * 64u + c;
    uint32_t bx, by, bz;
    cell_brick(cell, c, bx, by, bz);
    if (surface_region_mask(bx, by, bz, a.lo, a.hi) == 0ull) continue;  // (outside the region: both grids hold it already)
    uint64_t mine = 0ull;
    if (lane < 27u) {
      const uint32_t nx = bx + (uint32_t)off_x, ny = by + (uint32_t)off_y, nz = bz + (uint32_t)off_z;  // (-1 wraps to above 63: off the tree)
      if (nx < 64u && ny < 64u && nz < 64u) {
        if (kind == 2u) mine = surface_region_mask(nx, ny, nz, a.lo, a.hi);
        else mine = (kind == 0u ? a.brick_mask : a.loose_mask)[leaf_code(nx, ny, nz)];
      }
    }
    if (__ballot(lane < 9u && mine != 0ull) == 0ull) {  // nothing here and nothing that could arrive
      a.grid_out[(size_t)code * 64u + lane] = 0;
      if (lane == 0u) { a.mask_out[code] = 0ull; a.loose_out[code] = 0ull; }
      continue;
    }
    SettleBricks n;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      n.occ[i / 3][i % 3] = lane_word(mine, i);
      n.loose[i / 3][i % 3] = lane_word(mine, 9 + i) & n.occ[i / 3][i % 3];
      n.region[i / 3][i % 3] = lane_word(mine, 18 + i);
    }
    const SettleSlide s = settle_slide(n, dirs);
    const uint64_t own = n.occ[1][1];
    uint32_t byte = own != 0ull ? (uint32_t)a.grid[(size_t)code * 64u + lane] : 0u;
    if ((s.leave >> lane) & 1ull) byte = 0u;
    if ((s.arrive >> lane) & 1ull) {
      const Voxel v = brick_voxel(bx, by, bz, lane);
      const uint32_t sx = v.x + (uint32_t)src_x, sy = v.y + (uint32_t)src_y, sz = v.z + (uint32_t)src_z;
      if (sx < 256u && sy < 256u && sz < 256u) byte = a.grid[voxel_index(sx, sy, sz)];  // (always: the source lies in the region)
    }
    a.grid_out[(size_t)code * 64u + lane] = (uint8_t)byte;
    if (lane == 0u) {
      a.mask_out[code] = (own & ~s.leave) | s.arrive;
      a.loose_out[code] = (n.loose[1][1] & ~s.leave) | s.arrive;
    }
    slid += (uint32_t)__popcll(s.arrive);
    const uint64_t turned = s.leave | s.arrive;
    turned_any |= turned != 0ull;
    surface_axis_bounds(turned, kSurfaceX0, 16u, bx * 4u, lo[0], hi[0]);
    surface_axis_bounds(turned, kSurfaceY0, 4u, by * 4u, lo[1], hi[1]);
    surface_axis_bounds(turned, kSurfaceZ0, 1u, bz * 4u, lo[2], hi[2]);
  }
  if (lane < kSettleAccWords) part[wave][lane] = 0u;
  if (lane == 0u && turned_any) {  // the wave's partial record (hi >= lo then)
    uint32_t* p = part[wave];
    p[kSettleSlid] = slid;
    p[kSettleLo] = 255u - lo[0]; p[kSettleLo + 1] = 255u - lo[1]; p[kSettleLo + 2] = 255u - lo[2];
    p[kSettleHi] = hi[0]; p[kSettleHi + 1] = hi[1]; p[kSettleHi + 2] = hi[2];
  }
  flush_records(part, a.acc, wave, lane);
}

__global__ void __launch_bounds__(256) k_settle_masks(SettleMaskArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t code = cell * 64u + wave * 16u + k;
    const uint32_t byte = a.grid[(size_t)code * 64u + lane];
    const uint32_t index = (byte - 1u) & 255u;
    uint32_t word = 0u;  // the word of the loose mask that holds the index (selected, not indexed: the mask stays in scalar registers)
#pragma unroll
    for (uint32_t w = 0; w < 8u; ++w)
      if ((index >> 5) == w) word = a.loose[w];
    const uint64_t solid = __ballot(byte != 0u);
    const uint64_t loose = __ballot(byte != 0u && ((word >> (index & 31u)) & 1u) != 0u);
    if (lane == 0u) {
      if (a.brick_mask) a.brick_mask[code] = solid;
      a.loose_mask[code] = loose;
    }
  }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_settle(const SettleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_settle, dim3(a.cells_u * a.cells_v), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_settle_fall(const SettleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_settle_fall, dim3(a.cells_u * a.cells_v), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_settle_slide(const SettleSlideArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_settle_slide, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_settle_masks(const SettleMaskArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_settle_masks, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
