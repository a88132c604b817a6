// column.hip -- model columns (dust_hip_model_columns, _columns_apply): for every voxel column along an axis, where run `layer` of the
// solid starts, how long it is and how many runs the column has; and the edit that writes into those runs or into the gaps in front of
// them. A walk reads the brick masks (EditArgs::brick_mask, 2 MiB) and nothing else without a palette filter: a column of 256 voxels
// is 256 bits, gathered four at a time from the 64 bricks it crosses (fewer under a region) and handed to column_rule.hpp, which is
// shifts, popcounts and counts of zeros. A grid byte is read for the hit voxel's palette (a map or the table is asked for), for the
// voxels a filter has to judge, and by the apply's stores.
//
// Both kernels have one shape: a workgroup per root-cell column the region reaches in the (u, v) plane, 256 lanes, a lane per voxel
// column -- u = lane & 15 fastest, so a wave is four brick columns adjacent along u by one brick along v, 16 lanes load one mask word,
// and a wave writes the map as four 64-byte row segments. (The other shape, a lane per brick along the axis with the column's bits
// made wave-uniform by four ballots, was not built: it leaves 64 waves per root-cell column where this one has 4, and its map stores
// are one word per wave.)
//   k_columns        every wave folds hit columns (a ballot's popcount), voxels, runs, depths, the nearest and farthest key words and
//                    the bounds with cross-lane sums and maxima; the four waves fold their 12-word partial records through LDS at one
//                    barrier, and at most 12 ordinary vector atomics (adds and maxima) leave per workgroup. The table is 1 KiB of LDS,
//                    one LDS add per column, flushed non-zero bins only.
//   k_columns_apply  a lane writes only voxels of its own column, after the walk has read all it needs of that column (the masks,
//                    which nothing writes before the rebuild, and under a filter the column's own grid bytes): what is written is
//                    decided on the model as it stood when the call began, without a copy.
// (Integer atomic rates are unmeasured on this chip, so their number is kept small rather than budgeted.) Everything is integer: no
// order shows in any result. No fences, spins or waits BETWEEN workgroups.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "column.hpp"
#include "column_rule.hpp"

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

// the voxel column of a lane: thread t of workgroup `group`
struct ColumnLane {
  uint32_t u, v;
  bool inside;    // the column lies in the region
  uint32_t code;  // leaf_code of its brick with brick coordinate 0 on the axis: a brick's code is this | the axis's own bits
  uint32_t off;   // the voxel bit of its voxel with coordinate 0 (mod 4) on the axis
};
__device__ __forceinline__ ColumnLane column_lane(const ColumnArgs& a, uint32_t group, uint32_t t) {
  ColumnLane l;
  l.u = (a.cell_u + group % a.cells_u) * 16u + (t & 15u);
  l.v = (a.cell_v + group / a.cells_u) * 16u + (t >> 4);
  l.inside = l.u >= a.lo_u && l.u <= a.hi_u && l.v >= a.lo_v && l.v <= a.hi_v;
  uint32_t x, y, z;
  place(a.axis, 0u, l.u >> 2, l.v >> 2, x, y, z);
  l.code = leaf_code(x, y, z);
  place(a.axis, 0u, l.u & 3u, l.v & 3u, x, y, z);
  l.off = voxel_bit(x, y, z);
  return l;
}

// The lane's column under the query -- clipped to the region, turned, filtered -- and its run `layer`. A lane outside the region
// loads nothing and has the empty column.
__device__ __forceinline__ ColumnRun column_walk(const ColumnArgs& a, const ColumnLane& l) {
  const uint32_t stride = 16u >> (2u * a.axis);
  const uint32_t b_lo = a.lo_n >> 2, b_hi = a.hi_n >> 2;  // the bricks of the axis the region reaches
  Column raw;
#pragma unroll
  for (uint32_t w = 0; w < 4u; ++w) {
    uint64_t word = 0ull;
    const uint32_t first = umax(b_lo, 16u * w), last = umin(b_hi, 16u * w + 15u);
    if (l.inside) {
      for (uint32_t b = first; b <= last; ++b) {  // (uniform bounds; empty where the region does not reach this word)
        uint32_t bx, by, bz;
        place(a.axis, b, 0u, 0u, bx, by, bz);
        const uint32_t code = l.code | leaf_code(bx, by, bz);
        uint32_t nib = column_nibble(a.brick_mask[code], l.off, stride);
        if (a.byte != 0u && nib != 0u) {  // under a filter the voxels of other materials are see-through
#pragma unroll
          for (uint32_t i = 0; i < 4u; ++i)
            if (((nib >> i) & 1u) && a.grid[(size_t)code * 64u + l.off + i * stride] != a.byte) nib &= ~(1u << i);
        }
        word |= (uint64_t)nib << (4u * (b & 15u));
      }
    }
    raw.w[w] = word;
  }
  return column_run(column_turn(raw, a.lo_n, a.hi_n, a.from_high != 0u), a.layer);
}

}  // namespace

__global__ void __launch_bounds__(256) k_columns(ColumnArgs a) {
  __shared__ uint32_t bins[kColumnBins];  // the workgroup's table
  __shared__ uint32_t part[4][kColumnAccWords];
  const bool table = a.bins != nullptr;  // uniform: a kernel argument
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  if (table) {
    bins[threadIdx.x] = 0u;  // (256 threads, kColumnBins bins)
    __syncthreads();
  }
  const ColumnLane l = column_lane(a, blockIdx.x, threadIdx.x);
  const ColumnRun r = column_walk(a, l);
  const bool hit = l.inside && r.at != kColumnBits;
  uint32_t coord = 0, palette = 255u, x = 0, y = 0, z = 0, key = 0;
  if (hit) {
    coord = column_coord(r.at, a.lo_n, a.hi_n, a.from_high != 0u);
    place(a.axis, coord, l.u, l.v, x, y, z);
    key = (x << 16) | (y << 8) | z;
    palette = a.byte != 0u ? a.byte - 1u : (a.grid ? (uint32_t)a.grid[voxel_index(x, y, z)] - 1u : 0u) & 255u;
  }
  if (l.inside) {
    if (a.cells) a.cells[(size_t)(l.v - a.lo_v) * (a.hi_u - a.lo_u + 1u) + (l.u - a.lo_u)] = column_cell(coord, palette, r);
    if (table) atomicAdd(&bins[hit ? 1u + palette : 0u], 1u);
  }
  // the wave's partial record (a lane outside the region or without the layer adds nothing: its run is the empty column's)
  const uint32_t hits = (uint32_t)__popcll(__ballot(hit));
  const uint32_t voxels = wave_add(hit ? r.length : 0u), runs = wave_add(r.runs), depths = wave_add(hit ? r.at : 0u);
  const uint32_t near = wave_umax(hit ? column_near_word(r.at, key) : 0u), far = wave_umax(hit ? column_far_word(r.at, key) : 0u);
  const uint32_t lo_x = wave_umax(hit ? 255u - x : 0u), lo_y = wave_umax(hit ? 255u - y : 0u), lo_z = wave_umax(hit ? 255u - z : 0u);
  const uint32_t hi_x = wave_umax(x), hi_y = wave_umax(y), hi_z = wave_umax(z);
  if (lane == 0u) {
    uint32_t* p = part[wave];
    p[0] = hits; p[1] = voxels; p[2] = runs; p[3] = depths; p[4] = near; p[5] = far;
    p[6] = lo_x; p[7] = lo_y; p[8] = lo_z; p[9] = hi_x; p[10] = hi_y; p[11] = hi_z;
  }
  __syncthreads();
  if (wave == 0u && lane < kColumnAccWords) {  // the four partials into one, and one atomic per field that has something to say
    const uint32_t p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
    if (lane < kColumnAccSums) {
      const uint32_t sum = p0 + p1 + p2 + p3;
      if (sum != 0u) atomicAdd(&a.acc[lane], sum);
    } else {
      const uint32_t most = umax(umax(p0, p1), umax(p2, p3));
      if (most != 0u) atomicMax(&a.acc[lane], most);
    }
  }
  if (table) {  // flush: the non-zero bins only (the adds above are before the barrier)
    const uint32_t n = bins[threadIdx.x];
    if (n != 0u) atomicAdd(&a.bins[threadIdx.x], n);
  }
}

__global__ void __launch_bounds__(256) k_columns_apply(ColumnApplyArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const ColumnLane l = column_lane(a.q, blockIdx.x, threadIdx.x);
  const ColumnRun r = column_walk(a.q, l);  // everything that is read of the column to decide; a lane outside the region: a miss
  const ColumnSpan s = column_span(r, a.where, a.depth);
  uint32_t n = 0;
  for (uint32_t i = 0; i < s.count; ++i) {
    uint32_t x, y, z;
    place(a.q.axis, column_coord(s.first + i, a.q.lo_n, a.q.hi_n, a.q.from_high != 0u), l.u, l.v, x, y, z);
    const uint32_t at = voxel_index(x, y, z);
    if (a.grid[at] != a.to) {
      a.grid[at] = (uint8_t)a.to;
      ++n;
    }
  }
  n = wave_add(n);
  if (n != 0u && lane == 0u) atomicAdd(a.changed, n);
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_columns(const ColumnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_columns, dim3(a.cells_u * a.cells_v), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_columns_apply(const ColumnApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_columns_apply, dim3(a.q.cells_u * a.q.cells_v), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
