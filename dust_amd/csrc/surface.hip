// surface.hip -- model surfaces (dust_hip_model_surface, _surface_apply): where the solid meets the air and facing which way, counted,
// listed and repainted on the device. Exposure is decided from the brick masks alone (EditArgs::brick_mask, 2 MiB): a brick's word and
// its six neighbours' go through surface_rule.hpp and come back as six 64-bit exposure words. All seven words are wave-uniform, so in
// these wavefront-per-brick kernels the rule, the region mask, the counts (popcounts of the words) and the bounds are scalar work; the
// grid is read only for the material -- under a palette filter, for the tables, for a listed voxel's record, for an apply's `changed`.
//
// All three kernels share census's shape (cell_records.hpp): a workgroup per root cell the region reaches, four waves of 16 bricks,
// lane = voxel bit. A brick whose word is 0 costs one load.
//   k_surface_count  the wave adds up listed voxels, faces per direction, solid voxels and bounds over its 16 bricks in uniform
//                    registers; the four waves fold their 14-word partial records through LDS at one barrier, and at most 14
//                    ordinary vector atomics (adds and maxima) leave per cell. The tables are a 6 KiB LDS table per workgroup, one LDS
//                    add per (distinct material of a brick, direction), flushed non-zero bins only. Per brick the number of listed
//                    voxels goes into a kLattice table where it is not 0.
//   k_surface_list   after launch_table_scan over that table: a lane's rank is its brick's offset plus the popcount of the listed word
//                    below it; it writes its 8-byte record when the rank is below the capacity. A brick's records are one contiguous run.
//   k_surface_apply  every listed voxel takes a grid byte. Exposure reads only the brick masks, which nothing writes before the rebuild,
//                    and the filter reads the lane's own grid byte, which only that lane writes: what is listed is decided on the
//                    model as it stood when the call began.
// (The atomic rates measured for this chip are for float adds of full rows; integer adds of a few words per cell are unmeasured, so
// their number is kept small rather than budgeted.) Everything is integer: no order shows in any result. No fences, spins or waits
// BETWEEN workgroups.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "surface.hpp"
#include "surface_rule.hpp"

namespace dust {

namespace {

// the word of brick (bx, by, bz), or `outside` off the tree (coordinates -1 and 64 wrap to above 63)
__device__ __forceinline__ uint64_t brick_word(const uint64_t* mask, uint32_t bx, uint32_t by, uint32_t bz, uint64_t outside) {
  if (bx > 63u || by > 63u || bz > 63u) return outside;
  return uniform64(mask[leaf_code(bx, by, bz)]);
}

// brick c of root cell `cell` under the query: everything but `g` is wave-uniform
struct BrickFaces {
  uint64_t sel;     // the solid voxels inside the region that pass the palette filter
  uint64_t e[6];    // ... of them, per direction that counts, those whose face is exposed
  uint64_t listed;  // the union of e
  uint32_t g;       // this lane's grid byte (0 when `grid` is null)
  uint32_t code, bx, by, bz;
};
__device__ __forceinline__ void brick_faces(const SurfaceArgs& a, const uint8_t* grid, uint32_t cell, uint32_t c, uint32_t lane, BrickFaces& b) {
  b.sel = b.listed = 0ull;
  b.g = 0u;
  b.code = cell * 64u + c;
  const uint64_t own = uniform64(a.brick_mask[b.code]);
  if (own == 0ull) return;
  cell_brick(cell, c, b.bx, b.by, b.bz);
  uint64_t sel = own & surface_region_mask(b.bx, b.by, b.bz, a.lo, a.hi);
  if (sel == 0ull) return;
  if (grid) {
    b.g = grid[(size_t)b.code * 64u + lane];
    if (a.byte != 0u) sel &= __ballot(b.g == a.byte);  // (the host passes a grid whenever there is a filter)
    if (sel == 0ull) return;
  }
  b.sel = sel;
  const uint64_t outside = a.walls ? ~0ull : 0ull;
  const SurfaceWords w = surface_exposure(own, brick_word(a.brick_mask, b.bx - 1u, b.by, b.bz, outside), brick_word(a.brick_mask, b.bx + 1u, b.by, b.bz, outside),
                                          brick_word(a.brick_mask, b.bx, b.by - 1u, b.bz, outside), brick_word(a.brick_mask, b.bx, b.by + 1u, b.bz, outside),
                                          brick_word(a.brick_mask, b.bx, b.by, b.bz - 1u, outside), brick_word(a.brick_mask, b.bx, b.by, b.bz + 1u, outside));
#pragma unroll
  for (uint32_t d = 0; d < kSurfaceFaces; ++d) {
    b.e[d] = ((a.faces >> d) & 1u) ? (w.e[d] & sel) : 0ull;
    b.listed |= b.e[d];
  }
}

}  // namespace

__global__ void __launch_bounds__(256) k_surface_count(SurfaceArgs a) {
  __shared__ uint32_t table[kSurfaceFaces * kSurfaceBins];  // the workgroup's counters, [direction][grid byte]
  __shared__ uint32_t part[4][kSurfaceAccWords];
  const bool tables = a.tables != nullptr;  // uniform: a kernel argument
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  if (tables) {
    for (uint32_t i = threadIdx.x; i < kSurfaceFaces * kSurfaceBins; i += 256u) table[i] = 0u;
    __syncthreads();
  }
  const uint32_t cell = a.box.cell(blockIdx.x);
  const uint8_t* grid = (a.byte != 0u || tables) ? a.grid : nullptr;
  uint32_t voxels = 0, solid = 0, n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0, n5 = 0;  // of the wave (uniform)
  uint32_t lo_x = 255u, lo_y = 255u, lo_z = 255u, hi_x = 0, hi_y = 0, hi_z = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    BrickFaces b;
    brick_faces(a, grid, cell, wave * 16u + k, lane, b);
    if (b.sel == 0ull) continue;
    solid += (uint32_t)__popcll(b.sel);
    if (b.listed == 0ull) continue;
    const uint32_t n = (uint32_t)__popcll(b.listed);
    voxels += n;
    n0 += (uint32_t)__popcll(b.e[0]); n1 += (uint32_t)__popcll(b.e[1]); n2 += (uint32_t)__popcll(b.e[2]);
    n3 += (uint32_t)__popcll(b.e[3]); n4 += (uint32_t)__popcll(b.e[4]); n5 += (uint32_t)__popcll(b.e[5]);
    surface_axis_bounds(b.listed, kSurfaceX0, 16u, b.bx * 4u, lo_x, hi_x);
    surface_axis_bounds(b.listed, kSurfaceY0, 4u, b.by * 4u, lo_y, hi_y);
    surface_axis_bounds(b.listed, kSurfaceZ0, 1u, b.bz * 4u, lo_z, hi_z);
    if (a.brick_count && lane == 0u) a.brick_count[b.code] = n;
    if (tables) {  // one LDS add per distinct byte among the listed lanes and direction it is exposed in
      for (uint64_t rest = b.listed; rest != 0ull;) {
        const uint32_t byte = (uint32_t)__builtin_amdgcn_readlane((int)b.g, (int)__builtin_ctzll(rest));
        const uint64_t same = __ballot(b.g == byte) & b.listed;
#pragma unroll
        for (uint32_t d = 0; d < kSurfaceFaces; ++d) {
          const uint32_t nd = (uint32_t)__popcll(same & b.e[d]);
          if (nd != 0u && lane == 0u) atomicAdd(&table[d * kSurfaceBins + (byte & (kSurfaceBins - 1u))], nd);
        }
        rest &= ~same;
      }
    }
  }
  if (lane == 0u) {  // the wave's partial record
    uint32_t* p = part[wave];
    p[0] = voxels; p[1] = n0; p[2] = n1; p[3] = n2; p[4] = n3; p[5] = n4; p[6] = n5; p[7] = solid;
    p[8] = voxels ? 255u - lo_x : 0u; p[9] = voxels ? 255u - lo_y : 0u; p[10] = voxels ? 255u - lo_z : 0u;
    p[11] = hi_x; p[12] = hi_y; p[13] = hi_z;
  }
  __syncthreads();
  if (wave == 0u && lane < kSurfaceAccWords) {  // the four partials into one, and one atomic per field that has something to say
    const uint32_t p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
    if (lane < 8u) {
      const uint32_t sum = p0 + p1 + p2 + p3;
      if (sum != 0u) atomicAdd(&a.acc[lane], sum);
    } else {
      const uint32_t most = umax(umax(p0, p1), umax(p2, p3));
      if (most != 0u) atomicMax(&a.acc[lane], most);
    }
  }
  if (tables) {  // flush: the non-zero bins only
    for (uint32_t i = threadIdx.x; i < kSurfaceFaces * kSurfaceBins; i += 256u) {
      const uint32_t n = table[i];
      if (n != 0u) atomicAdd(&a.tables[i], n);
    }
  }
}

__global__ void __launch_bounds__(256) k_surface_list(SurfaceArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  for (uint32_t k = 0; k < 16u; ++k) {
    BrickFaces b;
    brick_faces(a, a.grid, cell, wave * 16u + k, lane, b);
    if (b.sel == 0ull || b.listed == 0ull) continue;
    const uint32_t first = uniform(a.brick_count[b.code] + a.scan_tmp[b.code >> 10]);  // exclusive scans: local + block base
    if (first >= a.capacity) break;  // (the wave's later bricks come later in the list)
    const uint32_t rank = first + (uint32_t)__popcll(b.listed & ((1ull << lane) - 1ull));
    if (((b.listed >> lane) & 1ull) && rank < a.capacity) {  // (no lane leaves the loop body early: the next brick's ballot sees all 64)
      uint32_t faces = 0;
#pragma unroll
      for (uint32_t d = 0; d < kSurfaceFaces; ++d) faces |= (uint32_t)((b.e[d] >> lane) & 1ull) << d;
      const uint32_t key = voxel_key(b.bx, b.by, b.bz, lane);
      a.voxels[rank] = (uint64_t)key | ((uint64_t)faces << 32) | ((uint64_t)((b.g - 1u) & 255u) << 40);
    }
  }
}

__global__ void __launch_bounds__(256) k_surface_apply(SurfaceApplyArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.q.box.cell(blockIdx.x);
  uint32_t n = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    BrickFaces b;
    brick_faces(a.q, a.grid, cell, wave * 16u + k, lane, b);
    if (b.sel == 0ull || b.listed == 0ull) continue;
    const bool differs = ((b.listed >> lane) & 1ull) && b.g != a.to;
    if (differs) a.grid[(size_t)b.code * 64u + lane] = (uint8_t)a.to;
    n += (uint32_t)__popcll(__ballot(differs));
  }
  if (n && lane == 0u) atomicAdd(a.changed, n);
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_surface_count(const SurfaceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_surface_count, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_surface_list(const SurfaceArgs& a, hipStream_t s) {
  if (a.capacity) hipLaunchKernelGGL(k_surface_list, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_surface_apply(const SurfaceApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_surface_apply, dim3(a.q.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
