// delta.hip -- model deltas (dust_hip_model_delta, _delta_apply): the voxels two models differ in, counted, listed and applied on the
// device. The two-model twin of surface.hip: a workgroup per root cell the region reaches, four waves of 16 bricks, lane = voxel bit.
// A brick's word in both models' brick masks (EditArgs::brick_mask, 2 MiB each) goes through delta_rule.hpp and comes back as the added
// voxels, the removed ones and the repaint candidates (solid in both). All of these are wave-uniform, so the rule, the region mask, the
// counts (popcounts of the words) and the bounds are scalar work. A brick whose two words are both 0 costs two loads. The grid bytes are
// read only where they can matter: for a brick with repaint candidates when REPAINTED is asked for -- one ballot of a != b turns the
// candidates into the repainted word, uniform again --, under a palette filter, for the tables, for a record.
//   k_delta_count  the wave adds up added, removed and repainted voxels, both models' solid voxels and the bounds over its 16 bricks in
//                  uniform registers; the four waves fold their 11-word partial records through LDS at one barrier, and at most 11
//                  ordinary vector atomics (adds and maxima) leave per cell, non-zero ones only. The tables are 2 KiB of LDS per
//                  workgroup, one LDS add per (distinct byte of a brick's listed voxels, row), flushed non-zero bins only. Per brick
//                  the number of listed voxels goes into a kLattice table where it is not 0.
//   k_delta_list   after launch_table_scan over that table: a lane's rank is its brick's offset plus the popcount of the listed word
//                  below it; it writes its 8-byte record when the rank is below the capacity. A brick's records are one contiguous run.
//   k_delta_apply  a thread per record (the host has left no key twice): it reads the voxel's grid byte, compares it with the expected
//                  one and writes the new one where it differs. Conflicts and changes are counted by ballot, one atomic each per wave.
// Everything is integer: no order shows in any result. No fences, spins or waits BETWEEN workgroups.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "delta.hpp"
#include "delta_rule.hpp"
#include "surface.hpp"  // surface_axis_bounds

namespace dust {

namespace {

// brick c of root cell `cell` under the query: everything but `ga` and `gb` is wave-uniform
struct BrickDelta {
  DeltaListed l;                     // what is listed of the brick, per kind
  uint32_t solid_before, solid_after;  // its solid voxels inside the region
  uint32_t ga, gb;                   // this lane's grid byte before and after (0 where the brick's bytes were not read)
  uint32_t code, bx, by, bz;
};
// `bytes`: the caller wants ga / gb for every listed voxel (a filter, the tables, a record), not only where the repaint needs them
__device__ __forceinline__ void brick_delta(const DeltaArgs& a, bool bytes, uint32_t cell, uint32_t c, uint32_t lane, BrickDelta& b) {
  b.l.added = b.l.removed = b.l.repainted = b.l.listed = 0ull;
  b.solid_before = b.solid_after = 0u;
  b.ga = b.gb = 0u;
  b.code = cell * 64u + c;
  const uint64_t mA = uniform64(a.mask_a[b.code]), mB = uniform64(a.mask_b[b.code]);
  if ((mA | mB) == 0ull) return;
  cell_brick(cell, c, b.bx, b.by, b.bz);
  const DeltaWords w = delta_words(mA, mB, surface_region_mask(b.bx, b.by, b.bz, a.lo, a.hi), a.kinds);
  b.solid_before = (uint32_t)__popcll(w.solid_before);
  b.solid_after = (uint32_t)__popcll(w.solid_after);
  uint64_t differs = 0ull, filter = ~0ull;
  // (the host passes both grids whenever REPAINTED is among the kinds, and whenever `bytes`)
  if (w.candidates != 0ull || (bytes && (w.added | w.removed) != 0ull)) {
    const size_t at = (size_t)b.code * 64u + lane;
    b.ga = a.grid_a[at];
    b.gb = a.grid_b[at];
    differs = __ballot(b.ga != b.gb);
    if (a.byte != 0u) filter = __ballot(b.ga == a.byte || b.gb == a.byte);
  }
  b.l = delta_listed(w, differs, filter);
}

// one LDS add per distinct byte `g` holds among the listed lanes
__device__ __forceinline__ void table_row(uint32_t* row, uint32_t g, uint64_t listed, uint32_t lane) {
  for (uint64_t rest = listed; rest != 0ull;) {
    const uint32_t byte = (uint32_t)__builtin_amdgcn_readlane((int)g, (int)__builtin_ctzll(rest));
    const uint64_t same = __ballot(g == byte) & listed;
    if (lane == 0u) atomicAdd(&row[byte & (kDeltaBins - 1u)], (uint32_t)__popcll(same));
    rest &= ~same;
  }
}

}  // namespace

__global__ void __launch_bounds__(256) k_delta_count(DeltaArgs a) {
  __shared__ uint32_t table[kDeltaRows * kDeltaBins];  // the workgroup's counters, [before / after][grid byte]
  __shared__ uint32_t part[4][kDeltaAccWords];
  const bool tables = a.tables != nullptr;  // uniform: a kernel argument
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  if (tables) {
    for (uint32_t i = threadIdx.x; i < kDeltaRows * kDeltaBins; i += 256u) table[i] = 0u;
    __syncthreads();
  }
  const uint32_t cell = a.box.cell(blockIdx.x);
  const bool bytes = a.byte != 0u || tables;
  uint32_t added = 0, removed = 0, repainted = 0, solid_before = 0, solid_after = 0;  // of the wave (uniform)
  uint32_t lo_x = 255u, lo_y = 255u, lo_z = 255u, hi_x = 0, hi_y = 0, hi_z = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    BrickDelta b;
    brick_delta(a, bytes, cell, wave * 16u + k, lane, b);
    solid_before += b.solid_before;
    solid_after += b.solid_after;
    if (b.l.listed == 0ull) continue;
    added += (uint32_t)__popcll(b.l.added);
    removed += (uint32_t)__popcll(b.l.removed);
    repainted += (uint32_t)__popcll(b.l.repainted);
    surface_axis_bounds(b.l.listed, kSurfaceX0, 16u, b.bx * 4u, lo_x, hi_x);
    surface_axis_bounds(b.l.listed, kSurfaceY0, 4u, b.by * 4u, lo_y, hi_y);
    surface_axis_bounds(b.l.listed, kSurfaceZ0, 1u, b.bz * 4u, lo_z, hi_z);
    if (a.brick_count && lane == 0u) a.brick_count[b.code] = (uint32_t)__popcll(b.l.listed);
    if (tables) {
      table_row(table, b.ga, b.l.listed, lane);
      table_row(table + kDeltaBins, b.gb, b.l.listed, lane);
    }
  }
  if (lane == 0u) {  // the wave's partial record
    const bool any = (added | removed | repainted) != 0u;
    uint32_t* p = part[wave];
    p[0] = added; p[1] = removed; p[2] = repainted; p[3] = solid_before; p[4] = solid_after;
    p[5] = any ? 255u - lo_x : 0u; p[6] = any ? 255u - lo_y : 0u; p[7] = any ? 255u - lo_z : 0u;
    p[8] = hi_x; p[9] = hi_y; p[10] = hi_z;
  }
  __syncthreads();
  if (wave == 0u && lane < kDeltaAccWords) {  // the four partials into one, and one atomic per field that has something to say
    const uint32_t p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
    if (lane < 5u) {
      const uint32_t sum = p0 + p1 + p2 + p3;
      if (sum != 0u) atomicAdd(&a.acc[lane], sum);
    } else {
      const uint32_t most = umax(umax(p0, p1), umax(p2, p3));
      if (most != 0u) atomicMax(&a.acc[lane], most);
    }
  }
  if (tables) {  // flush: the non-zero bins only
    for (uint32_t i = threadIdx.x; i < kDeltaRows * kDeltaBins; i += 256u) {
      const uint32_t n = table[i];
      if (n != 0u) atomicAdd(&a.tables[i], n);
    }
  }
}

__global__ void __launch_bounds__(256) k_delta_list(DeltaArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  for (uint32_t k = 0; k < 16u; ++k) {
    BrickDelta b;
    brick_delta(a, true, cell, wave * 16u + k, lane, b);
    if (b.l.listed == 0ull) continue;
    const uint32_t first = uniform(a.brick_count[b.code] + a.scan_tmp[b.code >> 10]);  // exclusive scans: local + block base
    if (first >= a.capacity) break;  // (the wave's later bricks come later in the list)
    const uint32_t rank = first + (uint32_t)__popcll(b.l.listed & ((1ull << lane) - 1ull));
    if (((b.l.listed >> lane) & 1ull) && rank < a.capacity) {  // (no lane leaves the loop body early: the next brick's ballot sees all 64)
      const uint32_t kind = ((b.l.added >> lane) & 1ull) ? kDeltaAdded : ((b.l.removed >> lane) & 1ull) ? kDeltaRemoved : kDeltaRepainted;
      const uint32_t key = voxel_key(b.bx, b.by, b.bz, lane);
      // a grid byte minus one is the palette index, and None (0) wraps to DUST_HIP_DELTA_NONE (255)
      a.voxels[rank] = (uint64_t)key | ((uint64_t)kind << 32) | ((uint64_t)((b.ga - 1u) & 255u) << 40) | ((uint64_t)((b.gb - 1u) & 255u) << 48);
    }
  }
}

__global__ void __launch_bounds__(256) k_delta_apply(DeltaApplyArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool conflict = false, differs = false;
  if (i < a.n) {
    const uint64_t r = a.records[i];
    const uint32_t key = (uint32_t)r, before = (uint32_t)(r >> 40) & 255u, after = (uint32_t)(r >> 48) & 255u;
    // a record's value plus one is the grid byte, and DUST_HIP_DELTA_NONE (255) wraps to None (0)
    const uint32_t expected = ((a.backward ? after : before) + 1u) & 255u, to = ((a.backward ? before : after) + 1u) & 255u;
    const size_t at = voxel_index(key >> 16, (key >> 8) & 255u, key & 255u);  // (the host has refused keys of 2^24 and above)
    const uint32_t g = a.grid[at];
    conflict = g != expected;
    differs = g != to;
    if (differs) a.grid[at] = (uint8_t)to;
  }
  const uint32_t n_differs = (uint32_t)__popcll(__ballot(differs)), n_conflicts = (uint32_t)__popcll(__ballot(conflict));
  if (lane == 0u) {
    if (n_differs) atomicAdd(&a.counters[0], n_differs);
    if (n_conflicts) atomicAdd(&a.counters[1], n_conflicts);
  }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_delta_count(const DeltaArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_delta_count, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_delta_list(const DeltaArgs& a, hipStream_t s) {
  if (a.capacity) hipLaunchKernelGGL(k_delta_list, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_delta_apply(const DeltaApplyArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_delta_apply, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
