// neighbour.hip -- model neighbourhoods (dust_hip_model_neighbours, _neighbours_apply): how many of a voxel's 6, 18 or 26 neighbours are
// solid, as a histogram and as one generation of a birth / survive rule, counted without writing anything (k_neighbours) or run
// generation by generation between two grids (k_neighbours_step). The counts are decided from the brick masks alone
// (EditArgs::brick_mask, 2 MiB): a brick's word and its 26 neighbour bricks' go through neighbour_rule.hpp and come back as five bit
// planes. All 27 words are wave-uniform, so in these wavefront-per-brick kernels the planes, the bit-sliced sum, the birth and survive
// words, the region mask, the popcounts and the bounds are scalar work.
//
// Both kernels share census's shape (cell_records.hpp): a workgroup per root cell the region reaches, four waves of 16 bricks, lane =
// voxel bit. The workgroup first stages the words of its 4^3 bricks and of the one-brick shell round them (6^3 words, 1.7 KiB of LDS):
// a brick's 27 words are then one LDS read by 27 lanes and 54 lane reads, not 27 global loads.
//   k_neighbours       reads the masks only. A brick whose 27 words are all 0 while count 0 gives no birth adds its region voxels to bin 0
//                      and is done. The histogram is kept with a bin per LANE (lane n < 27: the empty voxels with n neighbours, lane
//                      27 + n: the solid ones): every lane tests the five planes against its own n, so a brick costs no LDS traffic at
//                      all. The four waves fold their bins and their 10-word partial records through LDS at one barrier; at most 10 + 54
//                      ordinary vector atomics (adds and maxima) leave per cell, the non-zero ones only.
//   k_neighbours_step  one generation, never in place: masks A and grid A in, the brick's 64 bytes of grid B (one coalesced store) and
//                      its word of masks B out. A lane reads its own byte of grid A where the brick holds anything; the bytes of its
//                      neighbours only when it is born under MAJORITY, into 26 registers, and the vote is fully unrolled compares over
//                      them (no array indexed by a runtime value: nothing goes to scratch memory) -- a template instance of its own, so
//                      the fixed-palette kernel does not carry the vote's registers. Bricks of the cell the region does not reach are
//                      left alone: the host made both grids equal outside the region before the first generation. The generation's
//                      born, died and bounds go into its own slot of a device array, at most 9 atomics per workgroup.
// (The atomic rates measured for this chip are for float adds of full rows; integer adds of a few words per cell are unmeasured, so
// their number is kept small rather than budgeted.) Everything is integer: no order shows in any result. No fences, spins or waits
// BETWEEN workgroups.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "neighbour.hpp"
#include "neighbour_rule.hpp"
#include "surface.hpp"  // surface_axis_bounds

namespace dust {

namespace {

constexpr uint32_t kHaloSide = 6, kHaloWords = kHaloSide * kHaloSide * kHaloSide;

// the words of root cell `cell`'s bricks and of the shell round them into LDS: halo[(i * 6 + j) * 6 + k] is brick (4 cx - 1 + i,
// 4 cy - 1 + j, 4 cz - 1 + k), `outside` off the tree (coordinates -1 and 64 wrap to above 63)
__device__ __forceinline__ void stage_halo(const uint64_t* mask, uint32_t cell, uint64_t outside, uint64_t* halo) {
  if (threadIdx.x < kHaloWords) {
    const uint32_t i = threadIdx.x / 36u, j = (threadIdx.x / 6u) % 6u, k = threadIdx.x % 6u;
    const uint32_t bx = ((cell >> 8) << 2) + i - 1u, by = (((cell >> 4) & 15u) << 2) + j - 1u, bz = ((cell & 15u) << 2) + k - 1u;
    halo[threadIdx.x] = (bx > 63u || by > 63u || bz > 63u) ? outside : mask[leaf_code(bx, by, bz)];
  }
  __syncthreads();
}

__device__ __forceinline__ uint64_t lane_word(uint64_t v, int lane) {  // lane `lane`'s value, wave-uniform (lane is a constant)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// The 27 words of brick c of the cell out of the staged halo; false: all of them are 0 (then n is not set)
__device__ __forceinline__ bool brick_words(const uint64_t* halo, uint32_t c, uint32_t lane, NeighbourBricks& n) {
  const uint32_t rx = c >> 4, ry = (c >> 2) & 3u, rz = c & 3u;
  uint64_t mine = 0ull;
  if (lane < 27u) mine = halo[((rx + lane / 9u) * kHaloSide + ry + (lane / 3u) % 3u) * kHaloSide + rz + lane % 3u];
  if (__ballot(mine != 0ull) == 0ull) return false;
#pragma unroll
  for (int i = 0; i < 27; ++i) n.w[i] = lane_word(mine, i);
  return true;
}

__device__ __forceinline__ void changed_bounds(uint64_t changed, uint32_t bx, uint32_t by, uint32_t bz, uint32_t (&lo)[3], uint32_t (&hi)[3]) {
  surface_axis_bounds(changed, kSurfaceX0, 16u, bx * 4u, lo[0], hi[0]);
  surface_axis_bounds(changed, kSurfaceY0, 4u, by * 4u, lo[1], hi[1]);
  surface_axis_bounds(changed, kSurfaceZ0, 1u, bz * 4u, lo[2], hi[2]);
}

// The grid byte most of the solid neighbours of voxel (x, y, z) hold, among equals the lowest; 0 where none votes. `reach`: the largest
// |d|1 of the neighbourhood (1, 2 or 3). The bytes are held in registers: every loop below has constant bounds and is unrolled.
__device__ __forceinline__ uint32_t majority_byte(const uint8_t* grid, uint32_t x, uint32_t y, uint32_t z, uint32_t reach) {
  uint32_t v[26];
#pragma unroll
  for (int i = 0; i < 27; ++i) {
    if (i == 13) continue;
    const int dx = i / 9 - 1, dy = (i / 3) % 3 - 1, dz = i % 3 - 1;
    const uint32_t order = (uint32_t)((dx != 0) + (dy != 0) + (dz != 0));
    const uint32_t nx = x + (uint32_t)dx, ny = y + (uint32_t)dy, nz = z + (uint32_t)dz;  // (-1 wraps to above 255: off the tree, no vote)
    uint32_t byte = 0u;
    if (order <= reach && nx < 256u && ny < 256u && nz < 256u) byte = grid[voxel_index(nx, ny, nz)];
    v[i < 13 ? i : i - 1] = byte;
  }
  uint32_t best = 0u, best_votes = 0u;
#pragma unroll
  for (int i = 0; i < 26; ++i) {
    uint32_t votes = 0u;
#pragma unroll
    for (int j = 0; j < 26; ++j) votes += v[j] == v[i] ? 1u : 0u;
    if (v[i] != 0u && (votes > best_votes || (votes == best_votes && v[i] < best))) {
      best = v[i];
      best_votes = votes;
    }
  }
  return best;
}

}  // namespace

__global__ void __launch_bounds__(256) k_neighbours(NeighbourArgs a) {
  __shared__ uint64_t halo[kHaloWords];
  __shared__ uint32_t part[4][kNeighbourAccWords];
  __shared__ uint32_t bins[4][64];
  const bool tables = a.table != nullptr;  // uniform: a kernel argument
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  stage_halo(a.brick_mask, cell, a.walls ? ~0ull : 0ull, halo);
  const uint32_t row = lane >= kNeighbourBins ? 1u : 0u, my_n = lane - row * kNeighbourBins;  // this lane's bin (lanes 54..63: none)
  uint32_t bin = 0;                                                                           // ... and what it holds
  uint32_t voxels = 0, solid = 0, born = 0, died = 0;                                         // of the wave (uniform)
  uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u};
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t c = wave * 16u + k;
    uint32_t bx, by, bz;
    cell_brick(cell, c, bx, by, bz);
    const uint64_t region = surface_region_mask(bx, by, bz, a.lo, a.hi);
    if (region == 0ull) continue;
    voxels += (uint32_t)__popcll(region);
    NeighbourBricks n;
    const bool any = brick_words(halo, c, lane, n);
    if (!any && (a.birth & 1u) == 0u) {  // empty voxels without a neighbour, and none of them is born
      if (lane == 0u) bin += (uint32_t)__popcll(region);
      continue;
    }
    if (!any) {
#pragma unroll
      for (int i = 0; i < 27; ++i) n.w[i] = 0ull;
    }
    const uint64_t own = n.w[kNeighbourOwn];
    solid += (uint32_t)__popcll(own & region);
    const NeighbourCount count = neighbour_count(n, a.neighbourhood);
    const NeighbourChange g = neighbour_change(own, count, a.birth, a.survive, region);
    born += (uint32_t)__popcll(g.born);
    died += (uint32_t)__popcll(g.died);
    changed_bounds(g.born | g.died, bx, by, bz, lo, hi);
    if (tables && lane < kNeighbourTableWords) bin += (uint32_t)__popcll(neighbour_equals(count, my_n) & region & (row ? own : ~own));
  }
  if (lane == 0u) {  // the wave's partial record
    uint32_t* p = part[wave];
    const bool some = (born | died) != 0u;
    p[0] = voxels; p[1] = solid; p[2] = born; p[3] = died;
    p[4] = some ? 255u - lo[0] : 0u; p[5] = some ? 255u - lo[1] : 0u; p[6] = some ? 255u - lo[2] : 0u;
    p[7] = hi[0]; p[8] = hi[1]; p[9] = hi[2];
  }
  bins[wave][lane] = bin;
  __syncthreads();
  if (wave == 0u) {  // the four partials into one, and one atomic per word that has something to say
    if (lane < kNeighbourAccWords) {
      const uint32_t p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
      if (lane < 4u) {
        const uint32_t sum = p0 + p1 + p2 + p3;
        if (sum != 0u) atomicAdd(&a.acc[lane], sum);
      } else {
        const uint32_t most = umax(umax(p0, p1), umax(p2, p3));
        if (most != 0u) atomicMax(&a.acc[lane], most);
      }
    }
    if (tables && lane < kNeighbourTableWords) {
      const uint32_t sum = bins[0][lane] + bins[1][lane] + bins[2][lane] + bins[3][lane];
      if (sum != 0u) atomicAdd(&a.table[lane], sum);
    }
  }
}

// (kMajority: a kernel of its own for the vote, whose 26 bytes and unrolled compares take four times the registers of everything else)
template <bool kMajority>
__global__ void __launch_bounds__(256) k_neighbours_step(NeighbourStepArgs a) {
  __shared__ uint64_t halo[kHaloWords];
  __shared__ uint32_t part[4][kNeighbourSlotWords + 1];
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.q.box.cell(blockIdx.x);
  stage_halo(a.q.brick_mask, cell, a.q.walls ? ~0ull : 0ull, halo);
  const uint32_t reach = a.q.neighbourhood == kNeighbourFaces ? 1u : a.q.neighbourhood == kNeighbourEdges ? 2u : 3u;
  uint32_t solid = 0, born = 0, died = 0;  // of the wave (uniform)
  uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u};
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t c = wave * 16u + k, code = cell * 64u + c;
    uint32_t bx, by, bz;
    cell_brick(cell, c, bx, by, bz);
    const uint64_t region = surface_region_mask(bx, by, bz, a.q.lo, a.q.hi);
    if (region == 0ull) continue;  // (outside the region: both grids hold it already)
    NeighbourBricks n;
    const bool any = brick_words(halo, c, lane, n);
    if (!any && (a.q.birth & 1u) == 0u) {  // nothing here, nothing round it, nothing born: the brick is empty in the next generation too
      a.grid_out[(size_t)code * 64u + lane] = 0;
      if (lane == 0u) a.mask_out[code] = 0ull;
      continue;
    }
    if (!any) {
#pragma unroll
      for (int i = 0; i < 27; ++i) n.w[i] = 0ull;
    }
    const uint64_t own = n.w[kNeighbourOwn];
    solid += (uint32_t)__popcll(own & region);
    const NeighbourCount count = neighbour_count(n, a.q.neighbourhood);
    const NeighbourChange g = neighbour_change(own, count, a.q.birth, a.q.survive, region);
    uint32_t byte = own != 0ull ? (uint32_t)a.grid[(size_t)code * 64u + lane] : 0u;
    if ((g.died >> lane) & 1ull) byte = 0u;
    if (g.born != 0ull) {
      if ((g.born >> lane) & 1ull) {
        byte = a.byte;
        if (kMajority) {
          const Voxel v = brick_voxel(bx, by, bz, lane);
          const uint32_t voted = majority_byte(a.grid, v.x, v.y, v.z, reach);
          if (voted != 0u) byte = voted;
        }
      }
      born += (uint32_t)__popcll(g.born);
    }
    died += (uint32_t)__popcll(g.died);
    changed_bounds(g.born | g.died, bx, by, bz, lo, hi);
    a.grid_out[(size_t)code * 64u + lane] = (uint8_t)byte;
    if (lane == 0u) a.mask_out[code] = (own | g.born) & ~g.died;
  }
  if (lane == 0u) {  // the wave's partial record
    uint32_t* p = part[wave];
    const bool some = (born | died) != 0u;
    p[0] = born; p[1] = died;
    p[2] = some ? 255u - lo[0] : 0u; p[3] = some ? 255u - lo[1] : 0u; p[4] = some ? 255u - lo[2] : 0u;
    p[5] = hi[0]; p[6] = hi[1]; p[7] = hi[2];
    p[8] = solid;
  }
  __syncthreads();
  if (wave == 0u && lane < kNeighbourSlotWords + 1u) {
    const uint32_t p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
    if (lane < 2u) {
      const uint32_t sum = p0 + p1 + p2 + p3;
      if (sum != 0u) atomicAdd(&a.slot[lane], sum);
    } else if (lane < kNeighbourSlotWords) {
      const uint32_t most = umax(umax(p0, p1), umax(p2, p3));
      if (most != 0u) atomicMax(&a.slot[lane], most);
    } else if (a.solid) {
      const uint32_t sum = p0 + p1 + p2 + p3;
      if (sum != 0u) atomicAdd(a.solid, sum);
    }
  }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_neighbours(const NeighbourArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_neighbours, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_neighbours_step(const NeighbourStepArgs& a, hipStream_t s) {
  if (a.majority) hipLaunchKernelGGL(k_neighbours_step<true>, dim3(a.q.box.count()), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_neighbours_step<false>, dim3(a.q.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
