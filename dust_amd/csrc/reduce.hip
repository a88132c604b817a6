// reduce.hip -- dust_hip_model_reduce: one level of a model reduction, a grid of half the extent voted from a grid.
//
// k_reduce_level: a wavefront per destination brick (4^3 coarse voxels), lane = coarse voxel (grid.hpp brick_voxel). A lane's eight
// children are the 2^3 source voxels at twice its coordinates; a brick's children are an 8^3 box of the source, eight bricks of 64
// contiguous bytes. The two children along z share a brick and lie side by side in it at an even offset (voxel_index ends in z & 3,
// and 2Z is even), so a lane gathers four aligned 16-bit loads, packs them and calls reduce_vote (reduce_rule.hpp). The wave stores
// its 64 bytes as one coalesced brick -- or nothing, where the brick comes out empty and the destination is known to be zero. Lanes
// and bricks outside the coarse cube load nothing and store zero: that is how the last level clears what the levels before it left in
// the new model's grid. The two counts of the call come from the ballots, one atomic add per wave: integer adds commute, so the
// counts do not depend on the order. The source is never the destination (the host ping-pongs), so no wave reads what another writes.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "grid.hpp"
#include "reduce.hpp"
#include "reduce_rule.hpp"

namespace dust {

__global__ void __launch_bounds__(256) k_reduce_level(ReduceArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t brick = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));  // x-major among the 2^cover_log2 bricks per side
  const uint32_t side = a.cover_log2;
  if ((brick >> (3u * side)) != 0u) return;  // (a launch of fewer than four bricks)
  const uint32_t bx = brick >> (2u * side), by = (brick >> side) & ((1u << side) - 1u), bz = brick & ((1u << side) - 1u);
  const Voxel v = brick_voxel(bx, by, bz, lane);
  uint32_t out = 0, read = 0;
  const bool inside = bx * 4u < a.extent && by * 4u < a.extent && bz * 4u < a.extent;  // wave-uniform: the brick meets the coarse cube
  if (inside) {
    uint64_t children = 0;
    if (v.x < a.extent && v.y < a.extent && v.z < a.extent) {  // 2 * coordinate + 1 < 2 * extent <= 256
#pragma unroll
      for (uint32_t ij = 0; ij < 4u; ++ij) {
        const uint32_t at = voxel_index(2u * v.x + (ij >> 1), 2u * v.y + (ij & 1u), 2u * v.z);
        children |= (uint64_t)(*reinterpret_cast<const uint16_t*>(a.src + at)) << (16u * ij);
      }
    }
    out = reduce_vote(children, a.min_solid);
    if (a.count_src) {
#pragma unroll
      for (uint32_t k = 0; k < 8u; ++k) read += (uint32_t)__popcll(__ballot(((children >> (8u * k)) & 255ull) != 0ull));
    }
  }
  const unsigned long long solid = __ballot(out != 0u);
  if (solid != 0ull || !a.fresh) a.dst[(size_t)leaf_code(bx, by, bz) * 64u + lane] = (uint8_t)out;
  if (lane == 0u) {
    if (a.count_src && read != 0u) atomicAdd(a.count_src, read);
    if (a.count_dst && solid != 0ull) atomicAdd(a.count_dst, (uint32_t)__popcll(solid));
  }
}

hipError_t launch_reduce_level(const ReduceArgs& a, hipStream_t s) {
  const uint32_t bricks = 1u << (3u * a.cover_log2);
  hipLaunchKernelGGL(k_reduce_level, dim3((bricks + 3u) / 4u), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
