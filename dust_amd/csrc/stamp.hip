// stamp.hip -- dust_hip_model_stamp: the voxels of one model pasted into another's edit grid, rotated and mirrored.
//
// k_stamp stands on the skeleton k_edit_shapes stands on (cell_records.hpp): one workgroup per root cell (16^3 voxels) that some
// stamp's clipped image reaches, a lane's 16 voxels in registers, the cell's stamp list walked ONCE in call order. A stamp record is
// wave-uniform and rejected per brick by its integer bounds. Where k_edit_shapes evaluates a formula, k_stamp gathers: the source is a
// grid of the same brick-major layout, and a voxel's byte address in it, voxel_index (grid.hpp), is a bit scatter of its three
// coordinates that never mixes axes -- so the address is the sum of one term per DESTINATION axis, each the scatter of base +- d onto
// the source axis the orientation names. The x term is computed once per stamp, the y and z terms four times each; a voxel costs two
// adds and one byte load. A destination brick's image is a 4^3 box of the source: at most 8 bricks of 64 contiguous bytes. The palette
// map is 256 bytes of LDS. The source is never the grid being written (the host hands a copy when a model is stamped onto itself), so
// no workgroup reads what another writes.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cell_records.hpp"
#include "stamp.hpp"

namespace dust {

namespace {
// where coordinate c on axis `axis` (0 = x, 1 = y, 2 = z) lands in voxel_index (grid.hpp): its root-cell nibble,
// its brick pair and its voxel pair, each field 4 / 2 / 2 bits further down per axis. `axis` is wave-uniform: uniform shifts.
__device__ __forceinline__ uint32_t scatter(uint32_t c, uint32_t axis) {
  return ((c >> 4) << (20u - 4u * axis)) | (((c >> 2) & 3u) << (10u - 2u * axis)) | ((c & 3u) << (4u - 2u * axis));
}
}  // namespace

__global__ void __launch_bounds__(256) k_stamp(StampArgs a) {
  __shared__ uint8_t map[256];
  map[threadIdx.x] = a.palette_map[threadIdx.x];
  __syncthreads();
  walk_cell_records(a, [&](CellBricks& c, uint32_t id) -> uint32_t {
    const DevStamp s = a.stamps[id];
    const uint32_t lo_x = s.lo & 255u, lo_y = (s.lo >> 8) & 255u, lo_z = s.lo >> 16;
    const uint32_t hi_x = s.hi & 255u, hi_y = (s.hi >> 8) & 255u, hi_z = s.hi >> 16;
    if (c.bx < (lo_x >> 2) || c.bx > (hi_x >> 2)) return 0u;
    const Voxel p = brick_voxel(c.bx, c.by0, c.bz0, c.lane);  // this lane's voxel of the wave's first brick
    const uint32_t x = p.x, y0 = p.y, z0 = p.z;
    const uint32_t p0 = s.orient & 3u, p1 = (s.orient >> 2) & 3u, p2 = (s.orient >> 4) & 3u;
    const bool g0 = (s.orient >> 6) & 1u, g1 = (s.orient >> 7) & 1u, g2 = (s.orient >> 8) & 1u;
    const bool in_x = x >= lo_x && x <= hi_x;
    // (outside the image the terms are meaningless and never used: the load below is predicated on the bounds)
    const uint32_t ax = scatter((uint32_t)(s.base[0] + (g0 ? -(int32_t)x : (int32_t)x)), p0);
    uint32_t ay[4], az[4], in_y = 0, in_z = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t y = y0 + 4u * (uint32_t)q, z = z0 + 4u * (uint32_t)q;
      in_y |= (y >= lo_y && y <= hi_y ? 1u : 0u) << q;
      in_z |= (z >= lo_z && z <= hi_z ? 1u : 0u) << q;
      ay[q] = scatter((uint32_t)(s.base[1] + (g1 ? -(int32_t)y : (int32_t)y)), p1);
      az[q] = scatter((uint32_t)(s.base[2] + (g2 ? -(int32_t)z : (int32_t)z)), p2);
    }
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t by = c.by0 + (uint32_t)(k >> 2), bz = c.bz0 + (uint32_t)(k & 3);
      if (by < (lo_y >> 2) || by > (hi_y >> 2) || bz < (lo_z >> 2) || bz > (hi_z >> 2)) continue;
      const bool in = in_x && ((in_y >> (k >> 2)) & 1u) && ((in_z >> (k & 3)) & 1u);
      uint32_t from = 0;
      if (in) from = map[a.src[ax + ay[k >> 2] + az[k & 3]]];  // in the image: a source coordinate inside [src_lo, src_hi], < 256 per axis
      const uint32_t g = c.v[k];
      const uint32_t act = (s.table >> (((from ? 2u : 0u) | (g ? 1u : 0u)) * 2u)) & 3u;
      const uint32_t to = act == kStampKeep ? g : act == kStampTake ? from : 0u;
      n += c.set(k, in && to != g, to);
    }
    return n;
  });
}

hipError_t launch_stamp(const StampArgs& a, hipStream_t s) {
  if (a.n_cells) hipLaunchKernelGGL(k_stamp, dim3(a.n_cells), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
