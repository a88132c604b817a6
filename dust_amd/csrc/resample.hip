// resample.hip -- dust_hip_model_resample: the voxels of one model pasted into another's edit grid under any rotation, scale or shear.
//
// k_resample is k_stamp (stamp.hip) with another geometry, on the same skeleton (cell_records.hpp): one workgroup per root cell that
// some record's image may reach, a lane's 16 voxels in registers, the cell's record list walked ONCE in call order, the palette map in
// 256 bytes of LDS. Where a stamp's source coordinate is base +- d on a permuted axis, a resample's is the floor of a fixed-point
// affine form of all three destination coordinates (resample_rule.hpp: the text the host's binning runs too). The form is separable,
// so a lane computes its x terms once per record and its y and z terms four times each, per source axis; a voxel then costs three
// adds, three shifts and the compares against the sub-box, the address scatter of voxel_index (grid.hpp) on the three computed
// coordinates -- they differ from lane to lane, so unlike a stamp's they cannot be scattered per axis in advance -- and one predicated
// byte load. A voxel whose source coordinate falls outside the sub-box is not part of the image: it loads nothing and keeps its byte
// under every operation.
//
// The cull is the host's: a record is listed in a root cell only when the exact range of its map over the cell, clipped to the record's
// box, meets the sub-box on all three source axes (resample_cell_meets, model_records.hpp), so a thin piece turned out of the axes costs
// the cells near its image, not its bounding box. Inside a listed cell a brick is rejected by the record's box alone. (The same
// interval test per brick, on the scalar unit, was built and measured: it cost 45 to 65 spilled SGPRs and changed no time --
// docs/EXPERIMENTS.md -- and was taken out again.)
//
// The counts: changed goes out as the skeleton does it; covered, solid and blocked are popcounts of ballots summed per wave and record
// and sent as one ordinary vector atomic add each by lane 0, only where the sum is not zero. Integer adds: two runs give the same
// counts. k_resample_count is the dry run: the read-only walk, no set and no write-back, every record counted against the grid as it
// stands. The source is never the grid being written (the host hands a copy when a model is resampled onto itself).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cell_records.hpp"
#include "resample.hpp"
#include "stamp.hpp"

namespace dust {

namespace {
// record `id` of the chunk held against (kDry) or applied to the wave's bricks: -> the voxels it changes (would change) in this wave
template <bool kDry, class Bricks>
__device__ __forceinline__ uint32_t resample_record(const ResampleArgs& a, const uint8_t* map, Bricks& c, uint32_t id) {
  const DevResample s = a.records[id];
  const ResampleMap& r = s.map;
  const int32_t lo_x = (int32_t)(s.lo & 255u), lo_y = (int32_t)((s.lo >> 8) & 255u), lo_z = (int32_t)(s.lo >> 16);
  const int32_t hi_x = (int32_t)(s.hi & 255u), hi_y = (int32_t)((s.hi >> 8) & 255u), hi_z = (int32_t)(s.hi >> 16);
  const int32_t sl[3] = {(int32_t)(s.src_lo & 255u), (int32_t)((s.src_lo >> 8) & 255u), (int32_t)(s.src_lo >> 16)};
  const int32_t sh[3] = {(int32_t)(s.src_hi & 255u), (int32_t)((s.src_hi >> 8) & 255u), (int32_t)(s.src_hi >> 16)};
  // ---- wave-uniform: which of the wave's 16 bricks the record's box reaches
  if (c.bx < (uint32_t)(lo_x >> 2) || c.bx > (uint32_t)(hi_x >> 2)) return 0u;
  uint32_t reach = 0;
#pragma unroll
  for (int k16 = 0; k16 < 16; ++k16) {
    const int32_t by = (int32_t)c.by0 + (k16 >> 2), bz = (int32_t)c.bz0 + (k16 & 3);
    reach |= (by >= (lo_y >> 2) && by <= (hi_y >> 2) && bz >= (lo_z >> 2) && bz <= (hi_z >> 2) ? 1u : 0u) << k16;
  }
  if (reach == 0u) return 0u;
  // ---- per lane: the x terms once, the y and z terms four times each, per source axis
  const Voxel p = brick_voxel(c.bx, c.by0, c.bz0, c.lane);  // this lane's voxel of the wave's first brick
  const int32_t x = (int32_t)p.x, y0 = (int32_t)p.y, z0 = (int32_t)p.z;
  const bool in_x = x >= lo_x && x <= hi_x;
  int32_t qx[3], qy[3][4], qz[3][4];
  uint32_t in_y = 0, in_z = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) qx[k] = resample_term(r.m[k][0], x) + r.t2[k];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int32_t y = y0 + 4 * q, z = z0 + 4 * q;
    in_y |= (y >= lo_y && y <= hi_y ? 1u : 0u) << q;
    in_z |= (z >= lo_z && z <= hi_z ? 1u : 0u) << q;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      qy[k][q] = resample_term(r.m[k][1], y);
      qz[k][q] = resample_term(r.m[k][2], z);
    }
  }
  uint32_t n = 0, covered = 0, solid = 0, blocked = 0;  // of the wave (uniform)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int32_t qxy[3] = {qx[0] + qy[0][q], qx[1] + qy[1][q], qx[2] + qy[2][q]};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int k16 = q * 4 + w;
      if (!((reach >> k16) & 1u)) continue;
      const int32_t s0 = resample_floor(qxy[0] + qz[0][w]), s1 = resample_floor(qxy[1] + qz[1][w]), s2 = resample_floor(qxy[2] + qz[2][w]);
      const bool in = in_x && ((in_y >> q) & 1u) && ((in_z >> w) & 1u) && resample_inside(s0, sl[0], sh[0]) && resample_inside(s1, sl[1], sh[1]) &&
                      resample_inside(s2, sl[2], sh[2]);
      const uint64_t image = __ballot(in);
      if (image == 0ull) continue;
      uint32_t from = 0;
      if (in) from = map[a.src[voxel_index((uint32_t)s0, (uint32_t)s1, (uint32_t)s2)]];  // in the image: 0 <= src_lo <= s <= src_hi <= 255 per axis
      const uint32_t g = c.v[k16];
      const uint32_t act = (s.table >> (((from ? 2u : 0u) | (g ? 1u : 0u)) * 2u)) & 3u;
      const uint32_t to = act == kStampKeep ? g : act == kStampTake ? from : 0u;
      const bool differs = in && to != g;
      covered += (uint32_t)__popcll(image);
      solid += (uint32_t)__popcll(__ballot(in && from != 0u));
      blocked += (uint32_t)__popcll(__ballot(in && from != 0u && g != 0u));
      if constexpr (kDry) n += (uint32_t)__popcll(__ballot(differs));
      else n += c.set(k16, differs, to);
    }
  }
  if (c.lane == 0u) {
    uint32_t* extra = a.extra + (size_t)id * kResampleExtra;
    if (covered) atomicAdd(&extra[0], covered);
    if (solid) atomicAdd(&extra[1], solid);
    if (blocked) atomicAdd(&extra[2], blocked);
    if (kDry && n) atomicAdd(&a.changed[id], n);
  }
  return n;
}
}  // namespace

__global__ void __launch_bounds__(256) k_resample(ResampleArgs a) {
  __shared__ uint8_t map[256];
  map[threadIdx.x] = a.palette_map[threadIdx.x];
  __syncthreads();
  walk_cell_records(a, [&](CellBricks& c, uint32_t id) -> uint32_t { return resample_record<false>(a, map, c, id); });
}

__global__ void __launch_bounds__(256) k_resample_count(ResampleArgs a) {
  __shared__ uint8_t map[256];
  map[threadIdx.x] = a.palette_map[threadIdx.x];
  __syncthreads();
  read_cell_records(a, [&](const CellBricks& c, uint32_t id) { resample_record<true>(a, map, c, id); });
}

hipError_t launch_resample(const ResampleArgs& a, bool dry, hipStream_t s) {
  if (a.n_cells) {
    if (dry) hipLaunchKernelGGL(k_resample_count, dim3(a.n_cells), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_resample, dim3(a.n_cells), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace dust
