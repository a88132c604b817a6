// cell_records.hpp -- the skeleton of the kernels that apply a chunk of records, binned by root cell, to the grid (k_edit_shapes,
// k_stamp; the host side is batched_edit in capi_model.cpp) or only hold them against it (k_census; dust_hip_model_census). One
// workgroup per listed root cell (16^3 voxels), four waves of 16 bricks each: wave w owns the cell's child bits 16 w .. 16 w + 15 (one x slice of bricks), lane = voxel bit x<<4 | y<<2 | z, so a brick's 64
// grid bytes are one coalesced load. A lane keeps its 16 voxels in registers and the cell's record list is walked ONCE, in call order, by
// a wave-uniform id. Changes are counted per wave: one ordinary vector atomic add of the ballots' popcounts (integer adds: the counts do
// not depend on the order the waves arrive in). Bricks are written back once, and only those in which some lane changed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid.hpp"

namespace dust {

// a lane's view of its wave's 16 bricks: brick k is (bx, by0 + (k >> 2), bz0 + (k & 3)), v[k] the grid byte of voxel bit `lane` in it
struct CellBricks {
  uint32_t lane, bx, by0, bz0;
  uint32_t v[16], dirty;
  // voxel `lane` of brick k takes `to` where `differs`: -> in how many lanes of the wave
  __device__ __forceinline__ uint32_t set(int k, bool differs, uint32_t to) {
    const uint64_t m = __ballot(differs);
    if (differs) v[k] = to;
    dirty |= (m != 0ull ? 1u : 0u) << k;
    return (uint32_t)__popcll(m);
  }
};

// One text for both walkers, so that they share the load. kWrite: per_record(bricks, id) applies record `id` of the chunk with
// CellBricks::set and returns the sum of what the calls returned, which is added to a.changed[id]; the dirty bricks are written back.
// Otherwise the grid is only read (Args::grid may point to const): per_record looks at the bricks and sends off whatever it gathers
// itself. Either way the grid is read once per cell and launch, however long the cell's list is.
template <bool kWrite, class Args, class PerRecord>
__device__ __forceinline__ void for_cell_records(const Args& a, PerRecord&& per_record) {
  const uint32_t wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.cells[blockIdx.x];
  const uint32_t first = a.cell_start[blockIdx.x], last = a.cell_start[blockIdx.x + 1];
  CellBricks c;
  c.lane = threadIdx.x & 63u;
  cell_brick(cell, wave * 16u, c.bx, c.by0, c.bz0);
  auto* mine = a.grid + ((size_t)cell * 64u + wave * 16u) * 64u + c.lane;
#pragma unroll
  for (int k = 0; k < 16; ++k) c.v[k] = mine[k * 64];
  c.dirty = 0;
  for (uint32_t j = first; j < last; ++j) {
    const uint32_t id = uniform(a.ids[j]);
    if constexpr (kWrite) {
      const uint32_t n = per_record(c, id);
      if (n && c.lane == 0) atomicAdd(&a.changed[id], n);
    } else {
      per_record(c, id);
    }
  }
  if constexpr (kWrite) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if ((c.dirty >> k) & 1u) mine[k * 64] = (uint8_t)c.v[k];
  }
}

// Args: grid, cells, cell_start, ids, changed (EditShapeArgs, StampArgs)
template <class Args, class PerRecord>
__device__ __forceinline__ void walk_cell_records(const Args& a, PerRecord&& per_record) {
  for_cell_records<true>(a, static_cast<PerRecord&&>(per_record));
}
// the read-only twin (k_census). Args: grid (const), cells, cell_start, ids
template <class Args, class PerRecord>
__device__ __forceinline__ void read_cell_records(const Args& a, PerRecord&& per_record) {
  for_cell_records<false>(a, static_cast<PerRecord&&>(per_record));
}

}  // namespace dust
