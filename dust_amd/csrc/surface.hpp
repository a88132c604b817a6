// surface.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_surface, _surface_apply) and the surface kernels
// (surface.hip). The exposure rule itself is surface_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "grid.hpp"
#include "surface_rule.hpp"  // kSurfaceFaces

namespace dust {

constexpr uint32_t kSurfaceBins = 256;  // a row of the tables: bin 1 + p palette index p -- the grid byte itself; bin 0 stays 0
// What the device accumulates for a call, all of it zeroed by the caller and added to with integer atomics (adds and maxima: no order
// shows): [0] listed voxels, [1 + d] exposed faces of direction d, [7] solid voxels that pass the filter, [8 + r] 255 - the lower
// bound on axis r, [11 + r] the upper bound
constexpr uint32_t kSurfaceAccWords = 14;
// the list pass's scratch behind its kLattice per-brick counts: 256 block sums (scan.hpp), then the total
constexpr uint32_t kSurfaceScanWords = 256 + 1;

struct SurfaceArgs {
  const uint64_t* brick_mask;  // EditArgs::brick_mask, or launch_cast_masks' array for a model that is not editable: all that decides exposure
  const uint8_t* grid;         // EditArgs::grid, only read; null when no material is needed (no filter, no tables, no list)
  uint32_t faces;              // DUST_HIP_FACE_* bits that count, 1..63
  uint32_t walls;              // 1: the outside of the tree counts as solid
  uint32_t byte;               // 0: every solid voxel; else only voxels holding this grid byte (palette index + 1)
  uint32_t lo[3], hi[3];       // the inclusive region, clipped to the tree, lo <= hi
  CellBox box;                 // the root cells it reaches: one workgroup each
  uint32_t* acc;               // kSurfaceAccWords (count pass)
  uint32_t* tables;            // 6 * kSurfaceBins, zeroed by the caller; null: no tables were asked for (count pass)
  uint32_t* brick_count;       // kLattice, zeroed by the caller: listed voxels per brick, written where not 0 (count pass; null: not
                               // kept); after launch_table_scan the offsets the list pass reads, with its block sums in `scan_tmp`
  const uint32_t* scan_tmp;
  uint64_t* voxels;            // DustHipSurfaceVoxel records as one word each (key | faces << 32 | palette << 40), `capacity` of them (list pass)
  uint32_t capacity;
};
struct SurfaceApplyArgs {
  SurfaceArgs q;     // brick_mask, faces, walls, byte, lo, hi, box; the rest unused
  uint8_t* grid;     // EditArgs::grid: every listed voxel takes `to`
  uint32_t to;       // the grid byte (0 = None)
  uint32_t* changed;  // one word, zeroed by the caller
};

// the lowest and highest of a brick's four coordinates on an axis that `listed` touches (plane0: the axis's c == 0 plane); surface.hip
// and delta.hip keep their bounds with it
__device__ __forceinline__ void surface_axis_bounds(uint64_t listed, uint64_t plane0, uint32_t shift, uint32_t base, uint32_t& lo, uint32_t& hi) {
#pragma unroll
  for (uint32_t c = 0; c < 4u; ++c) {
    if (listed & (plane0 << (shift * c))) {
      lo = umin(lo, base + c);
      hi = umax(hi, base + c);
    }
  }
}

hipError_t launch_surface_count(const SurfaceArgs& a, hipStream_t s);
hipError_t launch_surface_list(const SurfaceArgs& a, hipStream_t s);
hipError_t launch_surface_apply(const SurfaceApplyArgs& a, hipStream_t s);

}  // namespace dust
