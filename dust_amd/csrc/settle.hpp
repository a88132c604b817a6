// settle.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_settle, _settle_apply) and the settling kernels
// (settle.hip). The rule itself is settle_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "column.hpp"  // column_u_axis, column_v_axis
#include "grid.hpp"
#include "settle_rule.hpp"

namespace dust {

// What the device accumulates for one step (a counted fall, a fall, a slide), zeroed by the caller and added to with integer atomics
// (adds and maxima: no order shows): [0] loose voxels of the region, [1] fixed ones, [2] loose voxels a fall moves, [3] voxels that turn
// solid or empty, [4] the sum of the falls, [5] columns with a moved voxel, [6] voxels a slide moves; then the maxima: [7] the longest
// fall, [8 + r] 255 - the lower bound of the voxels that turn solid or empty on axis r, [11 + r] their upper bound
constexpr uint32_t kSettleAccWords = 14;
constexpr uint32_t kSettleAccSums = 7;  // the first words are sums, the rest maxima
constexpr uint32_t kSettleSlid = 6, kSettleFallMax = 7, kSettleLo = 8, kSettleHi = 11;
// An apply's array: slot 0 the initial fall, slots 1 + 2 k and 2 + 2 k the slide and the fall of generation k
constexpr uint32_t kSettleMaxGenerations = 256;
constexpr uint32_t kSettleApplyWords = (1 + 2 * kSettleMaxGenerations) * kSettleAccWords;
// the library looks at the slots every so many generations and stops launching once four consecutive ones moved nothing
constexpr uint32_t kSettleCheckEvery = 8;

struct SettleArgs {
  const uint64_t* brick_mask;  // the solid voxels per brick (EditArgs::brick_mask's layout)
  const uint64_t* loose_mask;  // the loose ones among them; the same array when every index is loose
  uint8_t* grid;               // k_settle_fall: the grid whose bytes move, in place; k_settle: unused
  uint32_t axis;               // 0, 1, 2: the axis things fall along
  uint32_t from_high;          // 1: they fall toward hi[axis] (the +x, +y, +z sides)
  uint32_t lo_n, hi_n;         // the inclusive region, lo <= hi <= 255: along the axis,
  uint32_t lo_u, hi_u;         // along u
  uint32_t lo_v, hi_v;         // and along v
  uint32_t cell_u, cell_v;     // the first root cell (16 voxels) of the region along u and along v
  uint32_t cells_u, cells_v;   // ... and how many it reaches: a workgroup per root-cell column
  uint32_t* acc;               // kSettleAccWords
};
struct SettleSlideArgs {
  const uint64_t* brick_mask;  // the masks the slide reads
  const uint64_t* loose_mask;
  const uint8_t* grid;         // the grid it reads
  uint8_t* grid_out;           // the grid it writes: never the one it reads. Every brick the region reaches is written whole
  uint64_t* mask_out;          // ... and its two masks
  uint64_t* loose_out;
  uint32_t d_axis, d_up;       // the lateral direction: its axis, and 1 when it points to the high end
  uint32_t g_axis, g_up;       // the fall direction
  uint32_t lo[3], hi[3];       // the inclusive region, lo <= hi
  CellBox box;                 // the root cells it reaches: one workgroup each
  uint32_t* acc;               // kSettleAccWords: [kSettleSlid] and the bounds
};
struct SettleMaskArgs {
  const uint8_t* grid;
  uint64_t* brick_mask;        // out: the solid voxels of every brick of the box; null: not written
  uint64_t* loose_mask;        // out: the loose ones
  uint32_t loose[8];           // bit p: palette index p (grid byte p + 1) is loose
  CellBox box;
};

hipError_t launch_settle(const SettleArgs& a, hipStream_t s);
hipError_t launch_settle_fall(const SettleArgs& a, hipStream_t s);
hipError_t launch_settle_slide(const SettleSlideArgs& a, hipStream_t s);
hipError_t launch_settle_masks(const SettleMaskArgs& a, hipStream_t s);

}  // namespace dust
