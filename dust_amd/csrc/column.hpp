// column.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_columns, _columns_apply) and the column kernels
// (column.hip). What a column's 256 bits say is column_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "column_rule.hpp"
#include "grid.hpp"

namespace dust {

constexpr uint32_t kColumnBins = 256;  // the table: bin 0 the missed columns, bin 1 + p the hit columns whose nearest voxel has palette index p
// What the device accumulates for a call, all of it zeroed by the caller and added to with integer atomics (adds and maxima: no order
// shows): [0] hit columns, [1] the listed runs' voxels, [2] runs of every column, [3] the hit voxels' depths, [4] column_near_word of
// the nearest hit voxel, [5] column_far_word of the farthest, [6 + r] 255 - the lower bound on axis r, [9 + r] the upper bound
constexpr uint32_t kColumnAccWords = 12;
constexpr uint32_t kColumnAccSums = 4;  // the first words are sums, the rest maxima

struct ColumnArgs {
  const uint64_t* brick_mask;  // EditArgs::brick_mask, or launch_cast_masks' array for a model that is not editable: all a walk reads
  const uint8_t* grid;         // EditArgs::grid, only read: the filter's bytes and the hit voxel's palette; null when neither is needed
  uint32_t axis;               // 0, 1, 2: the axis the columns run along
  uint32_t from_high;          // 1: the walk starts at hi[axis] (the +x, +y, +z sides)
  uint32_t byte;               // 0: every solid voxel counts; else only voxels holding this grid byte (palette index + 1)
  uint32_t layer;              // the run of every column that is asked for, 0..255
  uint32_t lo_n, hi_n;         // the inclusive region, clipped to the tree, lo <= hi: along the axis,
  uint32_t lo_u, hi_u;         // along u (the row of the map)
  uint32_t lo_v, hi_v;         // and along v
  uint32_t cell_u, cell_v;     // the first root cell (16 voxels) of the region along u and along v
  uint32_t cells_u, cells_v;   // ... and how many it reaches: a workgroup per root-cell column, cells_u * cells_v of them
  uint32_t* acc;               // kColumnAccWords
  uint32_t* bins;              // kColumnBins, zeroed by the caller; null: no table was asked for
  uint32_t* cells;             // DustHipColumnCell records as one word each, row-major [v - lo_v][u - lo_u]; null: counts only
};
struct ColumnApplyArgs {
  ColumnArgs q;       // brick_mask, grid (under a filter), axis, from_high, byte, layer, lo_*, hi_*, cell_*, cells_*; the rest unused
  uint8_t* grid;      // EditArgs::grid: the voxels of every hit column's span take `to`
  uint32_t where;     // kColumnsRun / kColumnsGap
  uint32_t depth;     // 1..256
  uint32_t to;        // the grid byte (0 = None)
  uint32_t* changed;  // one word, zeroed by the caller
};

// mesh's in-plane axes: u the higher-numbered of the two remaining axes, v the other one
__host__ __device__ __forceinline__ uint32_t column_u_axis(uint32_t axis) { return axis == 2u ? 1u : 2u; }
__host__ __device__ __forceinline__ uint32_t column_v_axis(uint32_t axis) { return axis == 0u ? 1u : 0u; }

hipError_t launch_columns(const ColumnArgs& a, hipStream_t s);
hipError_t launch_columns_apply(const ColumnApplyArgs& a, hipStream_t s);

}  // namespace dust
