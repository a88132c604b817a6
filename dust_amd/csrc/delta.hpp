// delta.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_delta, _delta_apply) and the delta kernels (delta.hip).
// What the two brick words of a brick say is delta_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "delta_rule.hpp"
#include "grid.hpp"

namespace dust {

constexpr uint32_t kDeltaBins = 256;  // a row of the tables: the grid byte itself -- bin 0 None, bin 1 + p palette index p
constexpr uint32_t kDeltaRows = 2;    // row 0: the listed voxels' values before; row 1: their values after
// What the device accumulates for a call, all of it zeroed by the caller and added to with integer atomics (adds and maxima: no order
// shows): [0] added, [1] removed, [2] repainted, [3] solid before, [4] solid after, [5 + r] 255 - the lower bound on axis r,
// [8 + r] the upper bound
constexpr uint32_t kDeltaAccWords = 11;
constexpr uint32_t kDeltaMaxRecords = 1u << 24;  // a delta_apply call's records: a tree's voxels

struct DeltaArgs {
  const uint64_t* mask_a;  // the brick masks before and after: EditArgs::brick_mask, or launch_cast_masks' array for a model that is
  const uint64_t* mask_b;  // not editable
  const uint8_t* grid_a;   // EditArgs::grid of both, only read; null when no byte is needed: REPAINTED not among the kinds, no filter,
  const uint8_t* grid_b;   // no tables, no list
  uint32_t kinds;          // DUST_HIP_DELTA_* bits that count, 1..7
  uint32_t byte;           // 0: every change; else only voxels whose grid byte before or after is this one (palette index + 1)
  uint32_t lo[3], hi[3];   // the inclusive region, clipped to the tree, lo <= hi
  CellBox box;             // the root cells it reaches: one workgroup each
  uint32_t* acc;           // kDeltaAccWords (count pass)
  uint32_t* tables;        // kDeltaRows * kDeltaBins, zeroed by the caller; null: no tables were asked for (count pass)
  uint32_t* brick_count;   // kLattice, zeroed by the caller: listed voxels per brick, written where not 0 (count pass; null: not
                           // kept); after launch_table_scan the offsets the list pass reads, with its block sums in `scan_tmp`
  const uint32_t* scan_tmp;
  uint64_t* voxels;        // DustHipDeltaVoxel records as one word each (key | kind << 32 | before << 40 | after << 48), `capacity` of them (list pass)
  uint32_t capacity;
};
struct DeltaApplyArgs {
  const uint64_t* records;  // n DustHipDeltaVoxel records as one word each, no key twice
  uint32_t n;
  uint32_t backward;        // 0: a voxel takes `after` and is expected to hold `before`; 1: the other way round
  uint8_t* grid;            // EditArgs::grid
  uint32_t* counters;       // two words, zeroed by the caller: [0] voxels whose value changed, [1] records whose voxel did not hold the expected value
};

hipError_t launch_delta_count(const DeltaArgs& a, hipStream_t s);
hipError_t launch_delta_list(const DeltaArgs& a, hipStream_t s);
hipError_t launch_delta_apply(const DeltaApplyArgs& a, hipStream_t s);

}  // namespace dust
