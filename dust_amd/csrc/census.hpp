// census.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_census) and the census kernels (census.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "edit.hpp"  // DevEditShape: a census reads the shape records edit_shapes reads (solid_to / empty_to are not looked at)

namespace dust {

constexpr uint32_t kCensusBins = 256;  // a row of the tables: bin 0 None, bin 1 + p palette index p -- the grid byte itself

// What the device accumulates per shape that covers something: k_census_init writes the neutral element, k_census adds to it with
// integer atomics (no order shows in the result).
struct CensusAcc {  // 56 bytes
  uint32_t covered, solid;  // voxels whose centre the shape contains; ... of them solid
  uint32_t lo[3], hi[3];    // bounds of the solid covered voxels (255 / 0 while there is none)
  uint64_t sum[3];          // sums of x, of y, of z over them
};
static_assert(sizeof(CensusAcc) == 56, "census accumulator");

struct CensusArgs {
  const uint8_t* grid;          // EditArgs::grid, only read
  const DevEditShape* shapes;   // the chunk's shapes
  const uint32_t* cells;        // n_cells root cells some shape's bounds reach
  const uint32_t* cell_start;   // n_cells + 1: each cell's slice of `ids`
  const uint16_t* ids;          // indices into `shapes` (and `acc`, and the rows of `tables`)
  CensusAcc* acc;               // per shape of the chunk
  uint32_t* tables;             // per shape of the chunk kCensusBins counters, zeroed by the caller; null: no tables were asked for
  uint32_t n_cells;
};

hipError_t launch_census_init(CensusAcc* acc, uint32_t n, hipStream_t s);
hipError_t launch_census(const CensusArgs& a, hipStream_t s);

}  // namespace dust
