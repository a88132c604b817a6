// body.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_bodies) and the body kernels (body.hip). The arithmetic
// itself is body_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "body_rule.hpp"
#include "grid.hpp"

namespace dust {

// the kinds of groups, the values of DUST_HIP_BODIES_*
constexpr uint32_t kBodiesAll = 0, kBodiesMaterials = 1, kBodiesIslands = 2, kBodiesCells = 3;
constexpr uint32_t kBodyMaterials = 255;  // records of a MATERIALS call, and the entries of a weight table

// One group while its record is being accumulated: zeroed by the caller and added to with integer atomics (adds and maxima: no order
// shows). body_rule.hpp's BodyPart with the group's key in front.
struct BodyAcc {  // 128 bytes
  uint32_t key, voxels;
  uint32_t bounds[6];  // 255 - lo[3], then hi[3]
  unsigned long long sums[kBodySums];
  uint32_t pad[4];
};
static_assert(sizeof(BodyAcc) == 128 && offsetof(BodyAcc, sums) == 32, "body accumulator");

struct BodyArgs {
  const uint64_t* brick_mask;  // EditArgs::brick_mask, or launch_cast_masks' array for a model that is not editable
  const uint8_t* grid;         // EditArgs::grid, only read; null when nothing needs a material (no weights, no filter, not MATERIALS)
  const uint32_t* label;       // ISLANDS: the flat island labelling, by public key
  const uint16_t* field;       // CELLS: the cell field, brick-major
  const uint16_t* weights;     // kBodyMaterials weights by palette index; null: every voxel weighs 1
  const uint64_t* root_mask;   // ISLANDS: IslandArgs::root_mask, root_count (scanned) and scan_tmp -- an island's rank in key order
  const uint32_t* root_count;
  const uint32_t* scan_tmp;
  uint32_t group;              // kBodies*
  uint32_t byte;               // 0: every solid voxel; else only voxels holding this grid byte (palette index + 1)
  uint32_t lo[3], hi[3];       // the inclusive region, lo <= hi
  CellBox box;                 // the root cells it reaches: one workgroup each
  BodyAcc* acc;                // `capacity` accumulators, zeroed by the caller
  BodyRecord* records;         // `capacity` records
  uint32_t capacity;           // records wanted: min(groups, the caller's capacity); a group past it is not accumulated
};

// ISLANDS: the keys of the first a.capacity islands into their accumulators (an island without a counted voxel keeps its key)
hipError_t launch_body_keys(const BodyArgs& a, hipStream_t s);
// the region's counted voxels into the accumulators
hipError_t launch_bodies(const BodyArgs& a, hipStream_t s);
// accumulators -> records
hipError_t launch_bodies_emit(const BodyArgs& a, hipStream_t s);

}  // namespace dust
