// resample.hpp -- interface between the host runtime (capi_model.cpp) and the model resample kernels (resample.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resample_rule.hpp"

namespace dust {

// One record of dust_hip_model_resample as the device reads it: the caller's inverse map with the translation doubled (the rule's
// form), the destination box clipped to the tree, the source sub-box and the operation resolved into the stamp's table (stamp.hpp:
// two bits per case (source solid) << 1 | (destination solid) -- keep, take, clear). Records that cover nothing are never listed in
// a cell.
struct DevResample {  // 72 bytes
  ResampleMap map;
  uint32_t lo, hi;          // inclusive destination bounds, x | y << 8 | z << 16
  uint32_t src_lo, src_hi;  // inclusive source sub-box, packed alike
  uint32_t table;
  uint32_t pad;
};
constexpr uint32_t kResampleExtra = 3;  // the counts beside `changed`, per record: covered, solid, blocked
struct ResampleArgs {
  uint8_t* grid;               // the destination's EditArgs::grid (only read by the dry run)
  const uint8_t* src;          // the source as a grid of the same layout; never the grid being written
  const DevResample* records;  // the chunk's records, in call order
  const uint32_t* cells;       // n_cells root cells (16^3 voxels, (x>>4)<<8 | (y>>4)<<4 | (z>>4)) some record's image may reach
  const uint32_t* cell_start;  // n_cells + 1: each cell's slice of `ids`
  const uint16_t* ids;         // ascending indices into `records`
  uint32_t* changed;           // per record of the chunk, zeroed by the caller
  uint32_t* extra;             // kResampleExtra words per record of the chunk, zeroed by the caller
  const uint8_t* palette_map;  // 256 grid bytes, as StampArgs::palette_map
  uint32_t n_cells;
};

// dry: nothing is written; every record is counted against the grid as it stands
hipError_t launch_resample(const ResampleArgs& a, bool dry, hipStream_t s);

}  // namespace dust
