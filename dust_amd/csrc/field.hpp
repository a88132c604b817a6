// field.hpp -- what the per-voxel uint16 fields of an editable model (the flood's steps, the distance transform's values, a fracture's cells) have in
// common once they are computed: the value that means "none", looking values up, and writing a grid byte where the value is in a range
// (kernels in field.hip). A field is brick-major like the grid (grid.hpp voxel_index).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid.hpp"

namespace dust {

constexpr uint32_t kFieldNone = 0xFFFFu;  // DUST_HIP_FLOOD_UNREACHED, DUST_HIP_DISTANCE_FAR: above every value, matched by no range

struct FieldApplyArgs {
  uint8_t* grid;
  const uint16_t* field;
  uint32_t lo, hi, byte;  // every voxel with value != kFieldNone and lo <= value <= hi takes the grid byte (0 = None)
  CellBox box;            // the root cells to visit: no voxel outside them has a value in the range
  uint32_t* changed;      // one word, zeroed by the caller
};

// out[i] = the entry of voxel xyz[3 i ..] (coordinates checked by the host): of a brick-major field, of the island labels (by key)
hipError_t launch_lookup(const uint16_t* field, const uint32_t* xyz, uint16_t* out, uint32_t n, hipStream_t s);
hipError_t launch_lookup(const uint32_t* label, const uint32_t* xyz, uint32_t* out, uint32_t n, hipStream_t s);
hipError_t launch_field_apply(const FieldApplyArgs& a, hipStream_t s);

}  // namespace dust
