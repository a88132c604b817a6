// stamp.hpp -- interface between the host runtime (capi_model.cpp) and the model stamp kernel (stamp.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dust {

// One stamp of dust_hip_model_stamp as the device reads it: the caller's 32-byte record with the geometry folded into one affine map
// per destination axis, the image box clipped to the tree and the operation resolved into a table. Destination voxel d inside
// [lo, hi] reads the source voxel whose coordinate on SOURCE axis p[r] is base[r] + d[r] (g[r] == 0) or base[r] - d[r] (g[r] == 1),
// p and g the fields of `orient` as the header defines them. A clipped image has -255 <= offset <= 255, so base is a small integer.
// table: two bits per case (source solid) << 1 | (destination solid), what the destination voxel takes -- 0 keeps its byte,
// 1 the source's (mapped) byte, 2 None. Stamps that cover nothing are never listed in a cell.
constexpr uint32_t kStampKeep = 0, kStampTake = 1, kStampClear = 2;
struct DevStamp {  // 32 bytes
  int32_t base[3];
  uint32_t lo, hi;  // inclusive destination bounds, x | y << 8 | z << 16
  uint32_t orient;  // DustHipStamp::orient (valid: a permutation, bits 9.. zero)
  uint32_t table;
  uint32_t pad;
};
struct StampArgs {
  uint8_t* grid;               // the destination's EditArgs::grid
  const uint8_t* src;          // the source as a grid of the same layout; never the destination's own grid
  const DevStamp* stamps;      // the chunk's stamps, in call order
  const uint32_t* cells;       // n_cells root cells (16^3 voxels, (x>>4)<<8 | (y>>4)<<4 | (z>>4)) some stamp's image reaches
  const uint32_t* cell_start;  // n_cells + 1: each cell's slice of `ids`
  const uint16_t* ids;         // ascending indices into `stamps`
  uint32_t* changed;           // per stamp of the chunk, zeroed by the caller
  const uint8_t* palette_map;  // 256 grid bytes: [0] = 0 (None stays None), [i + 1] = the byte a source voxel of palette index i arrives as
  uint32_t n_cells;
};

hipError_t launch_stamp(const StampArgs& a, hipStream_t s);

}  // namespace dust
