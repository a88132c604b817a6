// cast.hpp -- interface between the host runtime (capi_model.cpp) and the model cast kernels (cast.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dust_dev.h"

namespace dust {

// One cast of dust_hip_model_cast as the device reads it. Source voxel s inside [lo, hi] stands, at placement k, at
//   d_k[r] = off[r] + k * step[r] + u[r],   u[r] = s[p[r]] - lo[p[r]]  (g[r] == 0)  or  hi[p[r]] - s[p[r]]  (g[r] == 1),
// p and g the fields of `orient` as the header defines them. off is the caller's offset clamped to +-kCastOffsetLimit: beyond it an axis
// is outside the tree at every placement 0..65535 either way, so the clamp changes no answer and every sum above stays a small int32.
// The device walks placements k_lo..k_hi only (the host's int64 interval in which the image box meets the tree, cut to 0..max_steps;
// under WALLS it begins at 0 and ends one past the last placement the image is inside): at most kCastMaxWalk of them, whatever the
// offset. max_steps is the caller's, or 0 when step is zero (every placement is then placement 0).
constexpr int32_t kCastOffsetLimit = 1 << 20;
constexpr uint32_t kCastMaxWalk = 256 + 255 + 2;
constexpr uint32_t kCastWalls = 1u << 16;  // in DevCast::orient, above the header's nine bits
struct DevCast {  // 48 bytes
  int32_t off[3];
  uint32_t orient;  // DustHipCast::orient | kCastWalls
  int32_t step[3];
  uint32_t max_steps;
  uint32_t k_lo, k_hi;  // k_lo > k_hi: nothing to walk
  uint32_t lo, hi;      // the source sub-box, inclusive, x | y << 8 | z << 16
};
struct CastItem {  // one workgroup: a cast of the chunk and a source root cell (16^3 voxels) its sub-box reaches
  uint32_t cast, cell;
};
// what the second kernel adds up per cast
struct CastAcc {  // 16 bytes
  uint32_t contacts, voxels, wall, pad;
};
constexpr unsigned long long kCastNoHit = ~0ull;
struct CastArgs {
  const uint64_t* src_mask;  // the source's EditArgs::brick_mask (kLattice, iter_leaf order, bit x<<4 | y<<2 | z): no grid byte is read.
                             // A source that is not editable has no such array: its Block records carry the same 64-bit masks, so
                             // k_cast_masks scatters them into a 2 MiB context scratch (cheaper than the stamps' 16 MiB expansion: one
                             // thread per block, no material stream) and the source stays as it is
  const uint64_t* dst_mask;  // the destination's
  const DevCast* casts;      // the chunk's casts
  const CastItem* items;     // n_items work items
  unsigned long long* best;  // per cast of the chunk: min over its blocked voxels of (first blocked placement << 24 | source key); kCastNoHit
  CastAcc* acc;              // per cast of the chunk, zeroed by the caller
  uint32_t n_items;
};

hipError_t launch_cast_masks(uint64_t* mask /* kLattice, zeroed */, const DustHipBlock* blocks, uint32_t n_blocks, hipStream_t s);
hipError_t launch_cast(const CastArgs& a, hipStream_t s);  // the walk, then the count at the placement it found

}  // namespace dust
