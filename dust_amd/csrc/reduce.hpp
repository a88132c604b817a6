// reduce.hpp -- interface between the host runtime (capi_model.cpp) and the model reduction kernel (reduce.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dust {

// one level of dust_hip_model_reduce as the kernel reads it (reduce_rule.hpp ReduceLevel, with the grids resolved)
struct ReduceArgs {
  const uint8_t* src;   // a grid of EditArgs::grid's layout, read inside [0, 2 * extent)^3; never `dst`
  uint8_t* dst;         // ... written inside [0, max(cover, 4))^3, whole bricks
  uint32_t extent;      // the coarse cube's side: 128, 64, ... 1
  uint32_t cover_log2;  // log2 of the bricks per side the launch covers, max(cover, 4) / 4
  uint32_t min_solid;   // 1..8
  uint32_t fresh;       // dst is zero wherever a zero would be stored: an empty brick is not stored
  uint32_t* count_src;  // null, or where the solid voxels read are added (zeroed by the caller)
  uint32_t* count_dst;  // null, or where the solid voxels written are added
};

hipError_t launch_reduce_level(const ReduceArgs& a, hipStream_t s);

}  // namespace dust
