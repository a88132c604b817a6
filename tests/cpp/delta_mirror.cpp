// A host's undo stack through the C++ mirror (include/dust_hip.hpp): what an edit changed is listed against a snapshot, the removed
// voxels are counted per material for the particles, and the list is played backwards to undo. Compiled (not run) by
// tests/test_delta_abi.py.
#include "dust_hip.hpp"

struct Undone { uint32_t restored; uint32_t conflicts; uint32_t debris; size_t records; };

Undone undo_last_edit(const dust::VoxGeometry& snapshot, dust::VoxGeometry& live) {
  DustHipDeltaQuery all{};
  all.kinds = DUST_HIP_DELTA_ALL;
  all.palette = -1;
  for (int r = 0; r < 3; ++r) all.hi[r] = 255;
  DustHipDeltaResult result{};
  std::vector<uint32_t> counts;
  const std::vector<DustHipDeltaVoxel> change = snapshot.delta(live, all, &result, &counts);   // snapshot -> live, every changed voxel
  uint32_t debris = 0;
  for (uint32_t p = 0; p < 255u; ++p) debris += counts[0 * DUST_HIP_DELTA_BINS + 1u + p];      // the listed voxels that held a material before
  uint32_t conflicts = 0;
  const uint32_t restored = live.delta_apply(change, true, &conflicts);                          // backwards: live takes `before`
  static_assert(sizeof(DustHipDeltaQuery) == 48 && sizeof(DustHipDeltaResult) == 64 && sizeof(DustHipDeltaVoxel) == 8 && DUST_HIP_DELTA_BINS == 256u &&
                    DUST_HIP_DELTA_NONE == 255u,
                "delta records");
  return Undone{restored, conflicts, debris + 0u * result.removed, change.size()};
}
