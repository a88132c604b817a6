// A host's "the debris falls" through the C++ mirror (include/dust_hip.hpp): a detached piece is cast straight down inside the ground it
// came from, with the tree's faces as walls, and stamped where it comes to rest; a prefab is placed only where it fits.
// Compiled (not run) by tests/test_cast_abi.py.
#include "dust_hip.hpp"

uint32_t settle(dust::Scene& scene, dust::VoxGeometry& ground, const dust::VoxGeometry& piece, const DustHipIsland& island,
                const dust::VoxGeometry& prefab, const int32_t (&site)[3]) {
  DustHipCast fall{};
  for (int k = 0; k < 3; ++k) { fall.offset[k] = island.lo[k]; fall.src_lo[k] = island.lo[k]; fall.src_hi[k] = island.hi[k]; }
  fall.orient = 0x24;
  fall.step[1] = -1;
  fall.max_steps = DUST_HIP_CAST_MAX_STEPS;
  fall.flags = DUST_HIP_CAST_WALLS;
  const DustHipCastHit hit = ground.cast(piece, {fall})[0];
  uint32_t placed = 0;
  if (!(hit.flags & DUST_HIP_CAST_OVERLAP)) {
    DustHipStamp rest{};
    for (int k = 0; k < 3; ++k) {
      rest.offset[k] = fall.offset[k] + int32_t(hit.steps) * fall.step[k];
      rest.src_lo[k] = fall.src_lo[k]; rest.src_hi[k] = fall.src_hi[k];
    }
    rest.orient = fall.orient;
    rest.op = DUST_HIP_STAMP_PLACE;
    placed = ground.stamp(piece, {rest})[0];
  }
  DustHipCast fit{};  // max_steps 0: a fit test
  for (int k = 0; k < 3; ++k) { fit.offset[k] = site[k]; fit.src_hi[k] = 63; }
  fit.orient = 0x24;
  const DustHipCastHit there = ground.cast(prefab, {fit})[0];
  if (there.flags == 0 && there.voxels != 0 && there.src_key == DUST_HIP_CAST_NO_KEY) {
    DustHipStamp put{};
    for (int k = 0; k < 3; ++k) { put.offset[k] = site[k]; put.src_hi[k] = 63; }
    put.orient = 0x24;
    placed += ground.stamp(prefab, {put})[0];
  }
  scene.commit();
  return placed;
}
