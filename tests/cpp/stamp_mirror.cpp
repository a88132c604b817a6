// A host's "the debris has come to rest" through the C++ mirror (include/dust_hip.hpp): a detached piece is stamped back into the
// ground a few voxels lower and turned a quarter about y, its materials renamed, and the scene commits. Compiled (not run) by
// tests/test_stamp_witness.py.
#include "dust_hip.hpp"

uint32_t settle(dust::Scene& scene, dust::VoxGeometry& ground, const dust::VoxGeometry& piece, const DustHipIsland& island, int32_t drop) {
  DustHipStamp s{};
  s.offset[0] = island.lo[0];
  s.offset[1] = int32_t(island.lo[1]) - drop;
  s.offset[2] = island.lo[2];
  s.orient = 2u | (1u << 2) | (0u << 4) | (1u << 6);  // x reads z backwards, z reads x: a quarter turn about y
  s.op = DUST_HIP_STAMP_PLACE;
  for (int k = 0; k < 3; ++k) { s.src_lo[k] = island.lo[k]; s.src_hi[k] = island.hi[k]; }
  std::array<uint8_t, 255> rubble{};
  for (size_t i = 0; i < rubble.size(); ++i) rubble[i] = uint8_t(i % 4);
  const uint32_t placed = ground.stamp(piece, {s}, &rubble)[0];
  ground.stamp(ground, {s});  // onto itself: the source is read as it stood when the call began
  scene.commit();
  return placed;
}
