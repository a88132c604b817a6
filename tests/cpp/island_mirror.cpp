// A host's "what did that explosion cut loose" through the C++ mirror (include/dust_hip.hpp): label the ground after a carve, move
// every island that does not touch the bottom layer into a geometry of its own (to fall as debris), delete the crumbs, commit.
// Compiled (not run) by tests/test_island_abi.py.
#include "dust_hip.hpp"

std::vector<std::unique_ptr<dust::VoxGeometry>> collapse(dust::Scene& scene, dust::VoxGeometry& ground, uint32_t crumb_voxels) {
  DustHipIslandQuery q{};
  q.struct_size = sizeof(q);
  q.connectivity = DUST_HIP_ISLANDS_FACES;
  q.anchor_hi[0] = q.anchor_hi[2] = 255;  // the y = 0 layer
  std::vector<std::unique_ptr<dust::VoxGeometry>> pieces;
  std::vector<uint32_t> crumbs;
  for (const DustHipIsland& island : ground.find_islands(q)) {
    if (island.flags & DUST_HIP_ISLAND_ANCHORED) continue;
    if (island.voxels <= crumb_voxels) crumbs.push_back(island.key);
    else pieces.push_back(ground.detach_islands({island.key}));
  }
  ground.detach_islands(crumbs, 0, false);
  const dust::UVec3 probe{0, 0, 0};
  if (ground.island_of({probe})[0] == DUST_HIP_NO_ISLAND) pieces.clear();
  scene.commit();
  return pieces;
}
