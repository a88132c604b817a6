// A host's collision and blast calls through the C++ mirror (include/dust_hip.hpp): is a player-sized box free, then remove every voxel
// a blast box covers. Compiled (not run) by tests/test_overlap_abi.py.
#include "dust_hip.hpp"

int blast(dust::Scene& scene, dust::VoxGeometry& model, const float centre[3], float radius) {
  DustHipBoxQuery player = {{centre[0] - 0.5f, centre[1], centre[2] - 0.5f}, 0u, {centre[0] + 0.5f, centre[1] + 2.0f, centre[2] + 0.5f}, 1u};
  DustHipVoxelRef touched;
  uint32_t hit = 0;
  scene.overlap_boxes(&player, 1, &hit, &touched, 1, /*any_hit=*/true);
  if (hit == 0) return 0;                       // the space is free
  std::vector<DustHipVoxelRef> records(4096);
  const DustHipBoxQuery box = {{centre[0] - radius, centre[1] - radius, centre[2] - radius}, 0u,
                               {centre[0] + radius, centre[1] + radius, centre[2] + radius}, uint32_t(records.size())};
  const std::vector<uint32_t> counts = scene.overlap_boxes(std::vector<DustHipBoxQuery>{box}, records);
  const uint32_t kept = counts[0] < records.size() ? counts[0] : uint32_t(records.size());
  for (uint32_t i = 0; i < kept; ++i)
    if (records[i].instance == touched.instance) model.set(dust::UVec3{records[i].xyz[0], records[i].xyz[1], records[i].xyz[2]}, std::nullopt);
  scene.commit();
  return int(kept);
}
