// A host's "the snow has fallen and the cave has to fit the boss" through the C++ mirror (include/dust_hip.hpp): grow the terrain by
// two voxels of snow, then ask whether a ball of the boss's radius fits at the spawn point and where the roomiest spot is otherwise.
// Compiled (not run) by tests/test_distance_abi.py.
#include "dust_hip.hpp"

uint32_t snow_and_spawn(dust::Scene& scene, dust::VoxGeometry& world, dust::UVec3 spawn, uint32_t boss_radius, uint8_t snow) {
  DustHipDistanceQuery q{};
  q.target = DUST_HIP_DISTANCE_TO_SOLID;
  q.metric = DUST_HIP_DISTANCE_EUCLIDEAN;
  q.max_radius = 2;
  if (world.distance(q).near != 0 && world.distance_apply(snow, 1, 4) != 0) scene.commit();
  q.flags = DUST_HIP_DISTANCE_WALLS;
  q.max_radius = DUST_HIP_DISTANCE_MAX_RADIUS;
  const DustHipDistanceResult room = world.distance(q);
  const uint16_t here = world.distance_at({spawn})[0];
  if (here == DUST_HIP_DISTANCE_FAR || here > boss_radius * boss_radius) return uint32_t(spawn[0]) << 16 | uint32_t(spawn[1]) << 8 | uint32_t(spawn[2]);
  return room.largest > boss_radius * boss_radius ? room.largest_key : DUST_HIP_DISTANCE_NO_KEY;
}
