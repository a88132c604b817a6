// A host's "the wall has a hole now: where do the drones go, and does the gas get out" through the C++ mirror (include/dust_hip.hpp):
// flood the air from the player, give every drone its next step, then test whether a room is sealed and fill it if it is.
// Compiled (not run) by tests/test_flood_abi.py.
#include "dust_hip.hpp"

std::vector<uint32_t> chase(dust::Scene& scene, dust::VoxGeometry& world, dust::UVec3 player, const std::vector<dust::UVec3>& drones,
                            dust::UVec3 room_lo, dust::UVec3 room_hi, uint8_t gas) {
  DustHipFloodQuery q{};
  q.medium = DUST_HIP_FLOOD_EMPTY;
  q.max_steps = DUST_HIP_FLOOD_MAX_STEPS;
  for (int k = 0; k < 3; ++k) q.hi[k] = 255;
  const DustHipFloodResult air = world.flood(q, {player});
  std::vector<uint32_t> next(drones.size(), DUST_HIP_NO_ISLAND);
  if (air.reached) {
    const std::vector<std::vector<uint32_t>> paths = world.flood_paths(drones, 2);
    for (size_t i = 0; i < paths.size(); ++i)
      if (paths[i].size() == 2) next[i] = paths[i][1];
    if (world.flood_at({drones.empty() ? player : drones[0]})[0] == DUST_HIP_FLOOD_UNREACHED) next.clear();
  }
  for (int k = 0; k < 3; ++k) { q.lo[k] = room_lo[k]; q.hi[k] = room_hi[k]; }
  q.max_steps = 64;
  if (world.flood(q, {room_lo}).boundary == 0 && world.flood_apply(gas, 32) != 0) scene.commit();
  return next;
}
