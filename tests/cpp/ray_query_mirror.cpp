// A host's picking call through the C++ mirror (include/dust_hip.hpp): the voxel under the cursor, then removing it and placing one
// on the face it was hit through. Compiled (not run) by tests/test_ray_query_abi.py.
#include "dust_hip.hpp"

int pick_and_dig(dust::Scene& scene, dust::VoxGeometry& model, const float eye[3], const float dir[3]) {
  DustHipRay ray = {{eye[0], eye[1], eye[2]}, 0.1f, {dir[0], dir[1], dir[2]}, 1e4f};
  const std::vector<DustHipRayHit> hits = scene.trace_rays(std::vector<DustHipRay>{ray});
  if (hits[0].instance == DUST_HIP_NO_HIT) return 0;
  const uint32_t axis = hits[0].face >> 1u;
  const int step = (hits[0].face & 1u) ? 1 : -1;
  dust::UVec3 at = {hits[0].xyz[0], hits[0].xyz[1], hits[0].xyz[2]};
  const uint8_t colour = hits[0].palette;
  model.set(at, std::nullopt);                  // dig it out
  at[axis] = uint32_t(int(at[axis]) + step);
  model.set(at, colour);                        // place one on the face it was hit through
  scene.commit();
  DustHipRayHit any;
  scene.trace_rays(&ray, &any, 1, /*any_hit=*/true);
  return 1 + int(any.instance != DUST_HIP_NO_HIT);
}
