// A host's "dig where the player clicked" through the C++ mirror (include/dust_hip.hpp): pick a voxel with a ray, carve a crater
// around its centre, pave the crater's floor, commit; the carve's count is the debris to spawn. Compiled (not run) by
// tests/test_shape_edit_abi.py.
#include "dust_hip.hpp"

uint32_t dig(dust::Scene& scene, dust::VoxGeometry& ground, const DustHipRay& click, float radius) {
  DustHipRayHit hit{};
  if (dust_hip_scene_trace_rays(scene.raw(), &click, &hit, 1, 0) != DUST_OK || hit.instance == DUST_HIP_NO_HIT) return 0;
  const float c[3] = {float(hit.xyz[0]) + 0.5f, float(hit.xyz[1]) + 0.5f, float(hit.xyz[2]) + 0.5f};  // tree coordinates: the voxel's centre
  DustHipEditShape crater{};
  crater.kind = DUST_HIP_SHAPE_SPHERE;
  crater.op = DUST_HIP_EDIT_CARVE;
  crater.radius = radius;
  DustHipEditShape floor{};
  floor.kind = DUST_HIP_SHAPE_BOX;
  floor.op = DUST_HIP_EDIT_PAINT;
  floor.palette = 17;
  for (int r = 0; r < 3; ++r) {
    crater.a[r] = c[r];
    floor.a[r] = c[r] - radius - 1.0f;
    floor.b[r] = c[r] + radius + 1.0f;
  }
  floor.b[1] = c[1] - radius;
  const std::vector<uint32_t> changed = ground.edit_shapes({crater, floor});
  scene.commit();
  return changed[0];
}
