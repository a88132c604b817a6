// A host's "the props beyond the second ring get a coarser model" through the C++ mirror (include/dust_hip.hpp): reduce the prop as it
// stands on the device by two levels, keeping every voxel's footprint (min_solid 1: no holes), and spawn the copy where the distant
// instances stand. Compiled (not run) by tests/test_reduce_abi.py.
#include "dust_hip.hpp"

std::unique_ptr<dust::VoxGeometry> distant_props(dust::Scene& scene, const dust::VoxGeometry& prop, const float (*far_transforms)[12], uint32_t n) {
  DustHipReduceResult counts{};
  std::unique_ptr<dust::VoxGeometry> coarse = prop.reduce(2, 1, &counts);
  if (counts.voxels == 0 || counts.extent != 64) return nullptr;  // an empty prop: nothing to show
  for (uint32_t i = 0; i < n; ++i) scene.spawn(*coarse, dust::VoxGeometry::lod_transform(far_transforms[i], 2).data());
  scene.commit();
  static_assert(DUST_HIP_REDUCE_MAX_LEVELS == 8u && sizeof(DustHipReduce) == 16 && sizeof(DustHipReduceResult) == 16, "reduce records");
  return coarse;
}
