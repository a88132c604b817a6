// A host's "snow on every open top, and how much paint does the rest need?" through the C++ mirror (include/dust_hip.hpp): the
// surface is counted per material, listed, and its tops repainted. Compiled (not run) by tests/test_surface_abi.py.
#include "dust_hip.hpp"

struct Snowfall { uint32_t covered; uint32_t area; size_t spawn_points; };

Snowfall snow(dust::VoxGeometry& terrain, uint8_t snow_index) {
  DustHipSurfaceQuery all{};
  all.faces = DUST_HIP_FACES_ALL;
  all.palette = -1;
  for (int r = 0; r < 3; ++r) all.hi[r] = 255;
  DustHipSurfaceResult result{};
  std::vector<uint32_t> counts;
  const std::vector<DustHipSurfaceVoxel> voxels = terrain.surface(all, &result, &counts);   // every surface voxel with its open faces
  uint32_t area = 0;
  for (uint32_t d = 0; d < 6u; ++d)
    for (uint32_t p = 0; p < 255u; ++p) area += counts[d * DUST_HIP_SURFACE_BINS + 1u + p];  // == result.faces
  DustHipSurfaceQuery tops = all;
  tops.faces = DUST_HIP_FACE_POS_Y;
  const uint32_t covered = terrain.surface_apply(tops, snow_index);                          // the open tops take the snow's index
  static_assert(sizeof(DustHipSurfaceQuery) == 48 && sizeof(DustHipSurfaceResult) == 64 && sizeof(DustHipSurfaceVoxel) == 8 && DUST_HIP_SURFACE_BINS == 256u,
                "surface records");
  return Snowfall{covered, area + 0u * result.faces, voxels.size()};
}
