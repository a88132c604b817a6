// A host's "what will this blast remove, and what does it weigh?" through the C++ mirror (include/dust_hip.hpp): the crater is
// described once, counted, and carved with the same array. Compiled (not run) by tests/test_census_abi.py.
#include "dust_hip.hpp"

struct Blast { uint32_t removed; double weight; float centre[3]; };

Blast blast(dust::VoxGeometry& terrain, const float at[3], float radius, const float density[255]) {
  DustHipEditShape crater{};
  crater.kind = DUST_HIP_SHAPE_SPHERE;
  crater.op = DUST_HIP_EDIT_CARVE;
  crater.radius = radius;
  for (int r = 0; r < 3; ++r) crater.a[r] = at[r];
  const std::vector<DustHipEditShape> shapes{crater};
  std::vector<uint32_t> counts;
  const std::vector<DustHipCensus> records = terrain.census(shapes, &counts);  // ask first
  Blast b{records[0].solid, 0.0, {0.0f, 0.0f, 0.0f}};
  for (uint32_t p = 0; p < 255u; ++p) b.weight += double(counts[1 + p]) * double(density[p]);
  if (records[0].solid)
    for (int r = 0; r < 3; ++r) b.centre[r] = float(double(records[0].sum[r]) / double(records[0].solid) + 0.5);
  const std::vector<uint32_t> changed = terrain.edit_shapes(shapes);            // carve after: changed[0] == records[0].solid
  (void)changed;
  static_assert(sizeof(DustHipCensus) == 40 && DUST_HIP_CENSUS_BINS == 256u && DUST_HIP_MAX_CENSUS_TABLES == 4096u && DUST_HIP_MAX_CENSUS_SHAPES == 65536u,
                "census records");
  return b;
}
