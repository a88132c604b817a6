// A terrain pass through the C++ mirror (include/dust_hip.hpp): the height map of a block seen from above, its mean height, then the
// oldest terrain edit there is -- the top voxel of every column becomes grass, the four stone voxels under it dirt -- and a voxel of
// snow on everything under open sky. Compiled (not run) by tests/test_column_abi.py.
#include "dust_hip.hpp"

struct Terrain { std::vector<uint8_t> height; double mean_depth; uint32_t occupied; uint32_t painted; };

Terrain dress_terrain(dust::VoxGeometry& block, uint8_t grass, uint8_t dirt, uint8_t stone, uint8_t snow) {
  DustHipColumnsQuery top{};
  top.face = DUST_HIP_FACE_POS_Y;                                        // looked at from above, walking down
  top.palette = -1;
  for (int r = 0; r < 3; ++r) top.hi[r] = 255;
  DustHipColumnsResult result{};
  std::vector<uint32_t> counts;
  const std::vector<DustHipColumnCell> map = block.columns(top, &result, &counts);   // [x][z], z fastest
  Terrain t{};
  for (const DustHipColumnCell& c : map) t.height.push_back(c.palette == 255 ? 0 : uint8_t(c.at));
  t.mean_depth = result.hit ? double(result.depth_sum) / result.hit : 0.0;
  t.occupied = result.columns - counts[0];                               // bin 0: the columns with nothing in them
  t.painted = block.columns_apply(top, DUST_HIP_COLUMNS_RUN, 1, grass);
  DustHipColumnsQuery under = top;
  under.palette = stone;                                                 // grass is see-through for a stone filter
  t.painted += block.columns_apply(under, DUST_HIP_COLUMNS_RUN, 4, dirt);
  t.painted += block.columns_apply(top, DUST_HIP_COLUMNS_GAP, 1, snow);
  static_assert(sizeof(DustHipColumnsQuery) == 48 && sizeof(DustHipColumnsResult) == 64 && sizeof(DustHipColumnCell) == 4 && DUST_HIP_COLUMNS_BINS == 256u &&
                    DUST_HIP_COLUMNS_NO_KEY == 0xFFFFFFFFu,
                "columns records");
  return t;
}
