// A wall broken into chunks through the C++ mirror (include/dust_hip.hpp): seeds scattered around an impact, the voxels within reach
// labelled, every non-empty cell copied into a geometry of its own, then all of them removed from the wall in one carving detach -- the
// header's recipe: the wall is rebuilt once. Compiled (not run) by tests/test_fracture_abi.py.
#include <memory>
#include <vector>

#include "dust_hip.hpp"

struct Chunks {
  std::vector<std::unique_ptr<dust::VoxGeometry>> pieces;
  uint32_t cut_faces;
};

Chunks shatter(dust::VoxGeometry& wall, const std::vector<DustHipFractureSeed>& seeds, uint32_t reach) {
  DustHipFractureQuery q{};
  q.palette = -1;                                                     // every material breaks
  q.max_distance2 = reach * reach;                                    // local damage
  q.scale[0] = 1; q.scale[1] = 4; q.scale[2] = 1;                     // splinters along y
  for (int r = 0; r < 3; ++r) q.hi[r] = 255;
  const dust::VoxGeometry::Fractured f = wall.fracture(q, seeds);
  Chunks out{};
  out.cut_faces = f.result.cut_faces;
  if (f.result.cells == 0) return out;
  std::vector<uint32_t> broken;
  for (uint32_t i = 0; i < f.cells.size(); ++i) {
    if (f.cells[i].voxels == 0) continue;
    out.pieces.push_back(wall.fracture_detach({i}, DUST_HIP_DETACH_KEEP_SOURCE));
    broken.push_back(i);
  }
  wall.fracture_detach(broken, 0, false);                             // one rebuild of the wall
  if (wall.fracture_at({{0, 0, 0}})[0] != DUST_HIP_NO_CELL) wall.fracture_apply(DUST_HIP_FRACTURE_LABELLED, std::nullopt);
  static_assert(sizeof(DustHipFractureSeed) == 16 && sizeof(DustHipFractureQuery) == 48 && sizeof(DustHipFractureResult) == 64 &&
                    sizeof(DustHipFractureCell) == 40 && DUST_HIP_MAX_FRACTURE_SEEDS == 4096u && DUST_HIP_NO_CELL == 0xFFFFu,
                "fracture records");
  return out;
}
