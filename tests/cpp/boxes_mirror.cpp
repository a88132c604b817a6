// A host's "compound collider for the rigid-body solver, one per detached piece" through the C++ mirror (include/dust_hip.hpp): the
// piece's solid voxels come back merged into boxes, materials ignored, as inclusive voxel bounds. Compiled (not run) by
// tests/test_boxes_abi.py.
#include "dust_hip.hpp"

struct Piece { uint32_t lo[3], hi[3]; };  // inclusive voxel bounds of one convex piece

std::vector<Piece> compound(const dust::VoxGeometry& island, uint32_t* volume) {
  DustHipBoxesQuery all{};
  all.axis = 1;  // stack along y last
  all.flags = DUST_HIP_BOXES_ANY_PALETTE;
  all.palette = -1;
  for (int r = 0; r < 3; ++r) all.hi[r] = 255;
  DustHipBoxesResult result{};
  const std::vector<DustHipBox> boxes = island.boxes(all, &result);
  std::vector<Piece> out;
  out.reserve(boxes.size());
  for (const DustHipBox& b : boxes) {
    Piece p{};
    p.lo[0] = b.key >> 16; p.lo[1] = (b.key >> 8) & 255u; p.lo[2] = b.key & 255u;
    p.hi[0] = p.lo[0] + b.dx; p.hi[1] = p.lo[1] + b.dy; p.hi[2] = p.lo[2] + b.dz;
    out.push_back(p);
  }
  static_assert(sizeof(DustHipBoxesQuery) == 48 && sizeof(DustHipBoxesResult) == 64 && sizeof(DustHipBox) == 8, "boxes records");
  if (volume) *volume = result.voxels;
  return out;
}
