// A physics hull brought into a block through the C++ mirror (include/dust_hip.hpp): fill the inside of a closed triangle mesh with
// stone, then draw its surface over it in a second material, vertices rounded from floats in voxels to the ABI's 1/256 voxel.
// Compiled (not run) by tests/test_triangle_abi.py.
#include <array>
#include <cmath>

#include "dust_hip.hpp"

struct Imported { uint32_t inside, shell; };

static DustHipTriangle triangle_of(const float (&v)[3][3], uint32_t op, int32_t palette) {
  DustHipTriangle t{};
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) t.v[k][r] = int32_t(std::lrint(double(v[k][r]) * DUST_HIP_TRIANGLE_UNIT));   // not clamped: out of range covers nothing
  t.op = op;
  t.palette = palette;
  return t;
}

Imported import_hull(dust::VoxGeometry& block, const std::vector<std::array<std::array<float, 3>, 3>>& hull) {
  std::vector<DustHipTriangle> triangles;
  for (const auto& face : hull) {
    const float v[3][3] = {{face[0][0], face[0][1], face[0][2]}, {face[1][0], face[1][1], face[1][2]}, {face[2][0], face[2][1], face[2][2]}};
    triangles.push_back(triangle_of(v, DUST_HIP_EDIT_FILL, 12));
  }
  DustHipFillMeshQuery stone{};
  stone.op = DUST_HIP_EDIT_PLACE;                                     // what is there stays
  stone.palette = 3;
  for (int r = 0; r < 3; ++r) stone.hi[r] = 255;
  const DustHipFillMeshResult filled = block.fill_mesh(triangles, stone);
  Imported out{};
  out.inside = filled.covered;
  if (filled.crossing == 0) return out;                               // nothing but vertical faces: no inside
  for (uint32_t n : block.edit_triangles(triangles)) out.shell += n;  // the surface, triangle by triangle, in order
  static_assert(sizeof(DustHipTriangle) == 48 && sizeof(DustHipFillMeshQuery) == 48 && sizeof(DustHipFillMeshResult) == 48 &&
                    DUST_HIP_MAX_EDIT_TRIANGLES == 65536u && DUST_HIP_MAX_MESH_TRIANGLES == 1048576u,
                "triangle records");
  return out;
}
