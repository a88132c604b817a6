// triangle.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_edit_triangles, _fill_mesh) and the voxelisation
// kernels (triangle.hip). The rule itself is triangle_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "edit.hpp"  // kEditKeep: an operation as the two grid bytes it writes
#include "grid.hpp"
#include "triangle_rule.hpp"

namespace dust {

// One triangle as the device reads it: the caller's vertices, the operation resolved into the two grid bytes it writes (edit_triangles;
// fill_mesh leaves them 0) and the inclusive voxel bounds the cell lists are made from -- for edit_triangles the voxels the vertices'
// extent touches, for fill_mesh the columns whose centre lies in that extent, with z = 0. Triangles that cover nothing are never listed.
struct DevTriangle {  // 52 bytes
  int32_t v[3][3];
  uint32_t solid_to, empty_to;  // the grid byte (palette index + 1, 0 = None) a covered solid / empty voxel takes; kEditKeep: it keeps its byte
  uint32_t lo, hi;              // x | y << 8 | z << 16, clipped to the tree (fill_mesh: to the region's columns)
};

struct EditTriangleArgs {  // the fields of EditShapeArgs: batched_edit fills them in
  uint8_t* grid;
  const DevTriangle* triangles;  // the chunk's triangles, in call order
  const uint32_t* cells;
  const uint32_t* cell_start;
  const uint16_t* ids;
  uint32_t* changed;
  uint32_t n_cells;
};

// k_fill_columns: a chunk of a mesh's crossing triangles binned by 16 x 16 column tile (the root cells with z = 0)
struct FillColumnsArgs {
  uint64_t* volume;              // kLattice words in EditArgs::brick_mask's layout: bit set = the voxel's centre is inside. XORed into.
  const DevTriangle* triangles;
  const uint32_t* cells;         // n_cells tiles, (x >> 4) << 8 | (y >> 4) << 4
  const uint32_t* cell_start;
  const uint16_t* ids;
  uint32_t n_cells;
};

// k_fill_apply: the operation on the inside voxels of the region
constexpr uint32_t kFillAccWords = 8;  // covered, changed, 255 - lo[3], hi[3]
struct FillApplyArgs {
  uint8_t* grid;
  const uint64_t* volume;
  uint32_t solid_to, empty_to;
  uint32_t lo[3], hi[3];  // the region
  CellBox box;            // the root cells it reaches
  uint32_t* acc;          // kFillAccWords, zeroed by the caller
};

hipError_t launch_edit_triangles(const EditTriangleArgs& a, hipStream_t s);
hipError_t launch_fill_columns(const FillColumnsArgs& a, hipStream_t s);
hipError_t launch_fill_apply(const FillApplyArgs& a, hipStream_t s);

}  // namespace dust
