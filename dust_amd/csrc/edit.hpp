// edit.hpp -- interface between the host runtime (capi_model.cpp) and the device-side tree rebuild (edit.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dust_dev.h"
#include "grid.hpp"  // the grid's brick order (leaf_code, kLattice): every kernel file of the model calls reads it from there

namespace dust {

constexpr uint32_t kSrgbRow = 64 * 255 + 1;  // colour sums 0 .. 64 * 255 per voxel count

struct EditHeader {  // what the host reads back after a rebuild
  uint32_t n_blocks, n_mid;
  uint32_t n_materials, pad;  // (at most 2^24: a byte per voxel)
  float bmin[3], bmax[3];
};

struct EditArgs {
  uint8_t* grid;             // kLattice * 64 bytes: palette index + 1 per voxel, [iter_leaf brick code][bit x<<4 | y<<2 | z]
  uint64_t* brick_mask;      // kLattice, iter_leaf order
  uint32_t* flag_leaf;       // kLattice (+ scan): brick non-empty, iter_leaf order   -> block index
  uint32_t* count_major;     // kLattice (+ scan): voxels per brick, collector order  -> material_ptr
  uint32_t* scan_tmp;        // 2 * 256 block sums
  DustHipBlock* blocks;      // capacity kLattice
  uint8_t* materials;        // capacity kLattice * 64
  const uint32_t* palette;   // RGBA8 x 256
  const uint16_t* srgb_lut;  // [64][kSrgbRow]: trunc(linear2srgb(sum / (n * 255)) * 1023), evaluated on the host
  uint8_t* root;             // one N16 node (kN16Bytes)
  DevN4* mid;                // capacity 4096
  uint64_t* dense_mask;      // capacity 4096 * 64
  EditHeader* header;
  // edit batch
  const uint32_t* xyz;
  const int32_t* values;
  int32_t* values_out;
  uint32_t n_edits;
};

// One shape of dust_hip_model_edit_shapes as the device reads it: the caller's 48-byte record with the operation resolved into the
// two grid bytes it writes and the shape's conservative voxel bounds. Shapes that cover nothing are never listed in a cell.
constexpr uint32_t kEditKeep = 256;  // solid_to: a solid voxel keeps its byte (PLACE)
struct DevEditShape {  // 48 bytes
  float a[3]; uint32_t kind;
  float b[3]; float radius;
  uint32_t solid_to, empty_to;  // the grid byte (palette index + 1, 0 = None) a covered solid / empty voxel takes
  uint32_t lo, hi;              // inclusive voxel bounds, x | y << 8 | z << 16, clipped to the tree: they cull, the float32 formulas decide
};
struct EditShapeArgs {
  uint8_t* grid;                // EditArgs::grid
  const DevEditShape* shapes;   // the chunk's shapes, in call order
  const uint32_t* cells;        // n_cells root cells (16^3 voxels, (x>>4)<<8 | (y>>4)<<4 | (z>>4)) some shape's bounds reach
  const uint32_t* cell_start;   // n_cells + 1: each cell's slice of `ids`
  const uint16_t* ids;          // ascending indices into `shapes`
  uint32_t* changed;            // per shape of the chunk, zeroed by the caller
  uint32_t n_cells;
};

hipError_t launch_edit_expand(const EditArgs& e, const DustHipBlock* blocks, const uint8_t* materials, uint32_t n_blocks, hipStream_t s);
hipError_t launch_edit_apply(const EditArgs& e, bool read, hipStream_t s);
hipError_t launch_edit_rebuild(const EditArgs& e, hipStream_t s);
hipError_t launch_edit_shapes(const EditShapeArgs& a, hipStream_t s);

}  // namespace dust
