// mesh.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_mesh) and the mesh kernels (mesh.hip). The merge rule
// itself is mesh_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "grid.hpp"
#include "mesh_rule.hpp"

namespace dust {

// What the device accumulates for a call, zeroed by the caller and added to with integer atomics (adds and one maximum: no order
// shows): [d] quads of direction d, [6 + d] faces of direction d (the quads' areas), [12] the area of the largest quad
constexpr uint32_t kMeshAccWords = 13;
// one workgroup per (direction, slice); its quad count is entry d << 8 | slice of the kLattice table the list pass scans
constexpr uint32_t kMeshSlices = kSurfaceFaces * kMeshExtent;
// the scan's scratch behind that table: 256 block sums (scan.hpp), then the total
constexpr uint32_t kMeshScanWords = 256 + 1;

struct MeshArgs {
  const uint64_t* brick_mask;  // EditArgs::brick_mask, or launch_cast_masks' array for a model that is not editable: all that decides exposure
  const uint8_t* grid;         // EditArgs::grid, only read; null when no material is needed (ANY_PALETTE without a filter, count pass)
  uint32_t faces;              // DUST_HIP_FACE_* bits that count, 1..63
  uint32_t walls;              // 1: the outside of the tree counts as solid
  uint32_t byte;               // 0: every solid voxel; else only voxels holding this grid byte (palette index + 1)
  uint32_t any_palette;        // 1: runs and quads merge across materials
  uint32_t lo[3], hi[3];       // the inclusive region, clipped to the tree, lo <= hi
  uint32_t* acc;               // kMeshAccWords (count pass)
  uint32_t* slice_count;       // kLattice, zeroed by the caller: quads per (direction, slice) at d << 8 | slice (count pass); after
                               // launch_table_scan the offsets the list pass reads, with its block sums in `scan_tmp`
  const uint32_t* scan_tmp;
  uint64_t* quads;             // DustHipMeshQuad records as one word each (mesh_record), `capacity` of them (list pass)
  uint32_t capacity;
};

hipError_t launch_mesh_count(const MeshArgs& a, hipStream_t s);
hipError_t launch_mesh_list(const MeshArgs& a, hipStream_t s);

}  // namespace dust
