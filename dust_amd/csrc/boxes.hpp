// boxes.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_boxes) and the boxes kernels (boxes.hip). The stacking
// rule itself is boxes_rule.hpp, on top of mesh_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "boxes_rule.hpp"
#include "grid.hpp"

namespace dust {

// What the device accumulates for a call, zeroed by the caller and added to with integer atomics (adds and maxima: no order shows):
// [0] rects of all slices, [1] those that continue the slice before (boxes = rects - continued), [2] voxels of S, [3 + k] 255 - the
// lowest coordinate of S on world axis k, [6 + k] the highest
constexpr uint32_t kBoxesAccWords = 9;
// one workgroup per slice of the stacking axis; its box starts are entry `slice` of the kLattice table the list pass scans
constexpr uint32_t kBoxesSlices = kMeshExtent;
// the D volume: a D plane (boxes_rule.hpp) per slice, 2 MiB
constexpr size_t kBoxesVolumeWords = size_t(kBoxesSlices) * kBoxesPlaneWords;

struct BoxesArgs {
  const uint64_t* brick_mask;  // EditArgs::brick_mask, or launch_cast_masks' array for a model that is not editable
  const uint8_t* grid;         // EditArgs::grid, only read; null when no material is needed (ANY_PALETTE without a filter, count pass)
  uint32_t axis;               // the stacking axis n, 0..2
  uint32_t byte;               // 0: every solid voxel; else only voxels holding this grid byte (palette index + 1)
  uint32_t any_palette;        // 1: runs, rects and boxes merge across materials
  uint32_t lo[3], hi[3];       // the inclusive region, clipped to the tree, lo <= hi
  uint32_t* acc;               // kBoxesAccWords (count pass)
  uint32_t* dvol;              // kBoxesVolumeWords: the count pass writes the D plane of every slice of the region, the list pass reads them
  uint32_t* slice_count;       // kLattice, zeroed by the caller: box starts per slice (count pass; null: counts only); after
                               // launch_table_scan the offsets the list pass reads, with its block sums in `scan_tmp`
  const uint32_t* scan_tmp;
  uint64_t* boxes;             // DustHipBox records as one word each (boxes_record), `capacity` of them (list pass)
  uint32_t capacity;
};

hipError_t launch_boxes_count(const BoxesArgs& a, hipStream_t s);
hipError_t launch_boxes_list(const BoxesArgs& a, hipStream_t s);

}  // namespace dust
