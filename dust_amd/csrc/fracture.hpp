// fracture.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_fracture, _fracture_detach, _fracture_apply) and
// the fracture kernels (fracture.hip). The rule itself is fracture_rule.hpp; the labels are a per-voxel field of field.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fracture_rule.hpp"
#include "grid.hpp"

namespace dust {

// What the device accumulates for the result record, zeroed by the caller and added to with integer atomics (adds and maxima: no order
// shows): [0] counted voxels, [1] labelled ones, [2] cut faces (each once), [3] the largest d2 of a labelled voxel to its seed,
// [4 + r] 255 - the lower bound of the labelled voxels on axis r, [7 + r] their upper bound, [10] cells with a voxel,
// [12], [13] the largest cell as one 64-bit maximum: voxels << 32 | ~index (the lowest index among equals)
constexpr uint32_t kFractureAccWords = 16;
constexpr uint32_t kFractureSolid = 0, kFractureLabelled = 1, kFractureCut = 2, kFractureMaxD2 = 3, kFractureLo = 4, kFractureHi = 7, kFractureCells = 10,
                   kFractureLargest = 12;
constexpr uint32_t kFractureSelectWords = kFractureMaxSeeds / 64;  // a bit per cell index

// One cell while its record is being accumulated: IslandAcc's zero-initialised form, the lower bounds kept as 255 - lo (atomicMax).
struct FractureAcc {  // 64 bytes
  uint32_t voxels, cut_faces;
  uint32_t inv_lo[3], hi[3];
  uint32_t pad[2];
  unsigned long long sum[3];
};
struct DevFractureCell {  // DustHipFractureCell, 40 bytes
  uint32_t voxels, cut_faces;
  uint32_t lo, hi;  // lo[0] | lo[1] << 8 | lo[2] << 16 (255, 255, 255 when empty); hi the same (0, 0, 0)
  uint32_t sum[6];  // three little-endian uint64
};
struct DevFractureSeed {  // DustHipFractureSeed, 16 bytes
  int32_t x, y, z;
  uint32_t reserved;
};
static_assert(sizeof(FractureAcc) == 64 && sizeof(DevFractureCell) == 40 && sizeof(DevFractureSeed) == 16, "fracture records");

struct FractureArgs {
  const uint8_t* grid;          // EditArgs::grid: read under a palette filter only
  const uint64_t* brick_mask;   // the solid voxels per brick (EditArgs::brick_mask), as the last rebuild left them
  uint16_t* field;              // kLattice * 64 labels, brick-major like the grid; every entry kFractureNoCell before k_fracture_label runs
  const DevFractureSeed* seeds;
  uint32_t n_seeds;
  uint32_t byte;                // the filter's grid byte (palette index + 1), 0: every solid voxel
  uint32_t limit;               // max_distance2, kFractureNoLimit: none
  uint32_t scale[3];
  uint32_t lo[3], hi[3];        // the inclusive region, clipped to the tree and not empty
  CellBox box;                  // the root cells it reaches: one workgroup each
  uint32_t cull;                // 0: every seed is a candidate of every cell (the measurement's switch)
  uint32_t* acc;                // kFractureAccWords
  FractureAcc* cells;           // n_seeds accumulators, zeroed by the caller (k_fracture_records)
  DevFractureCell* records;     // n_seeds records (k_fracture_emit)
};

struct FractureDetachArgs {
  uint8_t* src;              // the source model's grid
  uint8_t* dst;              // the new model's grid (every byte is written), or null
  uint16_t* field;           // the source's labels
  const uint64_t* selected;  // kFractureSelectWords: bit set for every cell being detached
  uint32_t carve;            // remove the voxels from the source, and their labels
};

struct FractureApplyArgs {
  uint8_t* grid;
  const uint16_t* field;
  uint32_t seams;    // 1: the labelled voxels with a face-neighbour of a higher cell; 0: every labelled voxel
  uint32_t byte;     // what they take (0 = None)
  CellBox box;       // the root cells that can hold a label
  uint32_t* changed; // one word, zeroed by the caller
};

// a.field cleared to kFractureNoCell, then the labels of the region's counted voxels; a.acc [solid], [labelled], [max d2]
hipError_t launch_fracture_label(const FractureArgs& a, hipStream_t s);
// the per-cell accumulators and the rest of a.acc from the labels, then the packed records and the largest cell
hipError_t launch_fracture_records(const FractureArgs& a, hipStream_t s);
hipError_t launch_fracture_detach(const FractureDetachArgs& a, hipStream_t s);
hipError_t launch_fracture_apply(const FractureApplyArgs& a, hipStream_t s);

}  // namespace dust
