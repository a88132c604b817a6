// neighbour.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_neighbours, _neighbours_apply) and the neighbourhood
// kernels (neighbour.hip). The rule itself is neighbour_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "grid.hpp"
#include "neighbour_rule.hpp"

namespace dust {

// What the device accumulates for a read-only call, zeroed by the caller and added to with integer atomics (adds and maxima: no order
// shows): [0] voxels of the region, [1] the solid ones, [2] born, [3] died, [4 + r] 255 - the lower bound of the changing voxels on axis
// r, [7 + r] their upper bound; behind it the table, 2 * kNeighbourBins words (the empty row, then the solid row)
constexpr uint32_t kNeighbourAccWords = 10;
constexpr uint32_t kNeighbourTableWords = 2 * kNeighbourBins;
// ... and per generation of an apply: [0] born, [1] died, [2 + r] 255 - the lower bound, [5 + r] the upper bound. An apply's array holds
// kNeighbourMaxGenerations such slots and, behind them, one word: the solid voxels of the region before the first generation
constexpr uint32_t kNeighbourSlotWords = 8;
constexpr uint32_t kNeighbourMaxGenerations = 256;
constexpr uint32_t kNeighbourApplyWords = kNeighbourMaxGenerations * kNeighbourSlotWords + 1;
// the library looks at the slots every so many generations and stops launching once one of them changed nothing
constexpr uint32_t kNeighbourCheckEvery = 8;

struct NeighbourArgs {
  const uint64_t* brick_mask;  // EditArgs::brick_mask, or launch_cast_masks' array for a model that is not editable: all the read-only call reads
  uint32_t neighbourhood;      // 6, 18 or 26
  uint32_t walls;              // 1: the outside of the tree counts as solid
  uint32_t birth, survive;     // bit masks over the count
  uint32_t lo[3], hi[3];       // the inclusive region, lo <= hi
  CellBox box;                 // the root cells it reaches: one workgroup each
  uint32_t* acc;               // kNeighbourAccWords (k_neighbours)
  uint32_t* table;             // kNeighbourTableWords, zeroed by the caller; null: no table was asked for (k_neighbours)
};
struct NeighbourStepArgs {
  NeighbourArgs q;             // brick_mask: the masks the generation reads; neighbourhood, walls, birth, survive, lo, hi, box; the rest unused
  const uint8_t* grid;         // the grid the generation reads (a survivor's byte, the votes of a born voxel's neighbours)
  uint8_t* grid_out;           // the grid it writes: never the one it reads. Every brick the region reaches is written whole; the rest is
                               // left alone (the caller made both grids equal there)
  uint64_t* mask_out;          // ... and the masks
  uint32_t byte;               // a born voxel's grid byte (palette index + 1); under `majority` the fallback where nobody votes
  uint32_t majority;           // 1: a born voxel takes the byte most of its solid neighbours hold, the lowest among equals
  uint32_t* slot;              // kNeighbourSlotWords: this generation's, zeroed by the caller
  uint32_t* solid;             // one word, zeroed by the caller: the region's solid voxels as the generation found them; null: not counted
};

hipError_t launch_neighbours(const NeighbourArgs& a, hipStream_t s);
hipError_t launch_neighbours_step(const NeighbourStepArgs& a, hipStream_t s);

}  // namespace dust
