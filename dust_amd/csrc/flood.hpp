// flood.hpp -- interface between the host runtime (capi_model.cpp) and the step-distance floods of an editable model (flood.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dust {

constexpr uint32_t kFloodBatch = 8;            // relaxation passes launched per read-back of the worklist's length

// the context's flood scratch, in 32-bit words (L = kLattice): two flag arrays and two worklists that take turns, three worklist lengths
// (read / appended to / zeroed for the pass after next) and the accumulator of the result reduction
constexpr size_t kFloodFlag = 0, kFloodList = 2, kFloodCount = 4;  // flag[k] at (kFloodFlag + k) * L, list[k] at (kFloodList + k) * L, the counts at kFloodCount * L
constexpr size_t kFloodAcc = 4;                                    // words behind the counts
constexpr size_t kFloodAccWords = 12;                              // reached, farthest, seeds_used, boundary, 255 - lo[3], hi[3], changed (apply), pad
constexpr size_t kFloodWorkWords = 16;                             // words behind the four arrays

struct FloodArgs {
  const uint8_t* grid;  // EditArgs::grid (brick-major)
  uint16_t* field;      // kLattice * 64 steps values, brick-major like the grid: leaf_code(bx, by, bz) * 64 + bit
  uint32_t medium;      // DUST_HIP_FLOOD_*
  uint32_t byte;        // MATERIAL: the grid byte (palette index + 1) that is passable
  uint32_t max_steps;
  uint32_t lo[3], hi[3];  // the inclusive region, clipped to the tree and not empty
  // one pass: the bricks to relax and where the bricks it wakes go
  const uint32_t* list;
  const uint32_t* count;
  uint32_t* flag;         // of `list`: a brick clears its own
  uint32_t* next_list;
  uint32_t* next_count;
  uint32_t* next_flag;
  uint32_t* zero_count;   // the count the pass after next appends to
  uint32_t first;         // the pass that follows the seeding: a seed on a brick face wakes the neighbour although its value did not drop
  const uint32_t* seeds;  // xyz triples (k_flood_seed)
  uint32_t n_seeds;
  uint32_t* acc;          // kFloodAccWords, zeroed by the caller
};

// memset + seeds: afterwards list 0 names the seeded bricks (the scratch's flags and counts zeroed by the caller)
hipError_t launch_flood_seed(const FloodArgs& a, hipStream_t s);
// one relaxation pass over a.list with `workgroups` workgroups (any number >= 1 is correct: the list is walked with a stride)
hipError_t launch_flood_relax(const FloodArgs& a, uint32_t workgroups, hipStream_t s);
hipError_t launch_flood_result(const FloodArgs& a, hipStream_t s);
hipError_t launch_flood_paths(const uint16_t* field, const uint32_t* starts, uint32_t n, uint32_t capacity, uint32_t* keys, uint32_t* lengths, hipStream_t s);

}  // namespace dust
