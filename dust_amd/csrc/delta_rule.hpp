// delta_rule.hpp -- the device-free half of the model deltas (dust_hip_model_delta): what the occupancy words of one 4^3 brick in two
// models say about the voxels they differ in. Bit x<<4 | y<<2 | z of a word is voxel (x, y, z) of the brick (grid.hpp voxel_bit;
// EditArgs::brick_mask). Integer work over values: no HIP call, no memory access. delta.hip calls it per brick, where every word is
// wave-uniform (scalar work); tests/cpp/delta_rule_test.cpp runs the same text on a CPU (tests/test_delta_rule.py).
#pragma once
#include <cstdint>

#include "surface_rule.hpp"  // surface_region_mask, DUST_SURFACE_FN

namespace dust {

// the DUST_HIP_DELTA_* kinds
constexpr uint32_t kDeltaAdded = 1, kDeltaRemoved = 2, kDeltaRepainted = 4;

struct DeltaWords {
  uint64_t solid_before, solid_after;  // the brick's solid voxels inside the region, whatever the kinds
  uint64_t added, removed;             // None before and solid after / solid before and None after, where the kind is asked for
  uint64_t candidates;                 // solid in both, where REPAINTED is asked for: only the grid bytes say which of them differ
};

// mA, mB: the brick's word before and after; region: the part of the query's region the brick holds (surface_region_mask)
DUST_SURFACE_FN DeltaWords delta_words(uint64_t mA, uint64_t mB, uint64_t region, uint32_t kinds) {
  DeltaWords w;
  w.solid_before = mA & region;
  w.solid_after = mB & region;
  w.added = (kinds & kDeltaAdded) ? (~mA & mB & region) : 0ull;
  w.removed = (kinds & kDeltaRemoved) ? (mA & ~mB & region) : 0ull;
  w.candidates = (kinds & kDeltaRepainted) ? (mA & mB & region) : 0ull;
  return w;
}

// What is listed of a brick once its grid bytes have spoken. differs: the voxels whose byte before is not the byte after (the ballot of
// a != b; only its bits among the candidates count); filter: the voxels whose byte before or after is the palette filter's (all ones
// without a filter).
struct DeltaListed {
  uint64_t added, removed, repainted, listed;
};
DUST_SURFACE_FN DeltaListed delta_listed(const DeltaWords& w, uint64_t differs, uint64_t filter) {
  DeltaListed l;
  l.added = w.added & filter;
  l.removed = w.removed & filter;
  l.repainted = w.candidates & differs & filter;
  l.listed = l.added | l.removed | l.repainted;
  return l;
}

}  // namespace dust
