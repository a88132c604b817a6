// A cave pass through the C++ mirror (include/dust_hip.hpp): ask what one generation of the 4-5 rule would do to a random fill, run
// eight generations of it, then take the specks off and close the pinholes, and let moss spread one ring in the material most
// neighbours carry. Compiled (not run) by tests/test_neighbour_abi.py.
#include "dust_hip.hpp"

struct Cave { uint32_t asked; uint64_t changed; uint32_t generations; uint32_t lonely; };

Cave dig_cave(dust::VoxGeometry& block, uint8_t stone) {
  DustHipNeighboursQuery rule{};
  rule.neighbourhood = DUST_HIP_NEIGHBOURS_CORNERS;
  rule.palette = stone;
  for (int r = 0; r < 3; ++r) rule.hi[r] = 255;
  for (uint32_t n = 14; n <= 26; ++n) rule.birth |= 1u << n;             // born with 14 or more solid neighbours
  for (uint32_t n = 13; n <= 26; ++n) rule.survive |= 1u << n;           // ... and kept with 13 or more
  std::vector<uint32_t> counts, rows;
  const DustHipNeighboursResult ask = block.neighbours(rule, &counts);   // ask first
  Cave c{};
  c.asked = ask.born + ask.died;
  c.lonely = counts[DUST_HIP_NEIGHBOURS_BINS + 0];                       // solid voxels without a solid neighbour
  const DustHipNeighboursApplied dug = block.neighbours_apply(rule, 8, &rows);   // apply after
  c.changed = dug.born + dug.died;
  c.generations = dug.generations;
  DustHipNeighboursQuery tidy = rule;
  tidy.neighbourhood = DUST_HIP_NEIGHBOURS_FACES;
  tidy.birth = (1u << 5) | (1u << 6);                                    // pinholes enclosed on 5 or 6 sides close
  tidy.survive = 0x7Fu & ~1u;                                            // specks without a face neighbour go
  tidy.flags = DUST_HIP_NEIGHBOURS_MAJORITY;
  c.changed += block.neighbours_apply(tidy).born;
  static_assert(sizeof(DustHipNeighboursQuery) == 48 && sizeof(DustHipNeighboursResult) == 64 && sizeof(DustHipNeighboursApplied) == 64 &&
                    DUST_HIP_NEIGHBOURS_BINS == 27u && DUST_HIP_NEIGHBOURS_WALLS == DUST_HIP_SURFACE_WALLS,
                "neighbours records");
  return c;
}
