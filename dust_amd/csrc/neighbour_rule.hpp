// neighbour_rule.hpp -- the device-free half of the model neighbourhoods (dust_hip_model_neighbours, _neighbours_apply): how many of a
// voxel's 6, 18 or 26 neighbours are solid, for all 64 voxels of a 4^3 brick at once, as ONE function of 27 64-bit words -- the brick's
// occupancy and its 26 neighbour bricks' -- and what a birth / survive pair of masks over that number makes of the brick. Bit
// x<<4 | y<<2 | z of a word is voxel (x, y, z) of the brick (grid.hpp voxel_bit; EditArgs::brick_mask), as in surface_rule.hpp, whose
// planes and region mask are used here. Integer work over values: no HIP call, no memory access, no array indexed by a runtime value
// (every index below is a template argument or the counter of a loop of constant length). neighbour.hip calls it per brick, where every
// word is wave-uniform (scalar work); tests/cpp/neighbour_rule_test.cpp runs the same text on a CPU (tests/test_neighbour_rule.py).
#pragma once
#include <cstdint>

#include "surface_rule.hpp"

#define DUST_NEIGHBOUR_FN DUST_SURFACE_FN

namespace dust {

constexpr uint32_t kNeighbourFaces = 6, kNeighbourEdges = 18, kNeighbourCorners = 26;  // DUST_HIP_NEIGHBOURS_*: the neighbourhood IS its size
constexpr uint32_t kNeighbourBins = 27;        // a count is 0..26
constexpr uint32_t kNeighbourCountPlanes = 5;  // ... in five bits

// a brick's word and its 26 neighbour bricks': w[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)] is the brick at offset (dx, dy, dz), w[13] the
// brick itself (a neighbour off the tree: 0, or all ones when the outside of the tree counts as solid)
struct NeighbourBricks {
  uint64_t w[27];
};
constexpr uint32_t kNeighbourOwn = 13;
// the number of solid neighbours of every voxel of a brick as bit planes: bit v of b[k] is bit k of voxel v's count
struct NeighbourCount {
  uint64_t b[kNeighbourCountPlanes];
};

// The occupancy of every voxel's neighbour one step along one axis: D < 0, `own` moved by one voxel towards the high end (`shift` bits up,
// so that bit v holds what voxel v - 1 held) with the facing plane of `side`, the brick on the low side, moved in on the plane c == 0;
// D > 0 the mirror image with the brick on the high side; D == 0 the word itself. surface_rule.hpp's N_d, one axis at a time.
template <int D>
DUST_NEIGHBOUR_FN uint64_t neighbour_step(uint64_t own, uint64_t side, uint64_t plane0, uint64_t plane3, uint32_t shift) {
  if (D < 0) return ((own << shift) & ~plane0) | ((side >> (3u * shift)) & plane0);
  if (D > 0) return ((own >> shift) & ~plane3) | ((side << (3u * shift)) & plane3);
  return own;
}
// The occupancy of every voxel's neighbour across the offset (DX, DY, DZ): the composition of the z, the y and the x step, each with the
// planes carried in from the bricks beside it -- so a diagonal neighbour across an edge or a corner of the brick comes from the brick
// across that edge or corner. Only the up to eight bricks the offset can reach are looked at.
template <int DX, int DY, int DZ>
DUST_NEIGHBOUR_FN uint64_t neighbour_plane(const NeighbourBricks& n) {
  // brick column (BX, BY) stepped along z: BX is 0 or DX, BY is 0 or DY
#define DUST_NEIGHBOUR_Z(BX, BY) \
  neighbour_step<DZ>(n.w[((BX) + 1) * 9 + ((BY) + 1) * 3 + 1], n.w[((BX) + 1) * 9 + ((BY) + 1) * 3 + 1 + DZ], kSurfaceZ0, kSurfaceZ3, 1u)
  const uint64_t y_own = neighbour_step<DY>(DUST_NEIGHBOUR_Z(0, 0), DUST_NEIGHBOUR_Z(0, DY), kSurfaceY0, kSurfaceY3, 4u);
  const uint64_t y_side = DX == 0 ? 0ull : neighbour_step<DY>(DUST_NEIGHBOUR_Z(DX, 0), DUST_NEIGHBOUR_Z(DX, DY), kSurfaceY0, kSurfaceY3, 4u);
#undef DUST_NEIGHBOUR_Z
  return neighbour_step<DX>(y_own, y_side, kSurfaceX0, kSurfaceX3, 16u);
}

// count += plane, bit-sliced: a ripple of half adders through the low BITS planes (the caller knows how large the count can be by now)
template <int BITS>
DUST_NEIGHBOUR_FN void neighbour_add(NeighbourCount& c, uint64_t plane) {
#pragma unroll
  for (int k = 0; k < BITS; ++k) {
    const uint64_t carry = c.b[k] & plane;
    c.b[k] ^= plane;
    plane = carry;
  }
}

// The counts of a brick under a neighbourhood (6: the offsets with |d|1 == 1; 18: |d|1 <= 2; 26: the 3^3 box without its centre). FACES
// is the sum of surface_rule.hpp's six N_d; the twelve edge and the eight corner planes come on top.
DUST_NEIGHBOUR_FN NeighbourCount neighbour_count(const NeighbourBricks& n, uint32_t neighbourhood) {
  NeighbourCount c{};
  neighbour_add<1>(c, neighbour_plane<-1, 0, 0>(n)); neighbour_add<2>(c, neighbour_plane<1, 0, 0>(n));
  neighbour_add<2>(c, neighbour_plane<0, -1, 0>(n)); neighbour_add<3>(c, neighbour_plane<0, 1, 0>(n));
  neighbour_add<3>(c, neighbour_plane<0, 0, -1>(n)); neighbour_add<3>(c, neighbour_plane<0, 0, 1>(n));
  if (neighbourhood >= kNeighbourEdges) {  // up to 18: four planes are enough until 16 is reached
    neighbour_add<3>(c, neighbour_plane<-1, -1, 0>(n)); neighbour_add<4>(c, neighbour_plane<-1, 1, 0>(n));
    neighbour_add<4>(c, neighbour_plane<1, -1, 0>(n)); neighbour_add<4>(c, neighbour_plane<1, 1, 0>(n));
    neighbour_add<4>(c, neighbour_plane<-1, 0, -1>(n)); neighbour_add<4>(c, neighbour_plane<-1, 0, 1>(n));
    neighbour_add<4>(c, neighbour_plane<1, 0, -1>(n)); neighbour_add<4>(c, neighbour_plane<1, 0, 1>(n));
    neighbour_add<4>(c, neighbour_plane<0, -1, -1>(n)); neighbour_add<5>(c, neighbour_plane<0, -1, 1>(n));
    neighbour_add<5>(c, neighbour_plane<0, 1, -1>(n)); neighbour_add<5>(c, neighbour_plane<0, 1, 1>(n));
  }
  if (neighbourhood >= kNeighbourCorners) {
    neighbour_add<5>(c, neighbour_plane<-1, -1, -1>(n)); neighbour_add<5>(c, neighbour_plane<-1, -1, 1>(n));
    neighbour_add<5>(c, neighbour_plane<-1, 1, -1>(n)); neighbour_add<5>(c, neighbour_plane<-1, 1, 1>(n));
    neighbour_add<5>(c, neighbour_plane<1, -1, -1>(n)); neighbour_add<5>(c, neighbour_plane<1, -1, 1>(n));
    neighbour_add<5>(c, neighbour_plane<1, 1, -1>(n)); neighbour_add<5>(c, neighbour_plane<1, 1, 1>(n));
  }
  return c;
}

// the voxels whose count is exactly n (n may differ per lane: neighbour.hip's histogram gives every lane a bin of its own)
DUST_NEIGHBOUR_FN uint64_t neighbour_equals(const NeighbourCount& c, uint32_t n) {
  uint64_t m = ~0ull;
#pragma unroll
  for (uint32_t k = 0; k < kNeighbourCountPlanes; ++k) m &= ((n >> k) & 1u) ? c.b[k] : ~c.b[k];
  return m;
}
// the voxels whose count n has bit n of `mask` set
DUST_NEIGHBOUR_FN uint64_t neighbour_match(const NeighbourCount& c, uint32_t mask) {
  uint64_t hit = 0ull;
#pragma unroll
  for (uint32_t n = 0; n < kNeighbourBins; ++n)
    if ((mask >> n) & 1u) hit |= neighbour_equals(c, n);
  return hit;
}

// What one generation makes of a brick: inside `region` (surface_region_mask) an empty voxel with bit n of `birth` set is born, a solid
// voxel with bit n of `survive` clear dies; every other voxel keeps its value.
struct NeighbourChange {
  uint64_t born, died;
};
DUST_NEIGHBOUR_FN NeighbourChange neighbour_change(uint64_t own, const NeighbourCount& c, uint32_t birth, uint32_t survive, uint64_t region) {
  NeighbourChange g;
  g.born = ~own & region & neighbour_match(c, birth);
  g.died = own & region & ~neighbour_match(c, survive);
  return g;
}

}  // namespace dust
