// fracture_rule.hpp -- the device-free half of the model fracture (dust_hip_model_fracture): the scaled squared distance from a voxel
// to a seed, its exact minimum and maximum over an inclusive voxel box, the order that picks a voxel's seed, and the predicate that
// prunes the seeds of a box. Integers only: a coordinate difference stays below 2^11 in magnitude (voxels 0..255, seeds -1024..1279),
// its square below 2^21, a scale is at most 16, so d2 stays below 3 * 16 * 1279^2 < 2^27 and nothing here can overflow 32 bits. No
// HIP call, no memory access. fracture.hip calls it per lane; tests/cpp/fracture_rule_test.cpp runs the same text on a CPU
// (tests/test_fracture_rule.py).
//
// Pruning. For a box B and the seed set S let U = min over s' in S of max_d2(s', B). A seed s is a candidate for B when
// min_d2(s, B) <= U (and min_d2(s, B) <= max_distance2 where a limit is set). The winner w of any voxel v in B -- the seed that
// minimises (d2(v, s), index) -- is a candidate, tie winner included:
//   with s' the seed that attains U, d2(v, w) <= d2(v, s') <= max_d2(s', B) = U, and min_d2(w, B) <= d2(v, w): so min_d2(w, B) <= U;
//   where v is labelled under a limit, d2(v, w) <= max_distance2, so min_d2(w, B) <= max_distance2 as well. (Where v is not, no
//   candidate is nearer than w, so the winner among the candidates is beyond the limit too and v stays unlabelled.)
// The comparison is <=, never <: with < a seed whose nearest point of the box is exactly U away -- the tie winner of that point when its
// index is the lower one -- would be dropped. The minimum of (d2, index) over the candidates does not depend on their order.
#pragma once
#include <cstdint>

#include "surface_rule.hpp"

#define DUST_FRACTURE_FN DUST_SURFACE_FN

namespace dust {

constexpr uint32_t kFractureMaxSeeds = 4096;        // DUST_HIP_MAX_FRACTURE_SEEDS
constexpr uint32_t kFractureNoCell = 0xFFFFu;       // DUST_HIP_NO_CELL (field.hpp's kFieldNone)
constexpr uint32_t kFractureNoLimit = 0xFFFFFFFFu;  // DUST_HIP_FRACTURE_NO_LIMIT
constexpr int32_t kFractureSeedMin = -1024, kFractureSeedMax = 1279;
constexpr uint32_t kFractureMaxScale = 16;

struct FractureBox {
  int32_t lo[3], hi[3];  // inclusive, lo <= hi, inside the tree
};

// a * b for |a|, |b| < 2^23 with a product that fits 32 bits: the 24-bit multiply on the device (differences fit 12 bits, their squares
// 22, a scale 5), the plain one on a host -- the same value
DUST_FRACTURE_FN uint32_t fracture_mul(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__umul24(a, b);
#else
  return a * b;
#endif
}
// scale * d * d for a difference d
DUST_FRACTURE_FN uint32_t fracture_term(uint32_t scale, int32_t d) {
  const uint32_t a = (uint32_t)(d < 0 ? -d : d);
  return fracture_mul(fracture_mul(a, a), scale);
}
DUST_FRACTURE_FN uint32_t fracture_d2(const uint32_t scale[3], int32_t dx, int32_t dy, int32_t dz) {
  return fracture_term(scale[0], dx) + fracture_term(scale[1], dy) + fracture_term(scale[2], dz);
}
// the smallest / largest |c - s| over lo <= c <= hi: the per-axis clamps
DUST_FRACTURE_FN int32_t fracture_axis_min(int32_t s, int32_t lo, int32_t hi) { return s < lo ? lo - s : (s > hi ? s - hi : 0); }
DUST_FRACTURE_FN int32_t fracture_axis_max(int32_t s, int32_t lo, int32_t hi) {
  const int32_t a = s - lo, b = hi - s;  // (one of them may be negative: then the other is the larger magnitude)
  const int32_t ua = a < 0 ? -a : a, ub = b < 0 ? -b : b;
  return ua > ub ? ua : ub;
}
// the exact minimum / maximum of d2(v, seed) over the voxels v of the box
DUST_FRACTURE_FN uint32_t fracture_min_d2(const uint32_t scale[3], int32_t sx, int32_t sy, int32_t sz, const FractureBox& b) {
  return fracture_d2(scale, fracture_axis_min(sx, b.lo[0], b.hi[0]), fracture_axis_min(sy, b.lo[1], b.hi[1]), fracture_axis_min(sz, b.lo[2], b.hi[2]));
}
DUST_FRACTURE_FN uint32_t fracture_max_d2(const uint32_t scale[3], int32_t sx, int32_t sy, int32_t sz, const FractureBox& b) {
  return fracture_d2(scale, fracture_axis_max(sx, b.lo[0], b.hi[0]), fracture_axis_max(sy, b.lo[1], b.hi[1]), fracture_axis_max(sz, b.lo[2], b.hi[2]));
}
// the order on (d2, index): seed a is taken before seed b
DUST_FRACTURE_FN bool fracture_before(uint32_t d2_a, uint32_t index_a, uint32_t d2_b, uint32_t index_b) {
  return d2_a < d2_b || (d2_a == d2_b && index_a < index_b);
}
// the pruning predicate (see above); u = the smallest max_d2 of any seed to the box, limit = max_distance2 (kFractureNoLimit: none)
DUST_FRACTURE_FN bool fracture_candidate(uint32_t min_d2, uint32_t u, uint32_t limit) {
  return min_d2 <= u && (limit == kFractureNoLimit || min_d2 <= limit);
}
// what a counted voxel whose winner is `index` at `d2` holds (index kFractureNoCell: there was no candidate)
DUST_FRACTURE_FN uint32_t fracture_label(uint32_t d2, uint32_t index, uint32_t limit) {
  return (index != kFractureNoCell && (limit == kFractureNoLimit || d2 <= limit)) ? index : kFractureNoCell;
}

}  // namespace dust
