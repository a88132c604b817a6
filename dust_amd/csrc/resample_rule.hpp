// resample_rule.hpp -- the device-free half of the model resample (dust_hip_model_resample): the fixed-point affine map from a
// destination voxel to a source voxel, the floor that ends it, the test against the source sub-box, and the exact range of the map over
// an inclusive destination box -- what decides whether a root cell can hold a voxel of the image.
// Integers only, 32 bits: with |m[k][r]| <= 8 * 65536 = 2^19, |t[k]| <= 2^28 and destination coordinates 0..255 a term m * (2 c + 1)
// stays below 2^19 * 511 < 2^28, and every partial sum of Q[k] = m[k][0] (2x+1) + m[k][1] (2y+1) + m[k][2] (2z+1) + 2 t[k] below
// 3 * 2^19 * 511 + 2^29 = 1 340 604 416 < 2^31. No HIP call, no memory access. resample.hip calls it per lane,
// model_records.hpp per root cell; tests/cpp/resample_rule_test.cpp runs the same text on a CPU (tests/test_resample_rule.py).
//
// The range. Q[k] is affine and separable: one term per destination axis, each monotone in its coordinate. Over a box its minimum
// (maximum) is the sum of the per-axis minima (maxima), each taken at one end of the axis' interval -- exact, not a bound. floor is
// monotone, so s[k] = floor(Q[k] / 131072) over the box lies in [floor(min), floor(max)] and attains both ends. A box whose interval
// misses [src_lo[k], src_hi[k]] on some axis k holds no voxel of the image. (The converse does not hold: the three axes attain their
// ranges at different voxels, and between the ends s[k] may step over a thin sub-box. The test culls; the per-voxel test decides.)
#pragma once
#include <cstdint>

#include "surface_rule.hpp"

#define DUST_RESAMPLE_FN DUST_SURFACE_FN

namespace dust {

constexpr int32_t kResampleOne = 65536;             // DUST_HIP_RESAMPLE_ONE: 1.0 in the matrix and the translation
constexpr int32_t kResampleMaxM = 8 * 65536;        // |m[k][r]| at most
constexpr int32_t kResampleMaxT = 1 << 28;          // |t[k]| at most
constexpr uint32_t kResampleMaxRecords = 65536;     // DUST_HIP_MAX_RESAMPLES
constexpr int32_t kResampleShift = 17;              // Q is in units of 1 / 131072 voxel: the doubled coordinates 2 c + 1

static_assert((-1 >> 1) == -1, "the floor is an arithmetic shift");

// the inverse map as the rule reads it: the caller's matrix, and twice its translation
struct ResampleMap {
  int32_t m[3][3];
  int32_t t2[3];
};
struct ResampleRange {
  int32_t lo, hi;
};

// the term of destination coordinate c (0..255) on one axis: m * (2 c + 1), the voxel's centre in half voxels
DUST_RESAMPLE_FN int32_t resample_term(int32_t m, int32_t c) { return m * (2 * c + 1); }
// floor(q / 131072), toward minus infinity: -1 -> -1
DUST_RESAMPLE_FN int32_t resample_floor(int32_t q) { return q >> kResampleShift; }
// Q[k] of destination voxel (x, y, z)
DUST_RESAMPLE_FN int32_t resample_q(const ResampleMap& r, int k, int32_t x, int32_t y, int32_t z) {
  return resample_term(r.m[k][0], x) + resample_term(r.m[k][1], y) + resample_term(r.m[k][2], z) + r.t2[k];
}
// whether source coordinate s lies in the inclusive lo..hi (0 <= lo <= hi <= 255; s may be negative)
DUST_RESAMPLE_FN bool resample_inside(int32_t s, int32_t lo, int32_t hi) { return (uint32_t)(s - lo) <= (uint32_t)(hi - lo); }

// the exact [min, max] of one axis' term over the inclusive coordinates lo..hi: the term is monotone, its ends are the interval's
DUST_RESAMPLE_FN ResampleRange resample_axis_range(int32_t m, int32_t lo, int32_t hi) {
  const int32_t a = resample_term(m, lo), b = resample_term(m, hi);
  return {a < b ? a : b, a < b ? b : a};
}
// the exact [min, max] of Q[k] over the inclusive destination box lo..hi (lo <= hi, inside the tree), k = 0, 1, 2
DUST_RESAMPLE_FN void resample_box_range(const ResampleMap& r, const int32_t lo[3], const int32_t hi[3], ResampleRange out[3]) {
  for (int k = 0; k < 3; ++k) {
    int32_t least = r.t2[k], most = r.t2[k];
    for (int a = 0; a < 3; ++a) {
      const ResampleRange t = resample_axis_range(r.m[k][a], lo[a], hi[a]);
      least += t.lo; most += t.hi;
    }
    out[k] = {least, most};
  }
}
// whether the source interval of a range of Q[k] meets the sub-box's lo..hi on that axis
DUST_RESAMPLE_FN bool resample_range_meets(int32_t q_lo, int32_t q_hi, int32_t src_lo, int32_t src_hi) {
  return resample_floor(q_hi) >= src_lo && resample_floor(q_lo) <= src_hi;
}
// the interval test: false -> no voxel of the destination box lo..hi reads a source voxel inside src_lo..src_hi
DUST_RESAMPLE_FN bool resample_box_meets(const ResampleMap& r, const int32_t lo[3], const int32_t hi[3], const int32_t src_lo[3], const int32_t src_hi[3]) {
  ResampleRange q[3];
  resample_box_range(r, lo, hi, q);
  return resample_range_meets(q[0].lo, q[0].hi, src_lo[0], src_hi[0]) && resample_range_meets(q[1].lo, q[1].hi, src_lo[1], src_hi[1]) &&
         resample_range_meets(q[2].lo, q[2].hi, src_lo[2], src_hi[2]);
}

}  // namespace dust
