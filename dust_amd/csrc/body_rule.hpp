// body_rule.hpp -- the device-free half of the model bodies (dust_hip_model_bodies): the ONE text of the arithmetic that turns the voxels
// of a 4^3 brick into mass, first and second moments. Bit x<<4 | y<<2 | z of a word is voxel (x, y, z) of the brick (grid.hpp voxel_bit).
// Integer work over values: no HIP call, no memory access, no array indexed by a runtime value. body.hip calls it per (brick, group),
// where every word is wave-uniform (scalar work); tests/cpp/body_rule_test.cpp runs the same text on a CPU (tests/test_body_rule.py).
//
// A brick's LOCAL moments are taken over lx, ly, lz in 0..3 and stay in 32 bits: each is at most 64 voxels x 65535 x 9 < 2^26.
// body_shift moves them to the brick's origin (X0, Y0, Z0) in 64 bits:
//   sum w x    = X0 W + sum w lx
//   sum w x^2  = X0^2 W + 2 X0 sum w lx + sum w lx^2
//   sum w x y  = X0 Y0 W + X0 sum w ly + Y0 sum w lx + sum w lx ly
// Overflow bound: a sum over the whole tree is at most 65535 * 255^2 * 2^24 < 2^56, below 2^63.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define DUST_BODY_FN __host__ __device__ __forceinline__
#else
#define DUST_BODY_FN inline
#endif

namespace dust {

constexpr uint32_t kBodySums = 10;  // mass; w x, w y, w z; w xx, w yy, w zz, w xy, w yz, w zx
constexpr uint32_t kBodyW = 0, kBodyX = 1, kBodyY = 2, kBodyZ = 3, kBodyXX = 4, kBodyYY = 5, kBodyZZ = 6, kBodyXY = 7, kBodyYZ = 8, kBodyZX = 9;
// the planes of a brick word with c == 0 on an axis, and how far a step along the axis moves a bit (surface_rule.hpp's)
constexpr uint64_t kBodyX0 = 0x000000000000FFFFull, kBodyY0 = 0x000F000F000F000Full, kBodyZ0 = 0x1111111111111111ull;
constexpr uint32_t kBodyShiftX = 16, kBodyShiftY = 4, kBodyShiftZ = 1;

struct BodyLocal {  // a brick's moments about its own origin, in kBody* order
  uint32_t v[kBodySums];
};
struct BodySums {  // the same about the tree's origin
  uint64_t v[kBodySums];
};
// What a set of voxels adds to a record. The neutral element is all zeroes: the lower bounds are kept as 255 - lo, so that a zeroed
// accumulator is empty and both bounds fold with a maximum.
struct BodyPart {
  uint32_t voxels;
  uint32_t inv_lo[3], hi[3];
  BodySums s;
};
struct BodyRecord {  // DustHipBody, 96 bytes
  uint32_t key, voxels;
  uint8_t lo[3], reserved0, hi[3], reserved1;
  uint64_t mass, m1[3], m2[6];
};
static_assert(sizeof(BodyRecord) == 96, "DustHipBody");

DUST_BODY_FN uint32_t body_popcount(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// The weighted path: what voxel `bit` of weight w adds to its brick's local moments. The caller sums the ten values over the voxels.
DUST_BODY_FN BodyLocal body_local_voxel(uint32_t w, uint32_t bit) {
  const uint32_t lx = bit >> 4, ly = (bit >> 2) & 3u, lz = bit & 3u;
  BodyLocal l;
  l.v[kBodyW] = w;
  l.v[kBodyX] = w * lx; l.v[kBodyY] = w * ly; l.v[kBodyZ] = w * lz;
  l.v[kBodyXX] = w * lx * lx; l.v[kBodyYY] = w * ly * ly; l.v[kBodyZZ] = w * lz * lz;
  l.v[kBodyXY] = w * lx * ly; l.v[kBodyYZ] = w * ly * lz; l.v[kBodyZX] = w * lz * lx;
  return l;
}

// The unweighted fast path: every local moment of the voxels of m, each weighing 1, as popcounts over the planes of m (first and pure
// second moments) and over its columns, the crossings of two planes (mixed moments). No sum across voxels is needed.
DUST_BODY_FN void body_axis_counts(uint64_t m, uint64_t plane0, uint32_t shift, uint32_t& first, uint32_t& second) {
  const uint32_t c1 = body_popcount(m & (plane0 << shift)), c2 = body_popcount(m & (plane0 << (2u * shift))), c3 = body_popcount(m & (plane0 << (3u * shift)));
  first = c1 + 2u * c2 + 3u * c3;
  second = c1 + 4u * c2 + 9u * c3;
}
DUST_BODY_FN uint32_t body_mixed_count(uint64_t m, uint64_t a0, uint32_t a_shift, uint64_t b0, uint32_t b_shift) {
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t a = 1; a < 4u; ++a) {
    const uint64_t ma = m & (a0 << (a_shift * a));
#pragma unroll
    for (uint32_t b = 1; b < 4u; ++b) sum += a * b * body_popcount(ma & (b0 << (b_shift * b)));
  }
  return sum;
}
DUST_BODY_FN BodyLocal body_local_unweighted(uint64_t m) {
  BodyLocal l;
  l.v[kBodyW] = body_popcount(m);
  body_axis_counts(m, kBodyX0, kBodyShiftX, l.v[kBodyX], l.v[kBodyXX]);
  body_axis_counts(m, kBodyY0, kBodyShiftY, l.v[kBodyY], l.v[kBodyYY]);
  body_axis_counts(m, kBodyZ0, kBodyShiftZ, l.v[kBodyZ], l.v[kBodyZZ]);
  l.v[kBodyXY] = body_mixed_count(m, kBodyX0, kBodyShiftX, kBodyY0, kBodyShiftY);
  l.v[kBodyYZ] = body_mixed_count(m, kBodyY0, kBodyShiftY, kBodyZ0, kBodyShiftZ);
  l.v[kBodyZX] = body_mixed_count(m, kBodyZ0, kBodyShiftZ, kBodyX0, kBodyShiftX);
  return l;
}

// local moments of the brick whose lowest voxel is (x0, y0, z0) -> moments about the tree's origin
DUST_BODY_FN BodySums body_shift(const BodyLocal& l, uint32_t x0, uint32_t y0, uint32_t z0) {
  const uint64_t X = x0, Y = y0, Z = z0, W = l.v[kBodyW];
  const uint64_t lx = l.v[kBodyX], ly = l.v[kBodyY], lz = l.v[kBodyZ];
  BodySums s;
  s.v[kBodyW] = W;
  s.v[kBodyX] = X * W + lx; s.v[kBodyY] = Y * W + ly; s.v[kBodyZ] = Z * W + lz;
  s.v[kBodyXX] = X * X * W + 2u * X * lx + l.v[kBodyXX];
  s.v[kBodyYY] = Y * Y * W + 2u * Y * ly + l.v[kBodyYY];
  s.v[kBodyZZ] = Z * Z * W + 2u * Z * lz + l.v[kBodyZZ];
  s.v[kBodyXY] = X * Y * W + X * ly + Y * lx + l.v[kBodyXY];
  s.v[kBodyYZ] = Y * Z * W + Y * lz + Z * ly + l.v[kBodyYZ];
  s.v[kBodyZX] = Z * X * W + Z * lx + X * lz + l.v[kBodyZX];
  return s;
}

// 255 - the lowest and the highest of a brick's four coordinates on an axis that m (not 0) touches
DUST_BODY_FN void body_axis_bounds(uint64_t m, uint64_t plane0, uint32_t shift, uint32_t base, uint32_t& inv_lo, uint32_t& hi) {
  const bool c0 = (m & plane0) != 0ull, c1 = (m & (plane0 << shift)) != 0ull, c2 = (m & (plane0 << (2u * shift))) != 0ull, c3 = (m & (plane0 << (3u * shift))) != 0ull;
  inv_lo = 255u - (base + (c0 ? 0u : (c1 ? 1u : (c2 ? 2u : 3u))));
  hi = base + (c3 ? 3u : (c2 ? 2u : (c1 ? 1u : 0u)));
}

DUST_BODY_FN BodyPart body_neutral() {
  BodyPart p;
  p.voxels = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) p.inv_lo[r] = p.hi[r] = 0;
#pragma unroll
  for (uint32_t k = 0; k < kBodySums; ++k) p.s.v[k] = 0;
  return p;
}
// the voxels m (not 0) of brick (bx, by, bz) with local moments l: a voxel of weight 0 still counts in `voxels` and the bounds
DUST_BODY_FN BodyPart body_brick_part(uint64_t m, const BodyLocal& l, uint32_t bx, uint32_t by, uint32_t bz) {
  BodyPart p;
  p.voxels = body_popcount(m);
  body_axis_bounds(m, kBodyX0, kBodyShiftX, bx * 4u, p.inv_lo[0], p.hi[0]);
  body_axis_bounds(m, kBodyY0, kBodyShiftY, by * 4u, p.inv_lo[1], p.hi[1]);
  body_axis_bounds(m, kBodyZ0, kBodyShiftZ, bz * 4u, p.inv_lo[2], p.hi[2]);
  p.s = body_shift(l, bx * 4u, by * 4u, bz * 4u);
  return p;
}
DUST_BODY_FN void body_fold(BodyPart& into, const BodyPart& p) {
  into.voxels += p.voxels;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    into.inv_lo[r] = into.inv_lo[r] > p.inv_lo[r] ? into.inv_lo[r] : p.inv_lo[r];
    into.hi[r] = into.hi[r] > p.hi[r] ? into.hi[r] : p.hi[r];
  }
#pragma unroll
  for (uint32_t k = 0; k < kBodySums; ++k) into.s.v[k] += p.s.v[k];
}
// accumulator -> record; a part without a voxel gives the zero record with its key, bounds 255,255,255 / 0,0,0
DUST_BODY_FN BodyRecord body_emit(uint32_t key, const BodyPart& p) {
  BodyRecord r;
  r.key = key;
  r.voxels = p.voxels;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.lo[k] = (uint8_t)(255u - p.inv_lo[k]);
    r.hi[k] = (uint8_t)p.hi[k];
  }
  r.reserved0 = r.reserved1 = 0;
  r.mass = p.s.v[kBodyW];
#pragma unroll
  for (int k = 0; k < 3; ++k) r.m1[k] = p.s.v[kBodyX + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) r.m2[k] = p.s.v[kBodyXX + k];
  return r;
}

}  // namespace dust
