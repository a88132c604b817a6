// settle_rule.hpp -- the device-free half of the model settling (dust_hip_model_settle, _settle_apply): where the loose voxels of one
// voxel column come to rest, and which loose voxels of a 4^3 brick slide one step sideways and down. A column is column_rule.hpp's
// Column, turned so that position 0 is the end things fall toward; `loose` and `fixed` are disjoint. A brick word is surface_rule.hpp's
// (bit x<<4 | y<<2 | z). Everything is shifts, popcounts and counts of zeros over values: no HIP call, no memory access, no array
// indexed by a runtime value (every loop over the four words, and every index into the 3 x 3 bricks, is constant). settle.hip calls it
// per lane (columns) and per wave (bricks, all scalar work); tests/cpp/settle_rule_test.cpp runs the same text on a CPU
// (tests/test_settle_rule.py).
#pragma once
#include <cstdint>

#include "column_rule.hpp"

#define DUST_SETTLE_FN DUST_SURFACE_FN

namespace dust {

// ------------------------------------------------------------------ the fall of one column
DUST_SETTLE_FN Column column_or(const Column& a, const Column& b) { return {{a.w[0] | b.w[0], a.w[1] | b.w[1], a.w[2] | b.w[2], a.w[3] | b.w[3]}}; }
DUST_SETTLE_FN Column column_and(const Column& a, const Column& b) { return {{a.w[0] & b.w[0], a.w[1] & b.w[1], a.w[2] & b.w[2], a.w[3] & b.w[3]}}; }
DUST_SETTLE_FN Column column_xor(const Column& a, const Column& b) { return {{a.w[0] ^ b.w[0], a.w[1] ^ b.w[1], a.w[2] ^ b.w[2], a.w[3] ^ b.w[3]}}; }
// positions a .. b - 1 (a <= b <= 256)
DUST_SETTLE_FN Column column_range(uint32_t a, uint32_t b) {
  Column r;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t base = 64u * k;
    const uint32_t lo = a > base ? a - base : 0u, hi = b > base ? b - base : 0u;  // the part of the range in this word: lo .. hi - 1, cut at 64
    const uint64_t below_hi = hi >= 64u ? ~0ull : ((1ull << hi) - 1ull);
    const uint64_t below_lo = lo >= 64u ? ~0ull : ((1ull << lo) - 1ull);
    r.w[k] = below_hi & ~below_lo;
  }
  return r;
}
// the lowest set position, kColumnBits when there is none
DUST_SETTLE_FN uint32_t column_first(const Column& c) {
  uint32_t p = kColumnBits;
#pragma unroll
  for (uint32_t i = 0; i < 4u; ++i) {
    const uint32_t k = 3u - i;
    if (c.w[k] != 0ull) p = 64u * k + column_ctz(c.w[k]);
  }
  return p;
}
// the highest set position, kColumnBits when there is none
DUST_SETTLE_FN uint32_t column_last(const Column& c) {
  uint32_t p = kColumnBits;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k)
    if (c.w[k] != 0ull) p = 64u * k + 63u - column_clz(c.w[k]);
  return p;
}
// the sum of the set positions: per word, bit k of a position counts 2^k times for every set bit whose position has it
DUST_SETTLE_FN uint32_t column_position_sum(const Column& c) {
  constexpr uint64_t kBit[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                                0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    sum += 64u * k * column_popcount(c.w[k]);
#pragma unroll
    for (uint32_t b = 0; b < 6u; ++b) sum += column_popcount(c.w[k] & kBit[b]) << b;
  }
  return sum;
}

// The floor of position i (< 256): one past the highest fixed position below i, 0 when there is none
DUST_SETTLE_FN uint32_t settle_floor(const Column& fixed, uint32_t i) { return i - column_zeros_below(fixed, i); }
// Where the loose voxel at position i comes to rest: its floor plus the loose voxels between the floor and it
DUST_SETTLE_FN uint32_t settle_destination(const Column& loose, const Column& fixed, uint32_t i) {
  const uint32_t f = settle_floor(fixed, i);
  return f + column_count(column_and(loose, column_range(f, i)));
}

// One fall of a column. now: the loose occupancy afterwards (the fixed voxels stay). loose, fixed: the counts. moved: the loose voxels
// whose position changes. fall_sum and fall_max over the loose voxels' falls (position before - position after).
struct SettleFall {
  Column now;
  uint32_t loose, fixed, moved, fall_sum, fall_max;
};
// A segment is the stretch between two fixed voxels (or an end of the column). Its n loose voxels end as positions f .. f + n - 1: a
// popcount per segment. Within a segment the falls never decrease with the position, so the longest is the top voxel's and the voxels
// that stay are the run of loose voxels standing on the floor.
DUST_SETTLE_FN SettleFall settle_fall(const Column& loose, const Column& fixed) {
  SettleFall r{};
  r.loose = column_count(loose);
  r.fixed = column_count(fixed);
  if (r.loose != 0u) {
    uint32_t f = 0;  // the floor of the segment at hand
    for (;;) {
      const uint32_t e = column_first(column_and(fixed, column_range(f, kColumnBits)));  // the fixed voxel that ends it, or 256
      const Column in = column_and(loose, column_range(f, e));
      const uint32_t n = column_count(in);
      if (n != 0u) {
        r.now = column_or(r.now, column_range(f, f + n));
        const uint32_t fall = column_last(in) - (f + n - 1u);
        r.fall_max = fall > r.fall_max ? fall : r.fall_max;
        r.moved += n - column_ones_from(in, f);
      }
      if (e >= kColumnBits) break;
      f = e + column_ones_from(fixed, e);  // past the fixed run
      if (f >= kColumnBits) break;
    }
    r.fall_sum = column_position_sum(loose) - column_position_sum(r.now);
  }
  return r;
}

// The same fall as a walk in ascending order, for the code that moves bytes: move(from, to) for every loose voxel whose position
// changes. `to` < `from`, and `to` is never above a position not yet visited: the moves can be made in place, in this order.
template <class Move>
DUST_SETTLE_FN void settle_walk(const Column& loose, const Column& fixed, Move&& move) {
  uint32_t next = 0;  // where the next loose voxel comes to rest
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    uint64_t word = loose.w[k] | fixed.w[k];
    while (word != 0ull) {
      const uint32_t b = column_ctz(word), p = 64u * k + b;
      word &= word - 1ull;
      if ((fixed.w[k] >> b) & 1ull) {
        next = p + 1u;
      } else {
        if (next != p) move(p, next);
        ++next;
      }
    }
  }
}

// ------------------------------------------------------------------ the slide of one brick
// An axis of a brick word: the plane c == 0 and the bits a step along it moves
struct SettleAxis {
  uint64_t plane0;
  uint32_t shift;
};
DUST_SETTLE_FN SettleAxis settle_axis(uint32_t axis) {
  SettleAxis a;
  a.plane0 = axis == 0u ? kSurfaceX0 : (axis == 1u ? kSurfaceY0 : kSurfaceZ0);
  a.shift = 16u >> (2u * axis);
  return a;
}
// What every voxel v of a brick sees K (1 or 2) voxels away along an axis, towards the high end (`up`) or the low end: `own` moved
// by K voxels, with the K facing planes of `side`, the brick on that side, moved in. neighbour_rule.hpp's step for a runtime axis.
template <uint32_t K>
DUST_SETTLE_FN uint64_t settle_look(uint64_t own, uint64_t side, const SettleAxis& a, bool up) {
  if (K == 0u) return own;
  const uint64_t low = K == 1u ? a.plane0 : (a.plane0 | (a.plane0 << a.shift));  // planes c < K
  const uint64_t high = low << ((4u - K) * a.shift);                              // planes c >= 4 - K
  if (up) return ((own >> (K * a.shift)) & ~high) | ((side << ((4u - K) * a.shift)) & high);
  return ((own << (K * a.shift)) & ~low) | ((side >> ((4u - K) * a.shift)) & low);
}

// The bricks a slide looks at: w[1 + i][1 + j] is the brick i bricks along the slide's lateral direction d and j bricks along the fall
// direction g (w[1][1] the brick itself). A brick off the tree: occ 0, region 0.
struct SettleBricks {
  uint64_t occ[3][3];     // solid voxels
  uint64_t loose[3][3];   // the loose ones among them
  uint64_t region[3][3];  // surface_region_mask: the voxels of the brick inside the region
};
// the direction of a slide and of the fall as the words see them
struct SettleDirs {
  SettleAxis d, g;
  bool d_up, g_up;  // the direction points to the high end of its axis
};
// what voxel v sees at v + A d + B g of a field given per brick (A in -1..1, B in -2..1)
template <int A, int B>
DUST_SETTLE_FN uint64_t settle_field(const uint64_t (&f)[3][3], const SettleDirs& s) {
  constexpr int sa = A < 0 ? -1 : (A > 0 ? 1 : 0), sb = B < 0 ? -1 : (B > 0 ? 1 : 0);
  constexpr uint32_t ka = A < 0 ? -A : A, kb = B < 0 ? -B : B;
  const uint64_t own = settle_look<kb>(f[1][1], f[1][1 + sb], s.g, (B > 0) == s.g_up);
  const uint64_t side = sa == 0 ? 0ull : settle_look<kb>(f[1 + sa][1], f[1 + sa][1 + sb], s.g, (B > 0) == s.g_up);
  return settle_look<ka>(own, side, s.d, (A > 0) == s.d_up);
}
// A loose voxel p of the region slides to p + d + g when the voxel above it (p - g) is empty or outside the region and p + d and
// p + d + g are inside the region and empty. leave: the voxels of the brick that slide away; arrive: the voxels of the brick a voxel
// slides into (from v - d - g). Both are decided on the bricks as they stand.
struct SettleSlide {
  uint64_t leave, arrive;
};
DUST_SETTLE_FN SettleSlide settle_slide(const SettleBricks& n, const SettleDirs& s) {
  uint64_t solid[3][3], blocked[3][3], loose[3][3];  // solid: of the region; blocked: solid or outside it
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      solid[i][j] = n.occ[i][j] & n.region[i][j];
      blocked[i][j] = n.occ[i][j] | ~n.region[i][j];
      loose[i][j] = n.loose[i][j] & n.region[i][j];
    }
  }
  SettleSlide r;
  r.leave = loose[1][1] & ~settle_field<0, -1>(solid, s) & ~settle_field<1, 0>(blocked, s) & ~settle_field<1, 1>(blocked, s);
  r.arrive = settle_field<-1, -1>(loose, s) & ~settle_field<-1, -2>(solid, s) & ~settle_field<0, -1>(blocked, s) & ~blocked[1][1];
  return r;
}

}  // namespace dust
