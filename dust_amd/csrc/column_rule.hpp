// column_rule.hpp -- the device-free half of the model columns (dust_hip_model_columns, _columns_apply): what the 256 voxels of one
// column along an axis say about its runs. A Column is 256 bits as four 64-bit words, bit 0 of word 0 first; column_turn clips a
// column given in coordinate order to lo..hi and turns it so the near end of the walk is bit 0. Everything after that is shifts,
// popcounts and counts of leading / trailing zeros over values: no HIP call, no memory access, no array indexed by a runtime value
// (every loop over the four words unrolls). column.hip calls it per lane; tests/cpp/column_rule_test.cpp runs the same text on a CPU
// (tests/test_column_rule.py).
#pragma once
#include <cstdint>

#include "surface_rule.hpp"  // DUST_SURFACE_FN

namespace dust {

constexpr uint32_t kColumnBits = 256;  // voxels of a column; also "no such position"
// DUST_HIP_COLUMNS_RUN / _GAP
constexpr uint32_t kColumnsRun = 0, kColumnsGap = 1;

struct Column {
  uint64_t w[4];
};

DUST_SURFACE_FN uint32_t column_popcount(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }
DUST_SURFACE_FN uint32_t column_ctz(uint64_t v) { return v ? (uint32_t)__builtin_ctzll(v) : 64u; }
DUST_SURFACE_FN uint32_t column_clz(uint64_t v) { return v ? (uint32_t)__builtin_clzll(v) : 64u; }
DUST_SURFACE_FN uint64_t column_reverse(uint64_t v) {
  v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
  v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
  v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
  v = ((v >> 8) & 0x00FF00FF00FF00FFull) | ((v & 0x00FF00FF00FF00FFull) << 8);
  v = ((v >> 16) & 0x0000FFFF0000FFFFull) | ((v & 0x0000FFFF0000FFFFull) << 16);
  return (v >> 32) | (v << 32);
}

// the four voxels a brick word holds of one column: those at bit `off` + i * `stride` (i = 0..3; stride 16, 4 or 1 for a column along
// x, y or z, grid.hpp voxel_bit), as bits 0..3
DUST_SURFACE_FN uint32_t column_nibble(uint64_t word, uint32_t off, uint32_t stride) {
  const uint64_t t = word >> off;
  return (uint32_t)((t & 1ull) | ((t >> (stride - 1u)) & 2ull) | ((t >> (2u * stride - 2u)) & 4ull) | ((t >> (3u * stride - 3u)) & 8ull));
}

// c moved down by n bits, 0 <= n < 256 (zeros come in at the top)
DUST_SURFACE_FN Column column_shift_down(const Column& c, uint32_t n) {
  const uint32_t words = n >> 6, bits = n & 63u;
  Column r;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    uint64_t lo = 0, hi = 0;  // words k + words and k + words + 1 of c
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      if (j == k + words) lo = c.w[j];
      if (j == k + words + 1u) hi = c.w[j];
    }
    r.w[k] = bits ? (lo >> bits) | (hi << (64u - bits)) : lo;
  }
  return r;
}

// raw: bit c is the voxel at coordinate c of the axis. The column a walk sees: only coordinates lo..hi (lo <= hi <= 255), bit 0 the
// voxel at hi when the walk comes from the high end, else the voxel at lo; bits hi - lo + 1 and above are 0.
DUST_SURFACE_FN Column column_turn(const Column& raw, uint32_t lo, uint32_t hi, bool from_high) {
  Column c;
  uint32_t down = lo;
  if (from_high) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) c.w[k] = column_reverse(raw.w[3u - k]);  // coordinate x -> bit 255 - x
    down = 255u - hi;
  } else {
    c = raw;
  }
  c = column_shift_down(c, down);
  const uint32_t len = hi - lo + 1u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t keep = len > 64u * k ? len - 64u * k : 0u;  // bits of word k that stay
    c.w[k] = keep >= 64u ? c.w[k] : (c.w[k] & ((1ull << keep) - 1ull));
  }
  return c;
}

// the first voxel of every run: occ & ~(occ << 1), the carry taken across words
DUST_SURFACE_FN Column column_starts(const Column& occ) {
  Column s;
  uint64_t carry = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    s.w[k] = occ.w[k] & ~((occ.w[k] << 1) | carry);
    carry = occ.w[k] >> 63;
  }
  return s;
}
DUST_SURFACE_FN uint32_t column_count(const Column& c) {
  return column_popcount(c.w[0]) + column_popcount(c.w[1]) + column_popcount(c.w[2]) + column_popcount(c.w[3]);
}

// where the k-th set bit of c is (k = 0 the lowest), or kColumnBits when c has k bits or fewer
DUST_SURFACE_FN uint32_t column_kth(const Column& c, uint32_t k) {
  uint64_t word = 0;
  uint32_t base = kColumnBits;
  bool found = false;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    const uint32_t n = column_popcount(c.w[j]);
    if (!found && k < n) { word = c.w[j]; base = 64u * j; found = true; }
    if (!found) k -= n;
  }
  if (!found) return kColumnBits;
  for (; k != 0u; --k) word &= word - 1ull;  // (k < 64 here)
  return base + column_ctz(word);
}

// the number of consecutive set bits of c from bit p upwards (p < 256): the length of the run that starts at p
DUST_SURFACE_FN uint32_t column_ones_from(const Column& c, uint32_t p) {
  uint32_t n = 0;
  bool open = true;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    if (open && p < 64u * (j + 1u)) {
      const uint32_t s = p > 64u * j ? p - 64u * j : 0u;
      const uint32_t t = column_ctz(~(c.w[j] >> s));  // (the zeros the shift brings in end the count at 64 - s)
      n += t;
      open = t == 64u - s;
    }
  }
  return n;
}
// the number of consecutive clear bits of c from bit p - 1 downwards (p <= 256): the length of the gap in front of a run that starts at p
DUST_SURFACE_FN uint32_t column_zeros_below(const Column& c, uint32_t p) {
  uint32_t n = p;
  bool open = true;
#pragma unroll
  for (uint32_t i = 0; i < 4u; ++i) {
    const uint32_t j = 3u - i;
    if (open && p > 64u * j) {
      const uint32_t e = p - 64u * j;  // bits of word j below p
      const uint64_t m = e >= 64u ? c.w[j] : (c.w[j] & ((1ull << e) - 1ull));
      if (m != 0ull) {
        n = p - (64u * j + 64u - column_clz(m));
        open = false;
      }
    }
  }
  return n;
}

// run `layer` of a column (0 = the nearest): where it starts, how long it is, how long the gap in front of it is, and how many runs
// the column has. A column with `layer` runs or fewer: at = kColumnBits, length = gap = 0.
struct ColumnRun {
  uint32_t at, length, gap, runs;
};
DUST_SURFACE_FN ColumnRun column_run(const Column& occ, uint32_t layer) {
  const Column starts = column_starts(occ);
  ColumnRun r;
  r.runs = column_count(starts);
  r.at = column_kth(starts, layer);
  r.length = r.gap = 0u;
  if (r.at != kColumnBits) {
    r.length = column_ones_from(occ, r.at);
    r.gap = column_zeros_below(occ, r.at);
  }
  return r;
}

// the stretch of positions first .. first + count - 1 an apply writes in a column whose run is r: the nearest min(depth, length)
// voxels of the run, or the min(depth, gap) voxels of the gap directly in front of it; count 0 for a miss
struct ColumnSpan {
  uint32_t first, count;
};
DUST_SURFACE_FN ColumnSpan column_span(const ColumnRun& r, uint32_t where, uint32_t depth) {
  ColumnSpan s{0u, 0u};
  if (r.at == kColumnBits) return s;
  if (where == kColumnsGap) {
    s.count = depth < r.gap ? depth : r.gap;
    s.first = r.at - s.count;
  } else {
    s.count = depth < r.length ? depth : r.length;
    s.first = r.at;
  }
  return s;
}

// ---- a cell of the map (DustHipColumnCell as one word) and the two keys of the result
// at | palette << 8 | (length - 1) << 16 | runs << 24; a miss: palette 255, at and length - 1 0
DUST_SURFACE_FN uint32_t column_cell(uint32_t at_coord, uint32_t palette, const ColumnRun& r) {
  if (r.at == kColumnBits) return (255u << 8) | (r.runs << 24);
  return at_coord | (palette << 8) | ((r.length - 1u) << 16) | (r.runs << 24);
}
// the coordinate on the axis of position p of a column turned by column_turn
DUST_SURFACE_FN uint32_t column_coord(uint32_t p, uint32_t lo, uint32_t hi, bool from_high) { return from_high ? hi - p : lo + p; }
// What the device keeps of the nearest and the farthest hit voxel, each with ONE 32-bit atomic maximum over a zeroed word: the depth
// and the key (24 bits) in one word, so that among equal depths the lowest key wins in both. kColumnNoKey when there is no hit.
constexpr uint32_t kColumnNoKey = 0xFFFFFFFFu;
DUST_SURFACE_FN uint32_t column_near_word(uint32_t depth, uint32_t key) { return ~((depth << 24) | key); }
DUST_SURFACE_FN uint32_t column_far_word(uint32_t depth, uint32_t key) { return (depth << 24) | (0xFFFFFFu - key); }
DUST_SURFACE_FN uint32_t column_near_key(uint32_t word) { return ~word & 0xFFFFFFu; }
DUST_SURFACE_FN uint32_t column_far_key(uint32_t word) { return 0xFFFFFFu - (word & 0xFFFFFFu); }

}  // namespace dust
