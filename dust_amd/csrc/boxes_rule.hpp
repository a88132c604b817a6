// boxes_rule.hpp -- the device-free half of the model boxes (dust_hip_model_boxes): the rule that stacks the rects of consecutive
// slices into boxes, as plain functions over the words of a row. It stands on mesh_rule.hpp: per slice of the stacking axis n the
// planes are that header's F (here simply S: solid, inside the region, passes the filter), J, K and C, a rect is its quad, and a rect
// start is F & ~J & ~C. New is the third dimension, a fifth plane per slice:
//   D  the rect that starts at (v0, u0) of slice s is also a rect of slice s - 1 -- that slice starts a rect at the same (v0, u0) whose
//      run ends at the same u1 (mesh_run_end) and whose walk down C ends at the same v1, and the two key voxels hold the same byte
//      (all bytes of a rect are equal, so one voxel decides; under ANY_PALETTE the bytes are not asked). The first slice of the
//      region continues nothing: its D is all clear, whatever lies before it.
// A box starts at a rect start whose D bit is clear; its depth is 1 + the number of following slices, up to the region's last, whose D
// has bit (v0, u0) -- by induction each of them holds the identical rect. No HIP call, no memory access beyond the pointers handed
// in, no array indexed past a row or past the D planes of the slices named. boxes.hip calls this text out of LDS (the planes) and
// global memory (the D volume); tests/cpp/boxes_rule_test.cpp runs it on a CPU (tests/test_boxes_rule.py).
#pragma once
#include <cstddef>
#include <cstdint>

#include "mesh_rule.hpp"

namespace dust {

constexpr uint32_t kBoxesPlaneWords = kMeshExtent * kMeshRowWords;  // a slice's D plane in the D volume: rows of 8 words, unpadded (8 KiB)

// the last row v1 of the rect that starts at (v0, u0): a walk down bit column u0 of C (mesh_row_quads' height walk)
DUST_MESH_FN uint32_t boxes_rect_end(const uint32_t* c, uint32_t stride, uint32_t v0, uint32_t u0) {
  uint32_t v1 = v0;
  while (v1 + 1u < kMeshExtent && mesh_bit(c + (v1 + 1u) * stride, u0)) ++v1;
  return v1;
}

// Word w of row v of a slice's D: the rect starts of the row whose rect is also a rect of the slice before. f, j, c are the slice's
// planes, pf, pj, pc those of the slice before it (all with `stride` words from row to row); same_byte(u0) says whether the key voxels
// (v, u0) of the two slices hold the same byte, and is asked only about starts both slices have (always true under ANY_PALETTE). The
// caller leaves D clear for the region's first slice and wherever the slice before is empty.
template <class Same>
DUST_MESH_FN uint32_t boxes_continued_word(const uint32_t* f, const uint32_t* j, const uint32_t* c, const uint32_t* pf, const uint32_t* pj,
                                           const uint32_t* pc, uint32_t stride, uint32_t v, uint32_t w, Same&& same_byte) {
  const uint32_t at = v * stride + w;
  uint32_t d = 0;
  for (uint32_t both = f[at] & ~j[at] & ~c[at] & pf[at] & ~pj[at] & ~pc[at]; both != 0u; both &= both - 1u) {
    const uint32_t b = mesh_ctz(both), u0 = (w << 5) + b;
    if (mesh_run_end(j + v * stride, u0) != mesh_run_end(pj + v * stride, u0)) continue;
    uint32_t v1 = v;  // the two walks down C in step: they end in the same row or the rects differ
    bool here, there;
    for (;;) {
      here = v1 + 1u < kMeshExtent && mesh_bit(c + (v1 + 1u) * stride, u0);
      there = v1 + 1u < kMeshExtent && mesh_bit(pc + (v1 + 1u) * stride, u0);
      if (!here || !there) break;
      ++v1;
    }
    if (here == there && same_byte(u0)) d |= 1u << b;
  }
  return d;
}

// The depth of the box that starts at (v0, u0) of slice s: 1 + the following slices, up to `last` (the region's hi[n]), whose D has
// the bit. dvol holds the D plane of slice t at dvol + t * kBoxesPlaneWords; only slices s + 1 .. last are read.
DUST_MESH_FN uint32_t boxes_depth(const uint32_t* dvol, uint32_t s, uint32_t last, uint32_t v0, uint32_t u0) {
  uint32_t t = s;
  while (t < last && mesh_bit(dvol + size_t(t + 1u) * kBoxesPlaneWords + v0 * kMeshRowWords, u0)) ++t;
  return t - s + 1u;
}

// the 64-bit record of a box (DustHipBox): key | palette << 32 | dx << 40 | dy << 48 | dz << 56, the extents minus 1 along the world
// axes -- the depth lies along n, u1 - u0 along u and v1 - v0 along v (mesh_rule.hpp's axes)
DUST_MESH_FN uint64_t boxes_record(uint32_t n, uint32_t s, uint32_t u0, uint32_t u1, uint32_t v0, uint32_t v1, uint32_t depth, uint32_t palette) {
  const uint32_t key = (mesh_x(n, s, u0, v0) << 16) | (mesh_y(n, s, u0, v0) << 8) | mesh_z(n, s, u0, v0);
  const uint32_t dn = depth - 1u, du = u1 - u0, dv = v1 - v0;
  const uint32_t dx = n == 0u ? dn : dv, dy = n == 0u ? dv : (n == 1u ? dn : du), dz = n == 2u ? dn : du;
  return uint64_t(key) | (uint64_t(palette & 255u) << 32) | (uint64_t(dx) << 40) | (uint64_t(dy) << 48) | (uint64_t(dz) << 56);
}

}  // namespace dust
