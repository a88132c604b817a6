// mesh_rule.hpp -- the device-free half of the model meshes (dust_hip_model_mesh): the rule that merges a direction's exposed faces
// into rectangles, as plain functions over the words of a row. Per (direction d, slice) everything the rule needs is three bit planes
// of 256 rows x 256 bits, a row being kMeshRowWords 32-bit words, bit u & 31 of word u >> 5:
//   F  the voxel's face d is in F_d (solid, inside the region, passes the filter, exposed, d among the query's faces);
//   J  the voxel and the one before it along u are both in F and hold the same byte (under ANY_PALETTE: just F & F << 1);
//   K  the same test against the voxel of the row above (row 0: all clear).
// Run starts are F & ~J; a run's end is the bit before the next clear bit of J; a run of a row continues the row above when that
// row starts a run at the same u0 that ends at the same u1 and K joins the two at u0: a fourth plane C, one bit per run start, made
// from the three (mesh_continued_word). A quad starts at a run start whose C bit is clear; its height is 1 + the number of following
// rows whose C has bit u0. No HIP call, no memory access beyond the row pointers handed in, no array indexed past a row. mesh.hip
// calls this text per row out of LDS; tests/cpp/mesh_rule_test.cpp runs it on a CPU (tests/test_mesh_rule.py).
#pragma once
#include <cstdint>

#include "surface_rule.hpp"

#ifdef __HIPCC__
#define DUST_MESH_FN __host__ __device__ __forceinline__
#else
#define DUST_MESH_FN inline
#endif

namespace dust {

constexpr uint32_t kMeshExtent = 256;   // rows of a slice, bits of a row, slices of a direction
constexpr uint32_t kMeshRowWords = 8;   // a row: 256 bits

// ---- axes. Direction d has the normal axis n = d >> 1; in the plane u is the higher-numbered remaining axis, v the other one:
// n = x: u = z, v = y; n = y: u = z, v = x; n = z: u = y, v = x. The voxel at (u, v) of slice s:
DUST_MESH_FN uint32_t mesh_x(uint32_t n, uint32_t s, uint32_t, uint32_t v) { return n == 0u ? s : v; }
DUST_MESH_FN uint32_t mesh_y(uint32_t n, uint32_t s, uint32_t u, uint32_t v) { return n == 0u ? v : (n == 1u ? s : u); }
DUST_MESH_FN uint32_t mesh_z(uint32_t n, uint32_t s, uint32_t u, uint32_t) { return n == 2u ? s : u; }

// the voxels of a brick word (bit x << 4 | y << 2 | z) whose coordinate on axis n is c (0..3)
DUST_MESH_FN uint64_t mesh_slice_plane(uint32_t n, uint32_t c) {
  return n == 0u ? kSurfaceX0 << (16u * c) : (n == 1u ? kSurfaceY0 << (4u * c) : kSurfaceZ0 << c);
}
// of those voxels, the four of row v = j (0..3) of the brick as a nibble, bit i = the voxel at u = i
DUST_MESH_FN uint32_t mesh_row_nibble(uint64_t word, uint32_t n, uint32_t c, uint32_t j) {
  if (n == 0u) return uint32_t(word >> (16u * c + 4u * j)) & 15u;  // x = c, y = j, z = i
  if (n == 1u) return uint32_t(word >> (16u * j + 4u * c)) & 15u;  // x = j, y = c, z = i
  const uint32_t t = uint32_t(word >> (16u * j + c)) & 0x1111u;    // x = j, y = i, z = c: bits 0, 4, 8, 12
  return (t | (t >> 3) | (t >> 6) | (t >> 9)) & 15u;
}
// E_d of a brick from its word and the word of the brick across d (surface_rule.hpp; the other five neighbours do not enter E_d)
DUST_MESH_FN uint64_t mesh_exposure(uint64_t own, uint64_t across, uint32_t d) {
  switch (d) {
    case 0u: return surface_exposure(own, across, 0, 0, 0, 0, 0).e[0];
    case 1u: return surface_exposure(own, 0, across, 0, 0, 0, 0).e[1];
    case 2u: return surface_exposure(own, 0, 0, across, 0, 0, 0).e[2];
    case 3u: return surface_exposure(own, 0, 0, 0, across, 0, 0).e[3];
    case 4u: return surface_exposure(own, 0, 0, 0, 0, across, 0).e[4];
    default: return surface_exposure(own, 0, 0, 0, 0, 0, across).e[5];
  }
}

// ---- rows
DUST_MESH_FN uint32_t mesh_ctz(uint32_t w) { return uint32_t(__builtin_ctz(w)); }  // (w != 0)
DUST_MESH_FN bool mesh_bit(const uint32_t* row, uint32_t u) { return (row[u >> 5] >> (u & 31u)) & 1u; }

// word w of J under ANY_PALETTE: F & F << 1 over the whole row
DUST_MESH_FN uint32_t mesh_join_any(const uint32_t* f_row, uint32_t w) {
  const uint32_t carry = w ? f_row[w - 1u] >> 31 : 0u;
  return f_row[w] & ((f_row[w] << 1) | carry);
}

// the last bit u1 of the run that starts at u0: the bit before the next clear bit of J above u0 (255 when there is none)
DUST_MESH_FN uint32_t mesh_run_end(const uint32_t* j_row, uint32_t u0) {
  uint32_t u = u0 + 1u;
  if (u >= kMeshExtent) return kMeshExtent - 1u;
  uint32_t w = u >> 5;
  uint32_t clear = ~j_row[w] & (~0u << (u & 31u));
  while (clear == 0u) {
    if (++w == kMeshRowWords) return kMeshExtent - 1u;
    clear = ~j_row[w];
  }
  return (w << 5) + mesh_ctz(clear) - 1u;
}

// Word w of a row's C: the run starts of the row whose run is also a run of the row above -- that row starts a run at the same u0,
// K joins the two voxels at u0 (the bytes of a run are all the same, so one voxel decides), and both runs end at the same u1. The row
// must have a row above it (row 0 continues nothing: its C is all clear).
DUST_MESH_FN uint32_t mesh_continued_word(const uint32_t* f_row, const uint32_t* j_row, const uint32_t* k_row, const uint32_t* f_above,
                                          const uint32_t* j_above, uint32_t w) {
  uint32_t c = 0;
  for (uint32_t both = f_row[w] & ~j_row[w] & k_row[w] & f_above[w] & ~j_above[w]; both != 0u; both &= both - 1u) {
    const uint32_t b = mesh_ctz(both), u0 = (w << 5) + b;
    if (mesh_run_end(j_row, u0) == mesh_run_end(j_above, u0)) c |= 1u << b;
  }
  return c;
}

// A walk over the quads that start in row v of a slice whose planes are f, j and c (mesh_continued_word of every row) with `stride`
// words from row to row (>= kMeshRowWords; the kernels pad it): the run starts of the row that continue nothing. A quad's height is
// 1 + the number of following rows whose C has bit u0 -- by induction each of them holds the run u0..u1. visit(u0, u1, v1) is called
// per quad in ascending u0; `heights` false: v1 is not worked out (v1 == v). Returns the number of quads.
template <class Visit>
DUST_MESH_FN uint32_t mesh_row_quads(const uint32_t* f, const uint32_t* j, const uint32_t* c, uint32_t stride, uint32_t v, bool heights, Visit&& visit) {
  const uint32_t* f_row = f + v * stride;
  const uint32_t* j_row = j + v * stride;
  const uint32_t* c_row = c + v * stride;
  uint32_t n = 0;
  for (uint32_t w = 0; w < kMeshRowWords; ++w) {
    for (uint32_t starts = f_row[w] & ~j_row[w] & ~c_row[w]; starts != 0u; starts &= starts - 1u) {
      const uint32_t u0 = (w << 5) + mesh_ctz(starts);
      const uint32_t u1 = mesh_run_end(j_row, u0);
      uint32_t v1 = v;
      if (heights)
        while (v1 + 1u < kMeshExtent && mesh_bit(c + (v1 + 1u) * stride, u0)) ++v1;
      visit(u0, u1, v1);
      ++n;
    }
  }
  return n;
}

// the 64-bit record of a quad (DustHipMeshQuad): key | face << 32 | palette << 40 | du << 48 | dv << 56
DUST_MESH_FN uint64_t mesh_record(uint32_t d, uint32_t s, uint32_t u0, uint32_t u1, uint32_t v0, uint32_t v1, uint32_t palette) {
  const uint32_t n = d >> 1;
  const uint32_t key = (mesh_x(n, s, u0, v0) << 16) | (mesh_y(n, s, u0, v0) << 8) | mesh_z(n, s, u0, v0);
  return uint64_t(key) | (uint64_t(d) << 32) | (uint64_t(palette & 255u) << 40) | (uint64_t(u1 - u0) << 48) | (uint64_t(v1 - v0) << 56);
}

}  // namespace dust
