// triangle_rule.hpp -- which voxels a triangle of include/dust_hip.h touches (dust_hip_model_edit_triangles) and which voxel centres
// of a column lie below it (dust_hip_model_fill_mesh): the header's integer contract as ONE text for everything that decides --
// k_edit_triangles and k_fill_columns (triangle.hip) and, on a CPU, tests/cpp/triangle_rule_test.cpp, which holds it to
// tests/triangle_witness.py. Device-free: no HIP header, no float, every predicate a sign test on int64 values. Vertices are in units
// of 1/256 voxel with |coordinate| <= 2^18, so an edge component is below 2^19 + 1, a normal component at most 2^39 + 2^20 and every
// sum of products below stays under 2^60; voxel and brick coordinates are those of boxes within +-2^18 units too (the tree's always
// are). No array is indexed by a runtime value.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DUST_TRIANGLE_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define DUST_TRIANGLE_FN inline
#endif

namespace dust {

constexpr int32_t kTriangleUnit = 256;         // vertex units per voxel: voxel x is [256 x, 256 x + 256], its centre 256 x + 128
constexpr int32_t kTriangleMaxCoord = 262144;  // |coordinate| <= 2^18

// one of the nine axes e x u: its two components (the one along u is 0), their absolute sum, and the triangle's extent along it
struct TriangleEdgeAxis {
  int32_t ap, aq, r;
  int64_t tmin, tmax;
};

// what the surface rule needs besides the voxel: computed once per triangle, the same for every voxel
struct TriangleSetup {
  int32_t v[3][3];
  int32_t lo[3], hi[3];      // the vertices' extent per axis
  int64_t n[3];              // (v1 - v0) x (v2 - v0)
  int64_t d, nr;             // dot(n, v0) (== dot(n, v1) == dot(n, v2)); |n.x| + |n.y| + |n.z|
  TriangleEdgeAxis axis[9];  // [3 j + u]: edge j (v0->v1, v1->v2, v2->v0) x unit axis u
};

DUST_TRIANGLE_FN int64_t triangle_abs64(int64_t v) { return v < 0 ? -v : v; }
DUST_TRIANGLE_FN int32_t triangle_abs32(int32_t v) { return v < 0 ? -v : v; }
DUST_TRIANGLE_FN int64_t triangle_min64(int64_t a, int64_t b) { return a < b ? a : b; }
DUST_TRIANGLE_FN int64_t triangle_max64(int64_t a, int64_t b) { return a > b ? a : b; }

// every coordinate within +-kTriangleMaxCoord: what triangle_setup requires (beyond: the triangle covers nothing)
DUST_TRIANGLE_FN bool triangle_in_range(const int32_t (&v)[3][3]) {
  bool ok = true;
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) ok = ok && v[k][r] >= -kTriangleMaxCoord && v[k][r] <= kTriangleMaxCoord;
  return ok;
}

DUST_TRIANGLE_FN TriangleSetup triangle_setup(const int32_t (&v)[3][3]) {
  TriangleSetup t;
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) t.v[k][r] = v[k][r];
  for (int r = 0; r < 3; ++r) {
    const int32_t a = v[0][r], b = v[1][r], c = v[2][r];
    t.lo[r] = a < b ? (a < c ? a : c) : (b < c ? b : c);
    t.hi[r] = a > b ? (a > c ? a : c) : (b > c ? b : c);
  }
  const int64_t e1[3] = {int64_t(v[1][0]) - v[0][0], int64_t(v[1][1]) - v[0][1], int64_t(v[1][2]) - v[0][2]};
  const int64_t e2[3] = {int64_t(v[2][0]) - v[0][0], int64_t(v[2][1]) - v[0][1], int64_t(v[2][2]) - v[0][2]};
  t.n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  t.n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  t.n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  t.d = t.n[0] * v[0][0] + t.n[1] * v[0][1] + t.n[2] * v[0][2];
  t.nr = triangle_abs64(t.n[0]) + triangle_abs64(t.n[1]) + triangle_abs64(t.n[2]);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int a = j, b = (j + 1) % 3, c = (j + 2) % 3;  // the edge a -> b; c is the vertex off it
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int p = (u + 1) % 3, q = (u + 2) % 3;  // (e x u)[p] = e[q], (e x u)[q] = -e[p], (e x u)[u] = 0
      TriangleEdgeAxis& x = t.axis[3 * j + u];
      x.ap = v[b][q] - v[a][q];
      x.aq = -(v[b][p] - v[a][p]);
      x.r = triangle_abs32(x.ap) + triangle_abs32(x.aq);
      const int64_t on = int64_t(x.ap) * v[a][p] + int64_t(x.aq) * v[a][q];   // both ends of the edge project here
      const int64_t off = int64_t(x.ap) * v[c][p] + int64_t(x.aq) * v[c][q];
      x.tmin = triangle_min64(on, off);
      x.tmax = triangle_max64(on, off);
    }
  }
  return t;
}

DUST_TRIANGLE_FN bool triangle_degenerate(const TriangleSetup& t) { return t.n[0] == 0 && t.n[1] == 0 && t.n[2] == 0; }

// The 13-axis separating-axis test of the closed triangle against the closed cube [l, l + 2 h]^3 (units; h the half edge): true
// iff no axis separates them, that is iff they share a point. Along an axis a the cube spans dot(a, centre) -+ h * (|a.x| + |a.y| +
// |a.z|), which is the minimum and the maximum of dot(a, corner); the comparisons are strict, so touching covers.
DUST_TRIANGLE_FN bool triangle_touches_box(const TriangleSetup& t, int32_t lx, int32_t ly, int32_t lz, int32_t h) {
  const int32_t c[3] = {lx + h, ly + h, lz + h};
  bool apart = false;
#pragma unroll
  for (int r = 0; r < 3; ++r) apart = apart || t.hi[r] < c[r] - h || t.lo[r] > c[r] + h;
  const int64_t pn = t.n[0] * c[0] + t.n[1] * c[1] + t.n[2] * c[2], rn = t.nr * h;
  apart = apart || t.d < pn - rn || t.d > pn + rn;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const TriangleEdgeAxis& x = t.axis[3 * j + u];
      const int64_t p = int64_t(x.ap) * c[(u + 1) % 3] + int64_t(x.aq) * c[(u + 2) % 3], r = int64_t(x.r) * h;
      apart = apart || x.tmax < p - r || x.tmin > p + r;
    }
  return !apart;
}
// voxel (x, y, z); the coordinates may lie outside the tree
DUST_TRIANGLE_FN bool triangle_covers(const TriangleSetup& t, int32_t x, int32_t y, int32_t z) {
  return triangle_touches_box(t, x * kTriangleUnit, y * kTriangleUnit, z * kTriangleUnit, kTriangleUnit / 2);
}
// the same test for the 4^3 brick (bx, by, bz): false only where triangle_covers is false for every voxel of the brick (along every
// axis the brick's span contains each of its voxels' spans), so asking it first never changes an answer
DUST_TRIANGLE_FN bool triangle_touches_brick(const TriangleSetup& t, int32_t bx, int32_t by, int32_t bz) {
  return triangle_touches_box(t, bx * 4 * kTriangleUnit, by * 4 * kTriangleUnit, bz * 4 * kTriangleUnit, 2 * kTriangleUnit);
}

// What the solid rule needs of a triangle: its vertices, n and s = sign(n.z). Computed once per triangle, the same for every column.
struct TriangleColumn {
  int32_t v[3][3];
  int64_t n[3];  // (v1 - v0) x (v2 - v0)
  int32_t s;     // sign(n.z)
};
DUST_TRIANGLE_FN TriangleColumn triangle_column(const int32_t (&v)[3][3]) {
  TriangleColumn t;
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) t.v[k][r] = v[k][r];
  const int64_t e1[3] = {int64_t(v[1][0]) - v[0][0], int64_t(v[1][1]) - v[0][1], int64_t(v[1][2]) - v[0][2]};
  const int64_t e2[3] = {int64_t(v[2][0]) - v[0][0], int64_t(v[2][1]) - v[0][1], int64_t(v[2][2]) - v[0][2]};
  t.n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  t.n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  t.n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  t.s = t.n[2] > 0 ? 1 : (t.n[2] < 0 ? -1 : 0);
  return t;
}
DUST_TRIANGLE_FN bool triangle_degenerate(const TriangleColumn& t) { return t.n[0] == 0 && t.n[1] == 0 && t.n[2] == 0; }

// The column test of dust_hip_model_fill_mesh: does the vertical line through (px, py) (units) cross the triangle, a line through an
// edge or a vertex shared by several triangles counted for exactly one of those on either side? s == 0: never.
DUST_TRIANGLE_FN bool column_crossed(const TriangleColumn& t, int32_t px, int32_t py) {
  if (t.s == 0) return false;
  bool in = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int a = j, b = (j + 1) % 3;
    const int64_t dx = int64_t(t.s) * (int64_t(t.v[b][0]) - t.v[a][0]), dy = int64_t(t.s) * (int64_t(t.v[b][1]) - t.v[a][1]);
    const int64_t e = dx * (int64_t(py) - t.v[a][1]) - dy * (int64_t(px) - t.v[a][0]);
    in = in && (e > 0 || (e == 0 && (dy > 0 || (dy == 0 && dx < 0))));
  }
  return in;
}

// How many of the column's voxel centres (px, py, 256 z + 128), z = 0 .. 255, the triangle is crossed above: those with
// s * dot(n, c - v0) < 0, the centres 0 .. count - 1 (0 .. 256; a crossing below the tree gives 0, one above it 256). Needs s != 0.
// With B = |n.z| and A = s * (n.x (px - v0.x) + n.y (py - v0.y)) the test is 256 B z < B v0.z - A - 128 B =: U, so the count is
// ceil(U / (256 B)) cut to 0 .. 256.
DUST_TRIANGLE_FN uint32_t crossing_count(const TriangleColumn& t, int32_t px, int32_t py) {
  const int64_t a = int64_t(t.s) * (t.n[0] * (int64_t(px) - t.v[0][0]) + t.n[1] * (int64_t(py) - t.v[0][1]));
  const int64_t b = int64_t(t.s) * t.n[2];
  const int64_t u = b * t.v[0][2] - a - 128 * b, den = 256 * b;
  if (u <= 0) return 0u;
  if (u > 255 * den) return 256u;
  return uint32_t(u / den) + (u % den != 0 ? 1u : 0u);
}

}  // namespace dust
