// shape_cover.hpp -- which voxel centres a box, sphere or capsule of include/dust_hip.h contains: the header's float32 contract,
// operation for operation, as ONE text for everything that decides membership -- k_edit_shapes (edit.hip), k_census (census.hip)
// and, on a CPU, tests/cpp/census_records_test.cpp, which holds it to tests/shape_edit_witness.py. Device-free: no HIP header, plain
// float arithmetic. Every user compiles it with -ffp-contract=off (nothing is fused; `/` is the IEEE division).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DUST_SHAPE_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define DUST_SHAPE_FN inline
#endif

namespace dust {

DUST_SHAPE_FN float shape_dot3(float u0, float u1, float u2, float v0, float v1, float v2) { return (u0 * v0 + u1 * v1) + u2 * v2; }

// what a shape's membership test needs besides the voxel centre: computed once per shape, the same for every voxel
struct ShapeCover {
  float a[3], b[3];
  uint32_t kind;  // DUST_HIP_SHAPE_BOX / SPHERE / CAPSULE
  float rr;       // radius * radius
  float ab[3], l;  // CAPSULE: b - a and dot(ab, ab)
};

DUST_SHAPE_FN ShapeCover shape_cover(const float* a, const float* b, uint32_t kind, float radius) {
  ShapeCover s;
  for (int r = 0; r < 3; ++r) { s.a[r] = a[r]; s.b[r] = b[r]; s.ab[r] = b[r] - a[r]; }
  s.kind = kind;
  s.rr = radius * radius;
  s.l = shape_dot3(s.ab[0], s.ab[1], s.ab[2], s.ab[0], s.ab[1], s.ab[2]);
  return s;
}

// does the shape contain the voxel centre (cx, cy, cz)? (small integers + 0.5: exact in float32)
DUST_SHAPE_FN bool shape_covers(const ShapeCover& s, float cx, float cy, float cz) {
  if (s.kind == 0u) return s.a[0] <= cx && cx <= s.b[0] && s.a[1] <= cy && cy <= s.b[1] && s.a[2] <= cz && cz <= s.b[2];
  const float d0 = cx - s.a[0], d1 = cy - s.a[1], d2 = cz - s.a[2];
  if (s.kind == 1u) return shape_dot3(d0, d1, d2, d0, d1, d2) <= s.rr;
  const float h = s.l == 0.0f ? 0.0f : fminf(fmaxf(shape_dot3(d0, d1, d2, s.ab[0], s.ab[1], s.ab[2]) / s.l, 0.0f), 1.0f);
  const float q0 = d0 - s.ab[0] * h, q1 = d1 - s.ab[1] * h, q2 = d2 - s.ab[2] * h;
  return shape_dot3(q0, q1, q2, q0, q1, q2) <= s.rr;
}

}  // namespace dust
