// walk_cell.hpp -- the cell arithmetic of the conservative brick walk (DESIGN.md "Conservative walk"), in one place: where a visit
// starts, whether the entry point of a whole 16-cell still needs the neighbour visit, and the step out of a cell. Plain float32 and
// integer work over values: no HIP calls, no LDS, no lane operations, no memory access. Both walks of traverse.hpp call these three
// functions -- the packet walk (trace_instance) and the per-lane walk (walk_begin / walk_step) -- so what a ray computes cannot
// depend on which of them carries it; tests/cpp/walk_cell_test.cpp runs the same text on a CPU (tests/test_walk_cell.py).
// Built with -ffp-contract=off, like everything that includes it: every operation below rounds on its own.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DUST_WALK_FN __device__ __forceinline__
#else
#define DUST_WALK_FN inline
#endif

namespace dust {
namespace {

DUST_WALK_FN int f2i_clamp(float f, int lo, int hi) {  // clamp(int(floor-ed f)) with NaN -> lo side of 0
  float c = fminf(fmaxf(f, (float)lo), (float)hi);    // fmaxf(NaN, lo) == lo
  return (int)c;
}

// Where a visit starts, given that the ray meets the model's bounds over [te, tx] (slab_box): the start time t, the cell ijk the ray is
// moving into there, the visit's near-plane tolerance, whether that first cell's entry point needs the exact near-plane test, and the
// time past which the walk has left the bounds. bmin / bmax: the model's tight bounds (multiples of 4), anything indexable.
template <int RT, class Bounds>
DUST_WALK_FN void walk_enter(const float (&oo)[3], const float (&dd)[3], const Bounds& bmin, const Bounds& bmax, float te, float tx, float tmin,
                             float& t, int (&ijk)[3], float& near_tol, bool& screen, float& tx_stop) {
  t = fmaxf(te, 0.0f);
  if (RT >= 2) t = fmaxf(t, tmin * (1.0f - 1e-6f));
  // Near-plane screen (see cell_exit): |p/4 - rint(p/4)| <= near_tol flags an entry point that may lie within
  // delta = 1e-6 (|o_a| + |p_a| + 16) of a brick plane. One tolerance for the whole visit: 3e-7 (20 % above delta / 4,
  // which covers evaluating p at the step's exit time instead of the clamped t) times the largest |o_a| + |p_a| the
  // walk can meet (p is linear in t, so the ends of [te, tx] bound it).
  float reach = 0.0f;
  screen = false;  // does the first cell's entry point need the exact near-plane test?
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // the cell the ray is moving into: floor for d >= 0, ceil - 1 for d < 0 (differs only on a cell plane), kept inside
    // the tight bounds: the start point is the origin inside them or the entry point on them, and an entry point that
    // rounding left a hair outside would otherwise start the walk one (empty) cell early, next to the plane, every time
    const float p = oo[a] + dd[a] * t;
    ijk[a] = f2i_clamp(dd[a] < 0.0f ? ceilf(p) - 1.0f : floorf(p), (int)bmin[a], (int)bmax[a] - 1);
    reach = fmaxf(reach, fabsf(oo[a]) + fmaxf(fabsf(p), fabsf(oo[a] + dd[a] * tx)));
  }
  near_tol = 3.0e-7f * (reach + 16.0f);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // The first cell gets the exact test's own shape with the looser tolerance, because it can tell what the cheap
    // distance-to-a-multiple-of-4 cannot: a walk that starts on the model's bounds (every visit from outside does:
    // the bounds are brick planes) is "near a plane" there by construction, but no brick exists beyond it, and that
    // is not worth a call. (A plane only matters if bricks can exist on its far side.)
    const int b0 = ijk[a] & ~3, blo = (int)bmin[a], bhi = (int)bmax[a] - 1;
    const float q = (oo[a] + dd[a] * t) - (float)b0;
    screen = screen | ((q <= 4.0f * near_tol) & (b0 - 1 >= blo)) | ((q >= 4.0f - 4.0f * near_tol) & (b0 + 4 <= bhi));
  }
  tx_stop = tx * (1.0f + 1e-5f) + 1e-5f;
}

// DEEP variants, `screen` raised, and the cell at ijk is a whole 16-cell with nothing untested in it (empty, missed, or tested brick
// by brick): the bricks inside it need no neighbour visit -- but a brick ACROSS the face the ray came in through does, whatever
// plane its other axes are near (round 2's kernels looked again at 16-plane granularity only and lost one such brick in 4 000
// random deep scenes: tools/stress_parity.py STRESS_DEEP=1, seed 20833). That brick lies in the 16-cell the walk has just
// left: if that was itself a whole cell with nothing untested (prev_whole) there is nothing to do; else its child mask
// is what the cache holds (key, mask4), and the visit is needed only if the mask has a brick there -- or for the rarer shapes (ties,
// two near planes, a near 16-plane). Returns the new `screen`.
DUST_WALK_FN bool whole_cell_screen(const float (&oo)[3], const float (&dd)[3], float t, const int (&ijk)[3], uint32_t stepped, float near_tol,
                                    bool prev_whole, int key, uint64_t mask4) {
  bool near16 = false, across_needed = true, sided = true;
  uint32_t near4 = 0;
  int c[3] = {ijk[0], ijk[1], ijk[2]};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (stepped & (1u << a)) {
      c[a] = dd[a] > 0.0f ? (ijk[a] & ~15) - 1 : (ijk[a] & ~15) + 16;  // back across the face
    } else {
      const float pa = oo[a] + dd[a] * t;
      const float r4 = pa * 0.25f;
      if (fabsf(r4 - rintf(r4)) <= near_tol) {
        near4 += 1u;
        const int b0 = ijk[a] & ~3;
        const float q = pa - (float)b0;
        // (a near plane that is a 16-cell's face has neighbours outside the cell on its own: the exact code looks)
        if (q <= 8.0f * near_tol) { c[a] = b0 - 1; near16 = near16 | ((b0 & 15) == 0); }
        else if (q >= 4.0f - 8.0f * near_tol) { c[a] = b0 + 4; near16 = near16 | (((b0 + 4) & 15) == 0); }
        else sided = false;  // (the integer cell and the point disagree about the side: let the exact code look)
      }
    }
  }
  if (stepped == 0u || near4 == 0u) across_needed = false;  // nothing lies across an entered face and near another plane
  else if (__builtin_popcount(stepped) == 1 && near4 == 1u && sided) {
    // (shifted as unsigned: c[a] is -1 beside plane 0, and no key the cache holds has those high bits)
    const int kd = (int)(((uint32_t)(c[0] >> 4) << 16) | ((uint32_t)(c[1] >> 4) << 8) | (uint32_t)(c[2] >> 4));
    const uint32_t bd = ((uint32_t)((c[0] >> 2) & 3) << 4) | ((uint32_t)((c[1] >> 2) & 3) << 2) | (uint32_t)((c[2] >> 2) & 3);
    if (prev_whole || (kd == key && !((mask4 >> bd) & 1ull))) across_needed = false;
  }
  return (__builtin_popcount(stepped) > 1) | near16 | !sided | across_needed;
}

// Leave the cell of size 2^cl_main that contains ijk: the exit planes come from integer cell coordinates (no accumulated error).
// tn: the exit time; next_ijk: the cell entered there; next_stepped: bit a set when axis a crosses a plane (an exact tie sets several);
// stuck: no axis moves; outside: the step leaves the model's extent E; next_screen: the next cell's entry point may lie within delta
// of further brick planes -- the distance of p to the nearest multiple of 4 on the axes that did not step, or an exact tie on exit --,
// a cheap superset of what the exact near-plane test (visit_neighbours) finds.
DUST_WALK_FN void cell_exit(const float (&oo)[3], const float (&dd)[3], const float (&inv)[3], const int (&ijk)[3], uint32_t cl_main, int E,
                            float near_tol, float& tn, int (&next_ijk)[3], uint32_t& next_stepped, bool& stuck, bool& outside, bool& next_screen) {
  const int S = 1 << cl_main;
  float ta[3];
  int cc[3];
  tn = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cc[a] = ijk[a] & ~(S - 1);
    if (dd[a] != 0.0f) {
      const float plane = (float)(dd[a] > 0.0f ? cc[a] + S : cc[a]);
      ta[a] = (plane - oo[a]) * inv[a];
    } else {
      ta[a] = INFINITY;
    }
    tn = fminf(tn, ta[a]);
  }
  stuck = !(tn < INFINITY);
  next_stepped = 0;
  outside = false;
  next_screen = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (ta[a] == tn) {
      next_stepped |= 1u << a;
      next_ijk[a] = dd[a] > 0.0f ? cc[a] + S : cc[a] - 1;
      if (next_ijk[a] < 0 || next_ijk[a] >= E) outside = true;
    } else {
      const float p = oo[a] + dd[a] * tn;  // the next cell's entry point on an axis that does not cross a plane
      next_ijk[a] = f2i_clamp(floorf(p), cc[a], cc[a] + S - 1);
      const float r = p * 0.25f;
      next_screen = next_screen | (fabsf(r - rintf(r)) <= near_tol);
    }
  }
  next_screen = next_screen | (__builtin_popcount(next_stepped) > 1);
}

}  // namespace
}  // namespace dust
