// top.hpp -- the top-level walk over DevGrid, one ray per lane (included by gi.hip: the ray streams; query.hip: caller-supplied
// rays), and copy16, the workgroup-wide copy into LDS both stage their data with.
#pragma once
#include "traverse.hpp"

namespace dust {

// Top-level walk. A ray steps through the grid's cells (one axis per step, exit planes from integer cell coordinates). The
// instances of a cell are taken in list order; an instance is skipped when the PREVIOUS cell of the path lies inside the block
// of cells the instance is listed in: it was dealt with there. (The cells of a block that lie on a monotone path are
// consecutive, so "listed in the previous cell" is the same as "listed in any earlier cell"; the block rides in the box
// record's spare words.) Boxes are grown by kGridMargin of the scene's size when they are listed (capi_scene.cpp, build_grid): far
// more than the rounding of the cell steps, so a ray that grazes a cell the steps skipped meets no box listed only there.
enum : uint32_t { RS_EMPTY = 0, RS_FETCH, RS_NEXT, RS_TOP, RS_BEGIN, RS_WALK, RS_DONE };
constexpr uint32_t kNoCell = 0xFFFFFFFFu;

// Cell coordinates travel as one word with a guard bit above every 8-bit field: x | y << 9 | z << 18, guards at bits 8, 17, 26.
// "p inside the block [lo, hi]" is then two subtractions: ((p | G) - lo) keeps a field's guard bit iff p >= lo there (no borrow
// leaves a field: 256 + p - lo fits its nine bits), likewise ((hi | G) - p).
constexpr uint32_t kCellGuard = (1u << 8) | (1u << 17) | (1u << 26);
struct TopState {
  uint32_t cell, prev;  // packed as above; prev = the path's previous cell (kNoCell: none)
  uint32_t cur, end;    // what is left of the cell's instance list (indices into DevGrid::items)
  float t_end;          // where the ray leaves the grid or its tmax
};
// where the top-level data is read from: LDS sections behind `base` (offsets of a DevStreamLds), or memory
struct TopSource {
  const unsigned char* base;
  uint32_t cells, items, boxes;  // byte offsets, 0xFFFFFFFF: not staged
};
__device__ __forceinline__ uint32_t grid_index(const DUST_CONST_AS DevGrid& g, uint32_t c) {
  return ((c >> 18) * g.dim[1] + ((c >> 9) & 255u)) * g.dim[0] + (c & 255u);
}
__device__ __forceinline__ void open_cell(ArgsRef a, const TopSource& src, uint32_t c, TopState& ts) {
  const uint32_t idx = grid_index(a.grid, c);
  const uint32_t packed = src.cells != 0xFFFFFFFFu ? reinterpret_cast<const uint32_t*>(src.base + src.cells)[idx] : a.grid.cells[idx];
  ts.cur = packed & ((1u << kGridItemBits) - 1u);
  ts.end = ts.cur + (packed >> kGridItemBits);
}
// the ray's first cell; false: the ray misses the grid (no instance can be hit)
__device__ __forceinline__ bool top_begin(ArgsRef a, const TopSource& src, V3 o, V3 d, V3 inv, float tmin, float tmax, TopState& ts) {
  const DUST_CONST_AS DevGrid& g = a.grid;
  float te, tx;
  if (!slab_box(o, d, inv, g.lo, g.hi, te, tx)) return false;
  const float t0 = fmaxf(fmaxf(te, tmin * (1.0f - 1e-5f)), 0.0f);
  const float t1 = fminf(tx, tmax);
  ts.t_end = t1 * (1.0f + 1e-5f) + 1e-3f;
  if (!(t0 <= ts.t_end)) return false;  // (NaN rays end here too)
  const float p[3] = {o.x + d.x * t0, o.y + d.y * t0, o.z + d.z * t0};
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) c |= (uint32_t)f2i_clamp(floorf((p[k] - g.lo[k]) * g.inv_cell[k]), 0, (int)g.dim[k] - 1) << (9 * k);
  ts.cell = c;
  ts.prev = kNoCell;
  open_cell(a, src, c, ts);
  return true;
}
// About `budget` grid steps / box tests. Returns RS_BEGIN with `inst` = an instance whose box the ray meets in front of `limit`
// (the ray's hit so far, or its tmax), RS_DONE when the ray is over -- out of the grid or of [tmin, tmax], or with a hit in front of
// the current cell's exit: every instance not yet looked at is listed only in cells beyond it --, RS_TOP when the budget ran
// out first. Two loops in turn, so that a wave's lanes share the code they run: (A) step from cell to cell until one lists
// something, (B) test what the cell lists.
// zero_axis (wave-uniform): some ray of the wave has a zero direction component -- the box tests then take the general slab test
__device__ __forceinline__ uint32_t top_next(ArgsRef a, const TopSource& src, V3 o, V3 d, V3 inv, float limit, bool found, TopState& ts, uint32_t& inst,
                                             uint32_t budget, bool zero_axis) {
  const DUST_CONST_AS DevGrid& g = a.grid;
  const bool lds_items = src.items != 0xFFFFFFFFu, lds_boxes_ = src.boxes != 0xFFFFFFFFu;
  for (uint32_t it = 0; it < budget;) {
    while (ts.cur >= ts.end) {  // (A) on to the next cell: the exit planes from the integer cell coordinates, one axis per step (a tie takes
      it += 1u;                 //     the lower axis now, the other one on the next step, at the same t). Selects only: no branch inside
      PROF_COUNT_LANES(P_L_EMPTY4, true);
      const uint32_t c0 = ts.cell & 255u, c1 = (ts.cell >> 9) & 255u, c2 = (ts.cell >> 18) & 255u;
      const bool p0 = d.x > 0.0f, p1 = d.y > 0.0f, p2 = d.z > 0.0f;
      const float q0 = (g.lo[0] + (float)(c0 + (p0 ? 1u : 0u)) * g.cell[0] - o.x) * inv.x;
      const float q1 = (g.lo[1] + (float)(c1 + (p1 ? 1u : 0u)) * g.cell[1] - o.y) * inv.y;
      const float q2 = (g.lo[2] + (float)(c2 + (p2 ? 1u : 0u)) * g.cell[2] - o.z) * inv.z;
      const float t0 = d.x != 0.0f ? q0 : INFINITY, t1 = d.y != 0.0f ? q1 : INFINITY, t2 = d.z != 0.0f ? q2 : INFINITY;
      const float tn = fminf(fminf(t0, t1), t2);
      const bool a0 = t0 <= t1 && t0 <= t2, a1 = !a0 && t1 <= t2;  // the stepping axis: 0, else 1, else 2
      const uint32_t step = a0 ? 1u : (a1 ? 1u << 9 : 1u << 18);
      const uint32_t ca = a0 ? c0 : (a1 ? c1 : c2), da = a0 ? g.dim[0] : (a1 ? g.dim[1] : g.dim[2]);
      const bool up = a0 ? p0 : (a1 ? p1 : p2);
      const bool edge = up ? ca + 1u >= da : ca == 0u;
      // over: no axis moves (a zero or NaN direction), what is left lies behind the hit, the ray's end, the grid's edge
      if (!(tn < INFINITY) || (found && limit < tn * (1.0f - 1e-5f) - 1e-4f) || tn > ts.t_end || edge) return RS_DONE;
      ts.prev = ts.cell;
      ts.cell = up ? ts.cell + step : ts.cell - step;
      open_cell(a, src, ts.cell, ts);
      if (it >= budget) return RS_TOP;
    }
    while (ts.cur < ts.end) {  // (B) the cell's instances
      it += 1u;
      PROF_COUNT_LANES(P_L_BRICK, true);
      const uint32_t ii = lds_items ? reinterpret_cast<const uint16_t*>(src.base + src.items)[ts.cur] : a.grid.items[ts.cur];
      ts.cur += 1u;
      f32x4 blo, bhi;
      if (lds_boxes_) { const f32x4* lb = reinterpret_cast<const f32x4*>(src.base + src.boxes); blo = lb[ii * 2u]; bhi = lb[ii * 2u + 1u]; }
      else { blo = *(DUST_RO(f32x4))(&a.boxes[ii].lo[0]); bhi = *(DUST_RO(f32x4))(&a.boxes[ii].hi[0]); }
      // listed in the cell the ray came from: dealt with there
      const uint32_t rl = __float_as_uint(blo.w), rh = __float_as_uint(bhi.w);
      const bool seen = ts.prev != kNoCell && ((((ts.prev | kCellGuard) - rl) & ((rh | kCellGuard) - ts.prev)) & kCellGuard) == kCellGuard;
      const float lo[3] = {blo.x, blo.y, blo.z}, hi[3] = {bhi.x, bhi.y, bhi.z};
      float te, tx;
      const bool box = zero_axis ? slab_box(o, d, inv, lo, hi, te, tx) : slab_box_nonzero(o, inv, lo, hi, te, tx);
      if (!seen && box && !(te * (1.0f - 2e-6f) > limit)) { inst = ii; return RS_BEGIN; }
      if (it >= budget) break;
    }
  }
  return RS_TOP;
}
__device__ __forceinline__ void copy16(unsigned char* dst, const DUST_CONST_AS void* src, uint32_t bytes) {  // bytes: a multiple of 16 (the image's sections are padded)
  DUST_RO(u32x4) s4 = (DUST_RO(u32x4))src;
  u32x4* d4 = reinterpret_cast<u32x4*>(dst);
  const uint32_t n = bytes / 16u, step = blockDim.x;
  uint32_t i = threadIdx.x;
  for (; i + 3u * step < n; i += 4u * step) {
    const u32x4 v0 = s4[i], v1 = s4[i + step], v2 = s4[i + 2u * step], v3 = s4[i + 3u * step];
    d4[i] = v0; d4[i + step] = v1; d4[i + 2u * step] = v2; d4[i + 3u * step] = v3;
  }
  for (; i < n; i += step) d4[i] = s4[i];
}

}  // namespace dust
