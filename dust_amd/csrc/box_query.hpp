// box_query.hpp -- what the scene's box kernels share: overlap.hip (boxes at rest) and sweep.hip (moving boxes) take a query per
// WAVE through the same steps, and every margin, tolerance and tie rule of the box-query contract (include/dust_hip.h) stands here once.
//  - the instance listing: which instances' conservative world boxes (DevBox) a world box meets, into the wave's LDS list;
//  - the per-instance setup: axis-aligned or not, the voxel range of a box through w2o with its margins;
//  - the 15 separating axes of a general instance and the support of a unit voxel on them;
//  - the per-axis overlap rule and the float32 corner formula of axis-aligned instances;
//  - the tree steps: the 256-cells of a 4096^3 tree, the 16-cells of a node, the brick of a lane in a mid node;
//  - the record words of a voxel (query.hip's hit record takes its palette index from here too);
//  - the wave helpers, the chunk fetch of the persistent kernels and the launch by MODE (all three query kernels).
// Each kernel keeps what differs: how it ranks and visits the list, what it computes per brick, and its own LDS.
#pragma once
#include <type_traits>

#include "top.hpp"
#include "query.hpp"
#include "grid.hpp"  // uniform

namespace dust {

constexpr uint32_t kBoxCand = 256;       // a wave's candidate list in LDS (the kernels keep as many slots again to rank it into)
constexpr uint32_t kBoxGridCells = 512;  // grid cells a box may cover for the grid path; more: the group boxes / the id-order scan
constexpr uint32_t kNoMid = 0xFFFFFFFFu;

// ---- small helpers
__device__ __forceinline__ void wave_sync_lds() {  // LDS written by some lanes of the wave, read by others
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float uniform_f(float v) { return __uint_as_float(uniform(__float_as_uint(v))); }
__device__ __forceinline__ bool finite(float v) { return __builtin_isfinite(v); }

// the wave's next chunk of queries from the device counter: the index of its first one, the same in every lane
__device__ __forceinline__ unsigned long long next_chunk(unsigned long long* counter, uint32_t chunk, uint32_t lane) {
  unsigned long long k = 0;
  if (lane == 0) k = atomicAdd(counter, (unsigned long long)chunk);
  return ((unsigned long long)uniform((uint32_t)(k >> 32)) << 32) | uniform((uint32_t)k);
}

// the kernel variant of a scene: bit 1 = DEEP (the scene holds a 4096^3 model), bit 2 = LARGE (more than kFlatCullMax instances: the
// group boxes exist). launch(std::integral_constant<int, MODE>) launches that variant.
template <class Launch>
inline hipError_t launch_by_mode(const FrameArgs& a, Launch launch) {
  switch ((a.deep ? 2 : 0) | (a.n_groups ? 4 : 0)) {
    case 0: launch(std::integral_constant<int, 0>()); break;
    case 2: launch(std::integral_constant<int, 2>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    default: launch(std::integral_constant<int, 6>()); break;
  }
  return hipGetLastError();
}

// ---- formulas
// the exact per-axis rule of the header: v_lo < hi && lo < v_hi; lo == hi: v_lo <= lo < v_hi
__device__ __forceinline__ bool slab_overlap(float vlo, float vhi, float lo, float hi) {
  return lo < hi ? (vlo < hi && lo < vhi) : (vlo <= lo && lo < vhi);
}

// axis-aligned instance (one nonzero per row and column of the 3 x 3 part), the header's corner formula: world coordinate r of a point
// whose model coordinate c is p. w_r = ((m[r][0] px + m[r][1] py) + m[r][2] pz) + m[r][3] with the two zero entries' products +-0: the
// same value as fl(fl(m[r][c] p_c) + m[r][3]) (a +-0 term changes at most the sign of a zero result, which no comparison sees)
__device__ __forceinline__ float plane(DUST_RO(float) o2w, int r, int c, float p) {
  const float px = c == 0 ? p : 0.0f, py = c == 1 ? p : 0.0f, pz = c == 2 ? p : 0.0f;
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(o2w[r * 4 + 0], px), __fmul_rn(o2w[r * 4 + 1], py)), __fmul_rn(o2w[r * 4 + 2], pz)), o2w[r * 4 + 3]);
}

// ---- the instance listing
__device__ __forceinline__ bool box_meets(const float lo[3], const float hi[3], f32x4 blo, f32x4 bhi) {
  return lo[0] <= bhi.x && blo.x <= hi[0] && lo[1] <= bhi.y && blo.y <= hi[1] && lo[2] <= bhi.z && blo.z <= hi[2];
}
__device__ __forceinline__ bool instance_meets(ArgsRef a, uint32_t id, const float lo[3], const float hi[3]) {
  return box_meets(lo, hi, *(DUST_RO(f32x4))(&a.boxes[id].lo[0]), *(DUST_RO(f32x4))(&a.boxes[id].hi[0]));
}

// The instances whose DevBox meets [lo, hi], unique and in no order, into cand[0 .. kBoxCand). Returns how many; a value above
// kBoxCand: not listed (the scene has no usable listing for this box, or more meet it than the list holds) -- the caller tests every
// instance box in id order, 64 per step. With a grid and a box over at most kBoxGridCells cells: the cells the box covers, an
// instance accepted in ONE cell only -- the component-wise max of the box's low cell and the instance's own block of cells
// (DevBox.pad0 / pad1). Else, a LARGE scene: the 64-wide group boxes, then the slots of the groups the box meets.
template <int MODE>
__device__ __forceinline__ uint32_t list_instances(ArgsRef a, const float lo[3], const float hi[3], uint32_t* cand, uint32_t lane) {
  const uint64_t lower = (1ull << lane) - 1ull;
  const DUST_CONST_AS DevGrid& g = a.grid;
  uint32_t cl[3] = {0, 0, 0}, ch[3] = {0, 0, 0};
  bool use_grid = g.cells != nullptr;
  if (use_grid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      cl[k] = (uint32_t)f2i_clamp(floorf((lo[k] - g.lo[k]) * g.inv_cell[k]), 0, (int)g.dim[k] - 1);
      ch[k] = (uint32_t)f2i_clamp(floorf((hi[k] - g.lo[k]) * g.inv_cell[k]), 0, (int)g.dim[k] - 1);
    }
    use_grid = (ch[0] - cl[0] + 1u) * (ch[1] - cl[1] + 1u) * (ch[2] - cl[2] + 1u) <= kBoxGridCells;
  }
  uint32_t n_cand = 0;
  if (use_grid) {
    for (uint32_t z = cl[2]; z <= ch[2]; ++z)
      for (uint32_t y = cl[1]; y <= ch[1]; ++y)
        for (uint32_t x = cl[0]; x <= ch[0]; ++x) {
          const uint32_t packed = g.cells[(z * g.dim[1] + y) * g.dim[0] + x];
          const uint32_t first = packed & ((1u << kGridItemBits) - 1u), count = packed >> kGridItemBits;
          for (uint32_t s = 0; s < count; s += 64u) {
            bool keep = false;
            uint32_t ii = 0;
            if (s + lane < count) {
              ii = g.items[first + s + lane];
              const f32x4 blo = *(DUST_RO(f32x4))(&a.boxes[ii].lo[0]), bhi = *(DUST_RO(f32x4))(&a.boxes[ii].hi[0]);
              const uint32_t rl = __float_as_uint(blo.w);
              // the one cell the instance is accepted in: max(the box's low cell, the instance's low cell), per axis
              const bool here = max(cl[0], rl & 255u) == x && max(cl[1], (rl >> 9) & 255u) == y && max(cl[2], (rl >> 18) & 255u) == z;
              keep = here && box_meets(lo, hi, blo, bhi);
            }
            const uint64_t bal = __ballot(keep);
            const uint32_t at = n_cand + (uint32_t)__popcll(bal & lower);
            if (keep && at < kBoxCand) cand[at] = ii;
            n_cand += (uint32_t)__popcll(bal);
          }
        }
  } else if (LARGE) {
    for (uint32_t s = 0; s < a.n_groups && n_cand <= kBoxCand; s += 64u) {
      bool meet = false;
      if (s + lane < a.n_groups) {
        const f32x4 glo = *(DUST_RO(f32x4))(&a.gboxes[s + lane].lo[0]), ghi = *(DUST_RO(f32x4))(&a.gboxes[s + lane].hi[0]);
        meet = box_meets(lo, hi, glo, ghi);
      }
      uint64_t groups = __ballot(meet);
      while (groups != 0ull && n_cand <= kBoxCand) {
        const uint32_t gi = s + (uint32_t)__builtin_ctzll(groups);
        groups &= groups - 1ull;
        const uint32_t sc = gi * 64u + lane;
        bool keep = false;
        uint32_t ii = 0;
        if (sc < a.n_instances) {
          const f32x4 blo = *(DUST_RO(f32x4))(&a.sboxes[sc].lo[0]), bhi = *(DUST_RO(f32x4))(&a.sboxes[sc].hi[0]);
          ii = __float_as_uint(blo.w);
          keep = box_meets(lo, hi, blo, bhi);
        }
        const uint64_t bal = __ballot(keep);
        const uint32_t at = n_cand + (uint32_t)__popcll(bal & lower);
        if (keep && at < kBoxCand) cand[at] = ii;
        n_cand += (uint32_t)__popcll(bal);
      }
    }
  } else {
    n_cand = kBoxCand + 1u;
  }
  return n_cand;
}

// ---- per instance, what the cell and brick tests need
struct BoxInst {
  uint32_t id;
  DUST_RO(float) o2w;
  bool aligned;
  int col[3];                       // axis-aligned: the model axis world axis r takes
  int vlo[3], vhi[3];               // the voxel range (inclusive)
  float half[3], ctr[3], ext[3];    // general instances: the half size and centre of the box at rest; per world axis, the half
                                    // extent of a unit voxel
};

// Instance id against a query: rlo / rhi is the box whose voxel range is wanted (the box itself, or the box swept along its path),
// lo / hi the box at rest and big the largest |coordinate| of the query. The range: the box (grown by tau / 2 of the box for a general
// instance) through w2o, floored, with a margin for the rounding of w2o and its inverse, clamped to the model's bounds. False: empty.
__device__ __forceinline__ bool box_instance(BoxInst& in, ArgsRef a, uint32_t id, const float rlo[3], const float rhi[3], const float lo[3],
                                             const float hi[3], float big) {
  const DUST_CONST_AS DevVisit& v = a.visits[id];
  ModelRef m = v.m;
  in.id = id;
  in.o2w = a.instances[id].o2w;
  int nz_row[3], nz_col[3] = {0, 0, 0};
  bool aligned = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    nz_row[r] = 0;
    in.col[r] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (in.o2w[r * 4 + c] != 0.0f) { nz_row[r] += 1; nz_col[c] += 1; in.col[r] = c; }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) aligned = aligned && nz_row[k] == 1 && nz_col[k] == 1;
  in.aligned = aligned;
  const float grow = aligned ? 0.0f : 0.5e-5f * (1.0f + big);
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int c = 0; c < 8; ++c) {
    const V3 p = mk((c & 1) ? rhi[0] + grow : rlo[0] - grow, (c & 2) ? rhi[1] + grow : rlo[1] - grow, (c & 4) ? rhi[2] + grow : rlo[2] - grow);
    const V3 w = xform_point(v.w2o, p);
    mn[0] = fminf(mn[0], w.x); mn[1] = fminf(mn[1], w.y); mn[2] = fminf(mn[2], w.z);
    mx[0] = fmaxf(mx[0], w.x); mx[1] = fmaxf(mx[1], w.y); mx[2] = fmaxf(mx[2], w.z);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float margin = 1.0f + 1e-5f * (((fabsf(v.w2o[k * 4]) + fabsf(v.w2o[k * 4 + 1])) + fabsf(v.w2o[k * 4 + 2])) * (big + grow) + fabsf(v.w2o[k * 4 + 3]));
    const float l = fmaxf(floorf(mn[k] - margin), m.bmin[k]), h = fminf(floorf(mx[k] + margin), m.bmax[k] - 1.0f);
    if (!(l <= h)) return false;
    in.vlo[k] = (int)l; in.vhi[k] = (int)h;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    in.half[r] = aligned ? 0.0f : 0.5f * hi[r] - 0.5f * lo[r];
    in.ctr[r] = aligned ? 0.0f : 0.5f * lo[r] + 0.5f * hi[r];
    in.ext[r] = aligned ? 0.0f : 0.5f * ((fabsf(in.o2w[r * 4]) + fabsf(in.o2w[r * 4 + 1])) + fabsf(in.o2w[r * 4 + 2]));
  }
  return true;
}

// ---- a general instance's 15 separating axes: the world axes, the voxel's face normals col_i x col_j, world axis r x col_k
__device__ __forceinline__ V3 column(DUST_RO(float) o2w, int k) {  // (selects, not a private array indexed at run time)
  return k == 0 ? mk(o2w[0], o2w[4], o2w[8]) : (k == 1 ? mk(o2w[1], o2w[5], o2w[9]) : mk(o2w[2], o2w[6], o2w[10]));
}
// axis k < 15: {L, the support of a UNIT voxel on L (a brick of 4 has four times as much)}
__device__ __forceinline__ f32x4 box_axis(DUST_RO(float) o2w, uint32_t k) {
  V3 l;
  if (k < 3u) {
    l = mk(k == 0u ? 1.0f : 0.0f, k == 1u ? 1.0f : 0.0f, k == 2u ? 1.0f : 0.0f);
  } else if (k < 6u) {
    const V3 u = column(o2w, ((int)k - 2) % 3), v = column(o2w, ((int)k - 1) % 3);
    l = mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
  } else {
    const int r = ((int)k - 6) / 3;
    const V3 e = column(o2w, ((int)k - 6) % 3);  // (unit r) x e
    l = r == 0 ? mk(0.0f, -e.z, e.y) : (r == 1 ? mk(e.z, 0.0f, -e.x) : mk(-e.y, e.x, 0.0f));
  }
  float rp = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) rp += 0.5f * fabsf(dot3(l, column(o2w, c)));
  f32x4 ax;
  ax.x = l.x; ax.y = l.y; ax.z = l.z; ax.w = rp * (1.0f + 1e-6f);
  return ax;
}

// ---- tree steps
// The 16-cells of the instance's voxel range, node by node: the root of a 256^3 tree, or the level-2 nodes of a 4096^3 tree -- the
// root's 256-cells in ascending child order (x slowest), those enter(x, y, z, 256.0f) lets in. cells(l2, base, c0, c1) takes one
// node's range [c0, c1] (16-cell coordinates, inclusive; base: the node's origin; l2 < 0: the root) and returns true to end the query.
template <int MODE, class Enter, class Cells>
__device__ __forceinline__ bool visit_nodes(ModelRef m, const BoxInst& in, Enter enter, Cells cells) {
  const int c0[3] = {in.vlo[0] >> 4, in.vlo[1] >> 4, in.vlo[2] >> 4}, c1[3] = {in.vhi[0] >> 4, in.vhi[1] >> 4, in.vhi[2] >> 4};
  if (!DEEP || m.n_levels == 2) {
    const int base[3] = {0, 0, 0};
    return cells(-1, base, c0, c1);
  }
  for (int rx = in.vlo[0] >> 8; rx <= (in.vhi[0] >> 8); ++rx)
    for (int ry = in.vlo[1] >> 8; ry <= (in.vhi[1] >> 8); ++ry)
      for (int rz = in.vlo[2] >> 8; rz <= (in.vhi[2] >> 8); ++rz) {
        if (!enter(rx * 256, ry * 256, rz * 256, 256.0f)) continue;
        uint32_t l2;
        if (!n16_child(m.root, -1, ((uint32_t)rx << 8) | ((uint32_t)ry << 4) | (uint32_t)rz, l2)) continue;
        const int base[3] = {rx * 256, ry * 256, rz * 256};
        const int s0[3] = {max(c0[0], rx * 16), max(c0[1], ry * 16), max(c0[2], rz * 16)};
        const int s1[3] = {min(c1[0], rx * 16 + 15), min(c1[1], ry * 16 + 15), min(c1[2], rz * 16 + 15)};
        if (cells((int)uniform(l2), base, s0, s1)) return true;
      }
  return false;
}

// one node's range of 16-cells, a lane per cell: cell j (z fastest) has child index idx in the node and its origin at model (x, y, z)
struct CellRange {
  uint32_t ny, nz, cells;
  int c0[3], off[3];  // the range's low corner; the node's origin, in 16-cells
  __device__ __forceinline__ CellRange(const int base[3], const int lo[3], const int hi[3])
      : ny((uint32_t)(hi[1] - lo[1] + 1)), nz((uint32_t)(hi[2] - lo[2] + 1)), cells((uint32_t)(hi[0] - lo[0] + 1) * ny * nz),
        c0{lo[0], lo[1], lo[2]}, off{base[0] / 16, base[1] / 16, base[2] / 16} {}
  __device__ __forceinline__ uint32_t index(uint32_t j, int& x, int& y, int& z) const {
    const uint32_t cz = j % nz, t = j / nz, cy = t % ny, cx = t / ny;
    x = (c0[0] + (int)cx) * 16; y = (c0[1] + (int)cy) * 16; z = (c0[2] + (int)cz) * 16;
    return ((uint32_t)(c0[0] + (int)cx - off[0]) << 8) | ((uint32_t)(c0[1] + (int)cy - off[1]) << 4) | (uint32_t)(c0[2] + (int)cz - off[2]);
  }
};
// the mid node of 16-cell idx of level-2 node l2 (found in l2_cells) or of the root (l2 < 0); kNoMid: empty
template <int MODE>
__device__ __forceinline__ uint32_t cell_mid(ModelRef m, int l2, uint32_t idx) {
  if (DEEP && l2 >= 0) return (*(DUST_RO(u32x4))(m.l2_cells + ((size_t)l2 * 4096u + idx))).x;
  uint32_t child;
  return n16_child(m.root, -1, idx, child) ? child : kNoMid;
}

// a mid node, a lane per BRICK: the brick of this lane at model (bx, by, bz). True: the brick exists and meets the instance's voxel
// range, and block is its index. (The caller loads the record: with the load in here, into a record handed in by reference, the box
// queries' 64^3 boxes ran 5 % slower -- docs/EXPERIMENTS.md, "Scene box kernels")
__device__ __forceinline__ bool lane_brick(ModelRef m, const BoxInst& in, uint32_t mid, const int base[3], uint32_t idx, uint32_t lane, int& bx, int& by,
                                           int& bz, uint32_t& block) {
  const u32x4 n = *(DUST_RO(u32x4))(m.mid + mid);
  const uint64_t mm = ((uint64_t)n.y << 32) | n.x;
  bx = base[0] + (int)(idx >> 8) * 16 + (int)((lane >> 4) & 3u) * 4;
  by = base[1] + (int)((idx >> 4) & 15u) * 16 + (int)((lane >> 2) & 3u) * 4;
  bz = base[2] + (int)(idx & 15u) * 16 + (int)(lane & 3u) * 4;
  const bool in_range = bx <= in.vhi[0] && bx + 3 >= in.vlo[0] && by <= in.vhi[1] && by + 3 >= in.vlo[1] && bz <= in.vhi[2] && bz + 3 >= in.vlo[2];
  block = n.z + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
  return ((mm >> lane) & 1ull) && in_range;
}

// ---- records
// the palette index of voxel v of a block: the popcount of the mask below v into the block's material stream
__device__ __forceinline__ uint32_t palette_index(const DustHipBlock& b, DUST_RO(uint8_t) materials, uint32_t v) {
  const uint32_t m1 = (uint32_t)b.mask, m2 = (uint32_t)(b.mask >> 32);
  const uint32_t ma = v < 32u ? (m1 & ((1u << (v & 31u)) - 1u)) : m1;
  const uint32_t mb = v >= 32u ? (m2 & ((1u << ((v - 32u) & 31u)) - 1u)) : 0u;
  return materials[b.material_ptr + (uint32_t)__popc(ma) + (uint32_t)__popc(mb)];
}
// the last two words of DustHipVoxelRef, and of DustHipSweepHit's voxel: x | y << 16, z | palette << 16 | voxel << 24
__device__ __forceinline__ void voxel_words(const DustHipBlock& b, DUST_RO(uint8_t) materials, uint32_t v, uint32_t& w2, uint32_t& w3) {
  const uint32_t pal = palette_index(b, materials, v);
  w2 = ((uint32_t)b.x + (v >> 4)) | (((uint32_t)b.y + ((v >> 2) & 3u)) << 16);
  w3 = ((uint32_t)b.z + (v & 3u)) | ((pal & 0xFFu) << 16) | (v << 24);
}

}  // namespace dust
