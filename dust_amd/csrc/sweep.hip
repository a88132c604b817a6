// sweep.hip -- caller-supplied moving world-space boxes against the committed scene (dust_hip_scene_sweep_boxes / _async): how far
// a box can move along delta before it touches a solid voxel, and the face that stops it -- a character controller's move-and-slide,
// thrown props, camera spring arms. The moving counterpart of overlap.hip's boxes; the contract is in include/dust_hip.h.
//
// One query per WAVE, as overlap.hip: persistent workgroups of kSweepWaves waves take kSweepChunk queries at a time from the ray
// queries' device counter (same stream, same protocol). A query:
//  1. lists the instances whose conservative world box (DevBox) meets the swept box (the union of the box at t = 0 and t = 1): the grid
//     cells it covers, the group boxes or every box in id order, as overlap.hip does (a copy: moving that code into a header both
//     kernels include raised k_overlap_boxes' VGPRs). Each listed instance gets the time the box enters
//     its DevBox (the contract's slab times; the DevBox grown by 2^-22 |translation| so that it encloses the float32 voxel corners,
//     whose rounding grows with the translation) and the list is ranked by (entry, id) in LDS. Instances are visited in that order
//     until the next entry is strictly later than the best t (an equal entry with a lower id can still win).
//  2. per instance: the swept box through w2o gives a voxel range; its 256-cells (4096^3 trees) and 16-cells are tested a lane per
//     cell by their own entry times, and only the cells the box enters before the best t have their mid node looked up; the occupied
//     ones are visited in ascending (entry, child) order, and a cell is skipped once its entry is later than the best t.
//     Each mid node is tested a lane per BRICK:
//       Axis-aligned instances: per world axis, the 5 planes of the brick's voxels by the box queries' corner formula; the brick's
//       slab first, then the 4 voxel slabs' entry / exit times; a voxel's T_in / T_out are a max / min of three. The times of an
//       enclosing slab (brick, cell, DevBox) come from the same planes through the same monotone float32 operations, so they enter no
//       later and leave no earlier than their voxels': no margin at those levels.
//       Other instances: a continuous separating-axis test (the box queries' 15 axes, kept in LDS per wave, with each axis' speed
//       delta . L) against the box grown by tau / 2, a brick first, then its voxels.
//  3. per mid node, a wave minimum of (t bits, lane): non-negative floats order as unsigned integers and block ids rise with the lane;
//     the winner is compared with the query's running best (t, instance, block, voxel) lexicographically, and lane 0 writes the
//     32-byte record at the end. No atomics on results; two runs give the same bytes. ANY_HIT ends the query at its first hit.
// Quotients: RN(x / d) as div_by with the query's three reciprocals (exact_div.hpp); the plain IEEE division where d_r is outside
// [2^-100, 2^100] (wave-uniform per query: a subnormal d_r's reciprocal overflows) or where a quotient or numerator leaves the range in
// which the three-operation sequence is exact.
#include "top.hpp"
#include "query.hpp"
#include "exact_div.hpp"

namespace dust {
namespace {

constexpr uint32_t kSweepCand = 256;       // a wave's candidate list in LDS (and as many slots to rank it into)
constexpr uint32_t kSweepGridCells = 512;  // grid cells a swept box may cover for the grid path; more: the group boxes / the id-order scan
constexpr uint32_t kNoMid = 0xFFFFFFFFu;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;   // a lane with nothing to offer to a wave minimum

struct SweepLds {
  uint32_t cand[2 * kSweepCand];  // [0, kSweepCand): as found; [kSweepCand, 2 kSweepCand): ranked by (entry, id)
  float entry[2 * kSweepCand];    // ... and when the box enters each one's DevBox (+inf: never in [0, 1))
  f32x4 axis[16];                 // general instances: the 15 separating axes {L, support of a unit voxel on L}
  f32x4 axis_m[16];               // ... {L . delta, support of the box on L, |L.x| + |L.y| + |L.z|, 1 / |L|}
  float axis_r[16];               // ... 1 / (L . delta)
};
__shared__ SweepLds g_sweep[kSweepWaves];

__device__ __forceinline__ void wave_sync_lds() {  // LDS written by some lanes of the wave, read by others
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float uniform_f(float v) { return __uint_as_float(uniform(__float_as_uint(v))); }
__device__ __forceinline__ bool finite(float v) { return __builtin_isfinite(v); }
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return uniform(v);
}

// one query, as the wave works on it (wave-uniform)
struct Sweep {
  float lo[3], hi[3], d[3];
  float rcp[3];                     // RN(1 / d_r) on the moving axes
  float slo[3], shi[3];             // the swept box: the union of the box at t = 0 and at t = 1
  float big;                        // max |coordinate| of the box at t = 0 and t = 1
  uint32_t moving, slow;            // bit r: d_r != 0; d_r outside [2^-100, 2^100] (the plain division)
  bool any_hit, ignore_start;
  // the best hit so far: (t, inst, block, voxel) is the order; w2 / w3 the record's xyz / palette / voxel words
  float t;
  uint32_t inst, block, voxel, w2, w3;
  float n[3];
};

// RN(a / d_r)
__device__ __forceinline__ float qdiv(float a, const Sweep& q, int r) {
  float v = div_by(a, q.d[r], q.rcp[r], false);
  const float q0 = a * q.rcp[r];
  if (((q.slow >> r) & 1u) || (a != 0.0f && !(fabsf(a) >= 0x1p-100f && fabsf(q0) >= 0x1p-100f && fabsf(q0) <= 0x1p100f))) v = a / q.d[r];
  return v;
}

// the box queries' per-axis rule: v_lo < hi && lo < v_hi; lo == hi: v_lo <= lo < v_hi
__device__ __forceinline__ bool slab_overlap(float vlo, float vhi, float lo, float hi) {
  return lo < hi ? (vlo < hi && lo < vhi) : (vlo <= lo && lo < vhi);
}

// the contract's entry / exit times of the world slab [a, b] on axis r; a resting axis: (-inf, +inf) in contact, else (+inf, -inf)
__device__ __forceinline__ void slab_times(float a, float b, const Sweep& q, int r, float& e, float& x) {
  if ((q.moving >> r) & 1u) {
    const bool pos = q.d[r] > 0.0f;
    e = qdiv(pos ? __fsub_rn(a, q.hi[r]) : __fsub_rn(b, q.lo[r]), q, r);
    x = qdiv(pos ? __fsub_rn(b, q.lo[r]) : __fsub_rn(a, q.hi[r]), q, r);
  } else {
    const bool c = slab_overlap(a, b, q.lo[r], q.hi[r]);
    e = c ? -INFINITY : INFINITY;
    x = c ? INFINITY : -INFINITY;
  }
}

// an enclosing slab (DevBox, cell, brick) the box may enter in [0, 1): its entry time clamped to 0, else +inf
__device__ __forceinline__ float entry_of(float tin, float tout) {
  return (tin < tout && tin < 1.0f && tout > 0.0f) ? fmaxf(tin, 0.0f) : INFINITY;
}

// axis-aligned instance: world coordinate r of a point whose model coordinate c is p (the others 0: their products are +-0, which
// changes at most the sign of a zero result -- the box queries' corner formula, as overlap.hip's aligned_mask)
__device__ __forceinline__ float plane(DUST_RO(float) o2w, int r, int c, float p) {
  const float px = c == 0 ? p : 0.0f, py = c == 1 ? p : 0.0f, pz = c == 2 ? p : 0.0f;
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(o2w[r * 4 + 0], px), __fmul_rn(o2w[r * 4 + 1], py)), __fmul_rn(o2w[r * 4 + 2], pz)), o2w[r * 4 + 3]);
}

// per instance, what the cell and brick tests need
struct SInst {
  uint32_t id;
  DUST_RO(float) o2w;
  bool aligned;
  int col[3];
  int vlo[3], vhi[3];               // the voxel range (inclusive)
  float ctr[3], ext[3];             // general instances: the box's centre at t = 0; per world axis, the half extent of a unit voxel
};

// general instance: the times t in which the parallelepiped o2w([x, x + size]^3) and the box grown by tau / 2 overlap, [tin, tout];
// kin: the axis that enters last (-1: none moves)
__device__ __forceinline__ void sat_times(const SweepLds& L, const SInst& in, float x, float y, float z, float size, const Sweep& q,
                                          float& tin, float& tout, int& kin) {
  const float hx = x + 0.5f * size, hy = y + 0.5f * size, hz = z + 0.5f * size;
  float c[3], big = q.big;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    c[r] = ((in.o2w[r * 4] * hx + in.o2w[r * 4 + 1] * hy) + in.o2w[r * 4 + 2] * hz) + in.o2w[r * 4 + 3];
    big = fmaxf(big, fabsf(c[r]) + in.ext[r] * size);   // the voxel's largest corner coordinate
  }
  const float slack = 0.5e-5f * (1.0f + big);
  const float d0[3] = {c[0] - in.ctr[0], c[1] - in.ctr[1], c[2] - in.ctr[2]};
  tin = -INFINITY; tout = INFINITY; kin = -1;
  for (int k = 0; k < 15; ++k) {
    const f32x4 a = L.axis[k], m = L.axis_m[k];
    const float dist = (a.x * d0[0] + a.y * d0[1]) + a.z * d0[2];
    const float reach = a.w * size + m.y + slack * m.z;
    if (fabsf(m.x) <= 0.25f * slack * m.z) {
      // resting on this axis (it moves less than a quarter of the slack over [0, 1], or the axis is degenerate): in contact or never
      if (fabsf(dist) > reach) { tin = INFINITY; tout = -INFINITY; }
    } else {
      const float e0 = (dist - reach) * L.axis_r[k], e1 = (dist + reach) * L.axis_r[k];
      const float e = fminf(e0, e1), xo = fmaxf(e0, e1);
      if (e > tin) { tin = e; kin = k; }
      tout = fminf(tout, xo);
    }
  }
}

// the entry time (clamped to 0; +inf: never in [0, 1)) of the block of cells at model (x, y, z) of `size` voxels a side
__device__ __forceinline__ float cell_entry(const SweepLds& L, const SInst& in, const Sweep& q, int x, int y, int z, float size) {
  float tin = -INFINITY, tout = INFINITY;
  if (in.aligned) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int c = in.col[r];
      const float p = (float)(c == 0 ? x : (c == 1 ? y : z));
      const float w0 = plane(in.o2w, r, c, p), w1 = plane(in.o2w, r, c, p + size);
      float e, xo;
      slab_times(fminf(w0, w1), fmaxf(w0, w1), q, r, e, xo);
      tin = fmaxf(tin, e); tout = fminf(tout, xo);
    }
  } else {
    int k;
    sat_times(L, in, (float)x, (float)y, (float)z, size, q, tin, tout, k);
  }
  return entry_of(tin, tout);
}

__device__ __forceinline__ float sel4(const float v[4], uint32_t i) {  // (selects, not a private array indexed at run time)
  return i == 0u ? v[0] : (i == 1u ? v[1] : (i == 2u ? v[2] : v[3]));
}

// axis-aligned instance, the brick at model (bx, by, bz): the lane's first hit voxel (best t, lowest bit on ties) and its normal
__device__ __forceinline__ void aligned_brick(const SInst& in, const Sweep& q, int bx, int by, int bz, uint64_t mask, float& best, uint32_t& bit,
                                              float nrm[3]) {
  float w[3][5];
  float btin = -INFINITY, btout = INFINITY;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int c = in.col[r];
    const int b = c == 0 ? bx : (c == 1 ? by : bz);
#pragma unroll
    for (int i = 0; i < 5; ++i) w[r][i] = plane(in.o2w, r, c, (float)(b + i));
    float e, xo;
    slab_times(fminf(w[r][0], w[r][4]), fmaxf(w[r][0], w[r][4]), q, r, e, xo);
    btin = fmaxf(btin, e); btout = fminf(btout, xo);
  }
  if (!(entry_of(btin, btout) <= q.t)) return;
  float e[3][4], x[3][4];  // per world axis, per voxel slab
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) slab_times(fminf(w[r][i], w[r][i + 1]), fmaxf(w[r][i], w[r][i + 1]), q, r, e[r][i], x[r][i]);
  // the same per MODEL axis (col is a permutation: model axis c is world axis r with col[r] == c)
  float E[3][4], X[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      E[c][i] = in.col[0] == c ? e[0][i] : (in.col[1] == c ? e[1][i] : e[2][i]);
      X[c][i] = in.col[0] == c ? x[0][i] : (in.col[1] == c ? x[1][i] : x[2][i]);
    }
  float lane_best = INFINITY;
  uint32_t lane_bit = 0;
#pragma unroll
  for (int ix = 0; ix < 4; ++ix)
#pragma unroll
    for (int iy = 0; iy < 4; ++iy) {
      const float exy = fmaxf(E[0][ix], E[1][iy]), xxy = fminf(X[0][ix], X[1][iy]);
#pragma unroll
      for (int iz = 0; iz < 4; ++iz) {
        const uint32_t v = (uint32_t)(ix * 16 + iy * 4 + iz);
        const float tin = fmaxf(exy, E[2][iz]), tout = fminf(xxy, X[2][iz]);
        const bool hit = ((mask >> v) & 1ull) && tin < tout && tin < 1.0f && tout > 0.0f && (!q.ignore_start || tin >= 0.0f);
        const float t = tin > 0.0f ? tin : 0.0f;
        if (hit && t < lane_best) { lane_best = t; lane_bit = v; }
      }
    }
  if (!(lane_best < INFINITY)) return;
  best = lane_best;
  bit = lane_bit;
  // the normal: -sign(d_r*) on r*, the lowest moving world axis whose entry equals T_in; 0 when the box started inside
  const uint32_t iv[3] = {lane_bit >> 4, (lane_bit >> 2) & 3u, lane_bit & 3u};
  float er[3], tin = -INFINITY;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int c = in.col[r];
    er[r] = sel4(e[r], c == 0 ? iv[0] : (c == 1 ? iv[1] : iv[2]));
    tin = fmaxf(tin, er[r]);
  }
  bool found = !(tin >= 0.0f);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const bool here = !found && ((q.moving >> r) & 1u) && er[r] == tin;
    nrm[r] = here ? (q.d[r] > 0.0f ? -1.0f : 1.0f) : 0.0f;
    found = found || here;
  }
}

// general instance, the brick at model (bx, by, bz): as aligned_brick, by the continuous separating-axis test
__device__ __forceinline__ void general_brick(const SweepLds& L, const SInst& in, const Sweep& q, int bx, int by, int bz, uint64_t mask, float& best,
                                              uint32_t& bit, float nrm[3]) {
  float tin, tout;
  int k;
  sat_times(L, in, (float)bx, (float)by, (float)bz, 4.0f, q, tin, tout, k);
  if (!(entry_of(tin, tout) <= q.t)) return;
  float lane_best = INFINITY, best_tin = 0.0f;
  uint32_t lane_bit = 0;
  int best_k = -1;
  uint64_t rest = mask;
  while (rest) {
    const uint32_t v = (uint32_t)__builtin_ctzll(rest);
    rest &= rest - 1ull;
    sat_times(L, in, (float)(bx + (int)(v >> 4)), (float)(by + (int)((v >> 2) & 3u)), (float)(bz + (int)(v & 3u)), 1.0f, q, tin, tout, k);
    const bool hit = tin < tout && tin < 1.0f && tout > 0.0f && (!q.ignore_start || tin >= 0.0f);
    const float t = tin > 0.0f ? tin : 0.0f;
    if (hit && t < lane_best) { lane_best = t; lane_bit = v; best_tin = tin; best_k = k; }
  }
  if (!(lane_best < INFINITY)) return;
  best = lane_best;
  bit = lane_bit;
  if (best_tin >= 0.0f && best_k >= 0) {  // the axis that entered last, pointing from the voxel toward the box: -sign(delta . L) L / |L|
    const f32x4 a = L.axis[best_k], m = L.axis_m[best_k];
    const float s = m.x > 0.0f ? -m.w : m.w;
    nrm[0] = a.x * s; nrm[1] = a.y * s; nrm[2] = a.z * s;
  } else {
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
  }
}

// one mid node: a lane per brick. Returns true when the query is over (any-hit with a hit)
template <int MODE>
__device__ __forceinline__ bool sweep_mid(Sweep& q, const SInst& in, ModelRef m, const SweepLds& L, uint32_t mid, int gx, int gy, int gz, uint32_t lane) {
  const u32x4 n = *(DUST_RO(u32x4))(m.mid + mid);
  const uint64_t mm = ((uint64_t)n.y << 32) | n.x;
  const int bx = gx + (int)((lane >> 4) & 3u) * 4, by = gy + (int)((lane >> 2) & 3u) * 4, bz = gz + (int)(lane & 3u) * 4;
  const bool in_range = bx <= in.vhi[0] && bx + 3 >= in.vlo[0] && by <= in.vhi[1] && by + 3 >= in.vlo[1] && bz <= in.vhi[2] && bz + 3 >= in.vlo[2];
  float best = INFINITY, nrm[3] = {0.0f, 0.0f, 0.0f};
  uint32_t bit = 0, block = 0;
  DustHipBlock b;
  b.x = b.y = b.z = b.w = 0; b.mask = 0; b.material_ptr = 0; b.avg_albedo = 0;
  if (((mm >> lane) & 1ull) && in_range) {
    block = n.z + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
    b = load_block(m.blocks + block);
    if (in.aligned) aligned_brick(in, q, bx, by, bz, b.mask, best, bit, nrm);
    else general_brick(L, in, q, bx, by, bz, b.mask, best, bit, nrm);
  }
  const uint32_t key = best < INFINITY ? __float_as_uint(best) : kNoKey;
  const uint32_t kmin = wave_min(key);
  if (kmin == kNoKey) return false;
  const uint32_t src = uniform((uint32_t)__builtin_ctzll(__ballot(key == kmin)));   // the lowest lane: the lowest block
  const float t = __uint_as_float(kmin);
  const uint32_t blk = uniform((uint32_t)__shfl((int)block, (int)src, 64)), vb = uniform((uint32_t)__shfl((int)bit, (int)src, 64));
  const bool better = t < q.t || (t == q.t && (in.id < q.inst || (in.id == q.inst && (blk < q.block || (blk == q.block && vb < q.voxel)))));
  if (better) {
    uint32_t w2 = 0, w3 = 0;
    if (lane == src) {
      const uint32_t m1 = (uint32_t)b.mask, m2 = (uint32_t)(b.mask >> 32);
      const uint32_t ma = vb < 32u ? (m1 & ((1u << (vb & 31u)) - 1u)) : m1;
      const uint32_t mb = vb >= 32u ? (m2 & ((1u << ((vb - 32u) & 31u)) - 1u)) : 0u;
      const uint32_t pal = m.materials[b.material_ptr + (uint32_t)__popc(ma) + (uint32_t)__popc(mb)];
      w2 = ((uint32_t)b.x + (vb >> 4)) | (((uint32_t)b.y + ((vb >> 2) & 3u)) << 16);
      w3 = ((uint32_t)b.z + (vb & 3u)) | ((pal & 0xFFu) << 16) | (vb << 24);
    }
    q.t = t; q.inst = in.id; q.block = blk; q.voxel = vb;
    q.w2 = uniform((uint32_t)__shfl((int)w2, (int)src, 64));
    q.w3 = uniform((uint32_t)__shfl((int)w3, (int)src, 64));
#pragma unroll
    for (int r = 0; r < 3; ++r) q.n[r] = uniform_f(__shfl(nrm[r], (int)src, 64));
  }
  return q.any_hit;
}

// the 16-cells in [c0, c1] (16-cell coordinates, inclusive) of one N16 node -- the root of a 256^3 tree (l2 < 0) or level-2 node l2 of
// a 4096^3 tree --: a lane per cell, only the cells the box enters before the best t looked up, the occupied ones in (entry, child) order
template <int MODE>
__device__ __forceinline__ bool sweep_cells(Sweep& q, const SInst& in, ModelRef m, const SweepLds& L, int l2, const int base[3], const int c0[3],
                                            const int c1[3], uint32_t lane) {
  const uint32_t nx = (uint32_t)(c1[0] - c0[0] + 1), ny = (uint32_t)(c1[1] - c0[1] + 1), nz = (uint32_t)(c1[2] - c0[2] + 1);
  const uint32_t cells = nx * ny * nz;
  for (uint32_t s = 0; s < cells; s += 64u) {
    const uint32_t j = s + lane;
    uint32_t mid = kNoMid, idx = 0, key = kNoKey;
    if (j < cells) {
      const uint32_t cz = j % nz, t = j / nz, cy = t % ny, cx = t / ny;
      idx = ((uint32_t)(c0[0] + (int)cx - base[0] / 16) << 8) | ((uint32_t)(c0[1] + (int)cy - base[1] / 16) << 4) | (uint32_t)(c0[2] + (int)cz - base[2] / 16);
      const float ent = cell_entry(L, in, q, (c0[0] + (int)cx) * 16, (c0[1] + (int)cy) * 16, (c0[2] + (int)cz) * 16, 16.0f);
      if (ent <= q.t) {
        if (DEEP && l2 >= 0) {
          const u32x4 cell = *(DUST_RO(u32x4))(m.l2_cells + ((size_t)l2 * 4096u + idx));
          mid = cell.x;
        } else {
          uint32_t child;
          if (n16_child(m.root, -1, idx, child)) mid = child;
        }
        key = mid != kNoMid ? __float_as_uint(ent) : kNoKey;
      }
    }
    for (;;) {
      const uint32_t kmin = wave_min(key);
      if (kmin == kNoKey || __uint_as_float(kmin) > q.t) break;   // (the rest enter later still)
      const uint32_t src = uniform((uint32_t)__builtin_ctzll(__ballot(key == kmin)));
      const uint32_t mu = uniform((uint32_t)__shfl((int)mid, (int)src, 64));
      const uint32_t iu = uniform((uint32_t)__shfl((int)idx, (int)src, 64));
      if (lane == src) key = kNoKey;
      const int gx = base[0] + (int)(iu >> 8) * 16, gy = base[1] + (int)((iu >> 4) & 15u) * 16, gz = base[2] + (int)(iu & 15u) * 16;
      if (sweep_mid<MODE>(q, in, m, L, mu, gx, gy, gz, lane)) return true;
    }
  }
  return false;
}

// one instance the box may enter. Returns true when the query is over (any-hit with a hit)
template <int MODE>
__device__ __forceinline__ bool sweep_instance(ArgsRef a, Sweep& q, uint32_t id, uint32_t lane, SweepLds& L) {
  const DUST_CONST_AS DevVisit& v = a.visits[id];
  ModelRef m = v.m;
  SInst in;
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
  // the voxel range: the swept box (grown by tau / 2 of the box) through w2o, floored, with the box queries' margin for the rounding
  const float grow = aligned ? 0.0f : 0.5e-5f * (1.0f + q.big);
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int c = 0; c < 8; ++c) {
    const V3 p = mk((c & 1) ? q.shi[0] + grow : q.slo[0] - grow, (c & 2) ? q.shi[1] + grow : q.slo[1] - grow, (c & 4) ? q.shi[2] + grow : q.slo[2] - grow);
    const V3 w = xform_point(v.w2o, p);
    mn[0] = fminf(mn[0], w.x); mn[1] = fminf(mn[1], w.y); mn[2] = fminf(mn[2], w.z);
    mx[0] = fmaxf(mx[0], w.x); mx[1] = fmaxf(mx[1], w.y); mx[2] = fmaxf(mx[2], w.z);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float margin = 1.0f + 1e-5f * (((fabsf(v.w2o[k * 4]) + fabsf(v.w2o[k * 4 + 1])) + fabsf(v.w2o[k * 4 + 2])) * (q.big + grow) + fabsf(v.w2o[k * 4 + 3]));
    const float lo = fmaxf(floorf(mn[k] - margin), m.bmin[k]), hi = fminf(floorf(mx[k] + margin), m.bmax[k] - 1.0f);
    if (!(lo <= hi)) return false;
    in.vlo[k] = (int)lo; in.vhi[k] = (int)hi;
  }
  if (!aligned) {
    float half[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      half[r] = 0.5f * q.hi[r] - 0.5f * q.lo[r];
      in.ctr[r] = 0.5f * q.lo[r] + 0.5f * q.hi[r];
      in.ext[r] = 0.5f * ((fabsf(in.o2w[r * 4]) + fabsf(in.o2w[r * 4 + 1])) + fabsf(in.o2w[r * 4 + 2]));
    }
    // the instance's 15 axes (lane k makes axis k; as overlap.hip), with their speed and the box's support on them
    if (lane < 15u) {
      V3 l;
      if (lane < 3u) {
        l = mk(lane == 0u ? 1.0f : 0.0f, lane == 1u ? 1.0f : 0.0f, lane == 2u ? 1.0f : 0.0f);
      } else if (lane < 6u) {
        const int i = ((int)lane - 2) % 3, j = ((int)lane - 1) % 3;
        const V3 u = mk(in.o2w[i], in.o2w[4 + i], in.o2w[8 + i]), w = mk(in.o2w[j], in.o2w[4 + j], in.o2w[8 + j]);
        l = mk(u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x);
      } else {
        const int r = ((int)lane - 6) / 3, i = ((int)lane - 6) % 3;
        const V3 e = mk(in.o2w[i], in.o2w[4 + i], in.o2w[8 + i]);  // (unit r) x column i
        l = r == 0 ? mk(0.0f, -e.z, e.y) : (r == 1 ? mk(e.z, 0.0f, -e.x) : mk(-e.y, e.x, 0.0f));
      }
      float rp = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) rp += 0.5f * fabsf(dot3(l, mk(in.o2w[k], in.o2w[4 + k], in.o2w[8 + k])));
      f32x4 ax, am;
      ax.x = l.x; ax.y = l.y; ax.z = l.z; ax.w = rp * (1.0f + 1e-6f);
      const float s = (l.x * q.d[0] + l.y * q.d[1]) + l.z * q.d[2];
      const float len = sqrtf(dot3(l, l));
      am.x = s;
      am.y = (half[0] * fabsf(l.x) + half[1] * fabsf(l.y)) + half[2] * fabsf(l.z);
      am.z = (fabsf(l.x) + fabsf(l.y)) + fabsf(l.z);
      am.w = len > 0.0f ? 1.0f / len : 0.0f;
      L.axis[lane] = ax;
      L.axis_m[lane] = am;
      L.axis_r[lane] = s != 0.0f ? 1.0f / s : 0.0f;
    }
    wave_sync_lds();
  } else {
#pragma unroll
    for (int r = 0; r < 3; ++r) in.ctr[r] = in.ext[r] = 0.0f;
  }
  const int c0[3] = {in.vlo[0] >> 4, in.vlo[1] >> 4, in.vlo[2] >> 4}, c1[3] = {in.vhi[0] >> 4, in.vhi[1] >> 4, in.vhi[2] >> 4};
  if (!DEEP || m.n_levels == 2) {
    const int base[3] = {0, 0, 0};
    return sweep_cells<MODE>(q, in, m, L, -1, base, c0, c1, lane);
  }
  // 4096^3: the root's 256-cells the box enters before the best t, in ascending child order, then each one's 16-cells
  for (int rx = in.vlo[0] >> 8; rx <= (in.vhi[0] >> 8); ++rx)
    for (int ry = in.vlo[1] >> 8; ry <= (in.vhi[1] >> 8); ++ry)
      for (int rz = in.vlo[2] >> 8; rz <= (in.vhi[2] >> 8); ++rz) {
        if (!(cell_entry(L, in, q, rx * 256, ry * 256, rz * 256, 256.0f) <= q.t)) continue;
        uint32_t l2;
        if (!n16_child(m.root, -1, ((uint32_t)rx << 8) | ((uint32_t)ry << 4) | (uint32_t)rz, l2)) continue;
        const int base[3] = {rx * 256, ry * 256, rz * 256};
        const int s0[3] = {max(c0[0], rx * 16), max(c0[1], ry * 16), max(c0[2], rz * 16)};
        const int s1[3] = {min(c1[0], rx * 16 + 15), min(c1[1], ry * 16 + 15), min(c1[2], rz * 16 + 15)};
        if (sweep_cells<MODE>(q, in, m, L, (int)uniform(l2), base, s0, s1, lane)) return true;
      }
  return false;
}

__device__ __forceinline__ bool box_meets(const Sweep& q, f32x4 blo, f32x4 bhi) {  // (the swept box)
  return q.slo[0] <= bhi.x && blo.x <= q.shi[0] && q.slo[1] <= bhi.y && blo.y <= q.shi[1] && q.slo[2] <= bhi.z && blo.z <= q.shi[2];
}

// when the box enters instance id's DevBox, grown by 2^-22 |translation| per axis: float32 voxel corners round by up to about
// 2^-24 (|w| + |translation|) while the DevBox pads by 1e-4 (|w| + 1), which covers the |w| part only
__device__ __forceinline__ float instance_entry(ArgsRef a, const Sweep& q, uint32_t id) {
  const f32x4 blo = *(DUST_RO(f32x4))(&a.boxes[id].lo[0]), bhi = *(DUST_RO(f32x4))(&a.boxes[id].hi[0]);
  DUST_RO(float) o2w = a.instances[id].o2w;
  const float lo[3] = {blo.x, blo.y, blo.z}, hi[3] = {bhi.x, bhi.y, bhi.z};
  float tin = -INFINITY, tout = INFINITY;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float g = 0x1p-22f * fabsf(o2w[r * 4 + 3]);
    float e, x;
    slab_times(__fsub_rn(lo[r], g), __fadd_rn(hi[r], g), q, r, e, x);
    tin = fmaxf(tin, e); tout = fminf(tout, x);
  }
  return entry_of(tin, tout);
}

// the candidates a wave listed in LDS (unique ids): their entry times, ranked by (entry, id), visited until one enters after the best t
template <int MODE>
__device__ __forceinline__ bool sweep_listed(ArgsRef a, Sweep& q, uint32_t n_cand, uint32_t lane, SweepLds& L) {
  wave_sync_lds();
  for (uint32_t j = lane; j < n_cand; j += 64u) L.entry[j] = instance_entry(a, q, L.cand[j]);
  wave_sync_lds();
  for (uint32_t j = lane; j < n_cand; j += 64u) {
    const uint32_t v = L.cand[j];
    const float e = L.entry[j];
    uint32_t rank = 0;
    for (uint32_t i = 0; i < n_cand; ++i) {
      const float ei = L.entry[i];
      rank += (ei < e || (ei == e && L.cand[i] < v)) ? 1u : 0u;
    }
    L.cand[kSweepCand + rank] = v;
    L.entry[kSweepCand + rank] = e;
  }
  wave_sync_lds();
  for (uint32_t i = 0; i < n_cand; ++i) {
    if (!(uniform_f(L.entry[kSweepCand + i]) <= q.t)) break;
    if (sweep_instance<MODE>(a, q, uniform(L.cand[kSweepCand + i]), lane, L)) return true;
  }
  return false;
}

template <int MODE>
__device__ void sweep_query(ArgsRef a, const SweepArgs& o, uint32_t qi, uint32_t lane, SweepLds& L) {
  const f32x4* bq = reinterpret_cast<const f32x4*>(o.sweeps) + (size_t)qi * 3u;
  const f32x4 b0 = bq[0], b1 = bq[1], b2 = bq[2];
  Sweep q;
  q.lo[0] = b0.x; q.lo[1] = b0.y; q.lo[2] = b0.z;
  q.hi[0] = b1.x; q.hi[1] = b1.y; q.hi[2] = b1.z;
  q.d[0] = b2.x; q.d[1] = b2.y; q.d[2] = b2.z;
  q.any_hit = o.any_hit != 0u;
  q.ignore_start = o.ignore_start != 0u;
  q.t = 1.0f;
  q.inst = 0xFFFFFFFFu;
  q.block = q.voxel = q.w2 = q.w3 = 0u;
  q.n[0] = q.n[1] = q.n[2] = 0.0f;
  q.big = 0.0f;
  q.moving = q.slow = 0u;
  bool ok = a.n_instances != 0u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ok = ok && finite(q.lo[k]) && finite(q.hi[k]) && finite(q.d[k]) && q.lo[k] <= q.hi[k];
    const float end_lo = q.lo[k] + q.d[k], end_hi = q.hi[k] + q.d[k];
    q.slo[k] = fminf(q.lo[k], end_lo);
    q.shi[k] = fmaxf(q.hi[k], end_hi);
    q.big = fmaxf(q.big, fmaxf(fmaxf(fabsf(q.lo[k]), fabsf(q.hi[k])), fmaxf(fabsf(end_lo), fabsf(end_hi))));
    q.moving |= q.d[k] != 0.0f ? (1u << k) : 0u;
    q.slow |= (fabsf(q.d[k]) >= 0x1p-100f && fabsf(q.d[k]) <= 0x1p100f) ? 0u : (1u << k);
    q.rcp[k] = 1.0f / q.d[k];
  }
  if (ok) {
    bool done = false, listed = false;
    const uint64_t lower = (1ull << lane) - 1ull;
    // (1) the grid: the block of cells the swept box covers (as overlap.hip)
    const DUST_CONST_AS DevGrid& g = a.grid;
    uint32_t cl[3] = {0, 0, 0}, ch[3] = {0, 0, 0};
    bool use_grid = g.cells != nullptr;
    if (use_grid) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        cl[k] = (uint32_t)f2i_clamp(floorf((q.slo[k] - g.lo[k]) * g.inv_cell[k]), 0, (int)g.dim[k] - 1);
        ch[k] = (uint32_t)f2i_clamp(floorf((q.shi[k] - g.lo[k]) * g.inv_cell[k]), 0, (int)g.dim[k] - 1);
      }
      use_grid = (ch[0] - cl[0] + 1u) * (ch[1] - cl[1] + 1u) * (ch[2] - cl[2] + 1u) <= kSweepGridCells;
    }
    if (use_grid) {
      uint32_t n_cand = 0;
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
                keep = here && box_meets(q, blo, bhi);
              }
              const uint64_t bal = __ballot(keep);
              const uint32_t at = n_cand + (uint32_t)__popcll(bal & lower);
              if (keep && at < kSweepCand) L.cand[at] = ii;
              n_cand += (uint32_t)__popcll(bal);
            }
          }
      if (n_cand <= kSweepCand) { listed = true; done = sweep_listed<MODE>(a, q, n_cand, lane, L); }
    } else if (LARGE) {
      // (2) a large scene: the group boxes, then the slots of the groups the swept box meets
      uint32_t n_cand = 0;
      for (uint32_t s = 0; s < a.n_groups && n_cand <= kSweepCand; s += 64u) {
        bool meet = false;
        if (s + lane < a.n_groups) {
          const f32x4 glo = *(DUST_RO(f32x4))(&a.gboxes[s + lane].lo[0]), ghi = *(DUST_RO(f32x4))(&a.gboxes[s + lane].hi[0]);
          meet = box_meets(q, glo, ghi);
        }
        uint64_t groups = __ballot(meet);
        while (groups != 0ull && n_cand <= kSweepCand) {
          const uint32_t gi = s + (uint32_t)__builtin_ctzll(groups);
          groups &= groups - 1ull;
          const uint32_t sc = gi * 64u + lane;
          bool keep = false;
          uint32_t ii = 0;
          if (sc < a.n_instances) {
            const f32x4 blo = *(DUST_RO(f32x4))(&a.sboxes[sc].lo[0]), bhi = *(DUST_RO(f32x4))(&a.sboxes[sc].hi[0]);
            ii = __float_as_uint(blo.w);
            keep = box_meets(q, blo, bhi);
          }
          const uint64_t bal = __ballot(keep);
          const uint32_t at = n_cand + (uint32_t)__popcll(bal & lower);
          if (keep && at < kSweepCand) L.cand[at] = ii;
          n_cand += (uint32_t)__popcll(bal);
        }
      }
      if (n_cand <= kSweepCand) { listed = true; done = sweep_listed<MODE>(a, q, n_cand, lane, L); }
    }
    // (3) every instance box in id order, 64 per step (no grid, or a list longer than the LDS takes); each skipped once the best t is
    // earlier than its entry
    for (uint32_t s = 0; !listed && !done && s < a.n_instances; s += 64u) {
      float ent = INFINITY;
      if (s + lane < a.n_instances) {
        const f32x4 blo = *(DUST_RO(f32x4))(&a.boxes[s + lane].lo[0]), bhi = *(DUST_RO(f32x4))(&a.boxes[s + lane].hi[0]);
        if (box_meets(q, blo, bhi)) ent = instance_entry(a, q, s + lane);
      }
      uint64_t bal = __ballot(ent <= q.t);
      while (bal != 0ull && !done) {
        const uint32_t src = (uint32_t)__builtin_ctzll(bal);
        bal &= bal - 1ull;
        if (uniform_f(__shfl(ent, (int)src, 64)) <= q.t) done = sweep_instance<MODE>(a, q, s + src, lane, L);
      }
    }
  }
  if (lane == 0u) {
    u32x4 r0, r1;
    r0.x = __float_as_uint(q.t); r0.y = q.inst; r0.z = q.block; r0.w = q.w2;
    r1.x = q.w3; r1.y = __float_as_uint(q.n[0]); r1.z = __float_as_uint(q.n[1]); r1.w = __float_as_uint(q.n[2]);
    u32x4* out = reinterpret_cast<u32x4*>(o.hits) + (size_t)qi * 2u;
    out[0] = r0;
    out[1] = r1;
  }
}

}  // namespace

// MODE: bit 1 = DEEP (the scene holds a 4096^3 model), bit 2 = LARGE (more than kFlatCullMax instances: the group boxes exist)
template <int MODE>
__global__ void __launch_bounds__(kSweepWaves * 64) k_sweep_boxes(const FrameArgs, const SweepArgs o) {
  ArgsRef a = launch_args();
  if (blockIdx.x == 0 && threadIdx.x == 0) *o.next_counter = 0ull;
  const uint32_t lane = threadIdx.x & 63u;
  SweepLds& L = g_sweep[threadIdx.x >> 6];
  for (;;) {  // the wave's next chunk of queries
    unsigned long long k = 0;
    if (lane == 0) k = atomicAdd(o.counter, (unsigned long long)kSweepChunk);
    k = ((unsigned long long)uniform((uint32_t)(k >> 32)) << 32) | uniform((uint32_t)k);
    if (k >= o.n) break;
    const uint32_t end = (uint32_t)min((unsigned long long)o.n, k + kSweepChunk);
    for (uint32_t qi = (uint32_t)k; qi < end; ++qi) sweep_query<MODE>(a, o, qi, lane, L);
  }
}

// grid, block: the host's choice (capi_scene.cpp sweep_boxes_impl); no dynamic LDS
hipError_t launch_sweep_boxes(const FrameArgs& a, const SweepArgs& o, uint32_t grid, uint32_t block, hipStream_t s) {
  switch ((a.deep ? 2 : 0) | (a.n_groups ? 4 : 0)) {
    case 0: hipLaunchKernelGGL(k_sweep_boxes<0>, dim3(grid), dim3(block), 0, s, a, o); break;
    case 2: hipLaunchKernelGGL(k_sweep_boxes<2>, dim3(grid), dim3(block), 0, s, a, o); break;
    case 4: hipLaunchKernelGGL(k_sweep_boxes<4>, dim3(grid), dim3(block), 0, s, a, o); break;
    default: hipLaunchKernelGGL(k_sweep_boxes<6>, dim3(grid), dim3(block), 0, s, a, o); break;
  }
  return hipGetLastError();
}

}  // namespace dust
