// sweep.hip -- caller-supplied moving world-space boxes against the committed scene (dust_hip_scene_sweep_boxes / _async): how far
// a box can move along delta before it touches a solid voxel, and the face that stops it -- a character controller's move-and-slide,
// thrown props, camera spring arms. The moving counterpart of overlap.hip's boxes; the contract is in include/dust_hip.h.
//
// One query per WAVE, as overlap.hip: persistent workgroups of kSweepWaves waves take kSweepChunk queries at a time from the ray
// queries' device counter (same stream, same protocol). The listing of instances (here: those the SWEPT box meets, the union of the
// box at t = 0 and t = 1), the per-instance voxel range (of the swept box), the separating axes, the float32 formulas and the tree
// steps are box_query.hpp's, shared with overlap.hip (sharing them left the registers where they were: here 256 VGPRs, 84 B scratch
// per lane, 12-14 SGPR spills, one wave per SIMD; k_overlap_boxes 185-191 VGPRs, no scratch, two waves -- docs/EXPERIMENTS.md,
// "Scene box kernels"). What this file owns:
//  1. the order of the visit: each listed instance gets the time the box enters its DevBox (the contract's slab times; the DevBox
//     grown by 2^-22 |translation| so that it encloses the float32 voxel corners, whose rounding grows with the translation) and the
//     list is ranked by (entry, id) in LDS. Instances are visited in that order until the next entry is strictly later than the best
//     t (an equal entry with a lower id can still win). A query that could not be listed tests every instance box in id order.
//  2. per instance: its 256-cells (4096^3 trees) and 16-cells are tested a lane per cell by their own entry times, and only the cells
//     the box enters before the best t have their mid node looked up; the occupied ones are visited in ascending (entry, child) order,
//     and a cell is skipped once its entry is later than the best t. Each mid node is tested a lane per BRICK:
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
#include "box_query.hpp"
#include "exact_div.hpp"

namespace dust {
namespace {

constexpr uint32_t kNoKey = 0xFFFFFFFFu;   // a lane with nothing to offer to a wave minimum

struct SweepLds {
  uint32_t cand[2 * kBoxCand];  // [0, kBoxCand): as found; [kBoxCand, 2 kBoxCand): ranked by (entry, id)
  float entry[2 * kBoxCand];    // ... and when the box enters each one's DevBox (+inf: never in [0, 1))
  f32x4 axis[16];               // general instances: the 15 separating axes {L, support of a unit voxel on L}
  f32x4 axis_m[16];             // ... {L . delta, support of the box on L, |L.x| + |L.y| + |L.z|, 1 / |L|}
  float axis_r[16];             // ... 1 / (L . delta)
};
__shared__ SweepLds g_sweep[kSweepWaves];

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

// general instance: the times t in which the parallelepiped o2w([x, x + size]^3) and the box grown by tau / 2 overlap, [tin, tout];
// kin: the axis that enters last (-1: none moves)
__device__ __forceinline__ void sat_times(const SweepLds& L, const BoxInst& in, float x, float y, float z, float size, const Sweep& q,
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
__device__ __forceinline__ float cell_entry(const SweepLds& L, const BoxInst& in, const Sweep& q, int x, int y, int z, float size) {
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
__device__ __forceinline__ void aligned_brick(const BoxInst& in, const Sweep& q, int bx, int by, int bz, uint64_t mask, float& best, uint32_t& bit,
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
__device__ __forceinline__ void general_brick(const SweepLds& L, const BoxInst& in, const Sweep& q, int bx, int by, int bz, uint64_t mask, float& best,
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

// one mid node (16-cell idx of the node at base): a lane per brick. Returns true when the query is over (any-hit with a hit)
template <int MODE>
__device__ __forceinline__ bool sweep_mid(Sweep& q, const BoxInst& in, ModelRef m, const SweepLds& L, uint32_t mid, const int base[3], uint32_t idx,
                                          uint32_t lane) {
  int bx, by, bz;
  float best = INFINITY, nrm[3] = {0.0f, 0.0f, 0.0f};
  uint32_t bit = 0, block;
  DustHipBlock b;
  b.x = b.y = b.z = b.w = 0; b.mask = 0; b.material_ptr = 0; b.avg_albedo = 0;
  if (lane_brick(m, in, mid, base, idx, lane, bx, by, bz, block)) {
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
    if (lane == src) voxel_words(b, m.materials, vb, w2, w3);
    q.t = t; q.inst = in.id; q.block = blk; q.voxel = vb;
    q.w2 = uniform((uint32_t)__shfl((int)w2, (int)src, 64));
    q.w3 = uniform((uint32_t)__shfl((int)w3, (int)src, 64));
#pragma unroll
    for (int r = 0; r < 3; ++r) q.n[r] = uniform_f(__shfl(nrm[r], (int)src, 64));
  }
  return q.any_hit;
}

// the 16-cells in [c0, c1] of one node (box_query.hpp, visit_nodes): a lane per cell, only the cells the box enters before the best t
// looked up, the occupied ones in (entry, child) order
template <int MODE>
__device__ __forceinline__ bool sweep_cells(Sweep& q, const BoxInst& in, ModelRef m, const SweepLds& L, int l2, const int base[3], const int c0[3],
                                            const int c1[3], uint32_t lane) {
  const CellRange range(base, c0, c1);
  for (uint32_t s = 0; s < range.cells; s += 64u) {
    const uint32_t j = s + lane;
    uint32_t mid = kNoMid, idx = 0, key = kNoKey;
    if (j < range.cells) {
      int x, y, z;
      idx = range.index(j, x, y, z);
      const float ent = cell_entry(L, in, q, x, y, z, 16.0f);
      if (ent <= q.t) {
        mid = cell_mid<MODE>(m, l2, idx);
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
      if (sweep_mid<MODE>(q, in, m, L, mu, base, iu, lane)) return true;
    }
  }
  return false;
}

// one instance the box may enter. Returns true when the query is over (any-hit with a hit)
template <int MODE>
__device__ __forceinline__ bool sweep_instance(ArgsRef a, Sweep& q, uint32_t id, uint32_t lane, SweepLds& L) {
  ModelRef m = a.visits[id].m;
  BoxInst in;
  if (!box_instance(in, a, id, q.slo, q.shi, q.lo, q.hi, q.big)) return false;
  if (!in.aligned) {
    // the instance's 15 axes (lane k makes axis k), with their speed and the box's support on them
    if (lane < 15u) {
      const f32x4 ax = box_axis(in.o2w, lane);
      const V3 l = mk(ax.x, ax.y, ax.z);
      f32x4 am;
      const float s = (l.x * q.d[0] + l.y * q.d[1]) + l.z * q.d[2];
      const float len = sqrtf(dot3(l, l));
      am.x = s;
      am.y = (in.half[0] * fabsf(l.x) + in.half[1] * fabsf(l.y)) + in.half[2] * fabsf(l.z);
      am.z = (fabsf(l.x) + fabsf(l.y)) + fabsf(l.z);
      am.w = len > 0.0f ? 1.0f / len : 0.0f;
      L.axis[lane] = ax;
      L.axis_m[lane] = am;
      L.axis_r[lane] = s != 0.0f ? 1.0f / s : 0.0f;
    }
    wave_sync_lds();
  }
  // (4096^3: only the 256-cells the box enters before the best t)
  return visit_nodes<MODE>(
      m, in, [&](int x, int y, int z, float size) { return cell_entry(L, in, q, x, y, z, size) <= q.t; },
      [&](int l2, const int base[3], const int c0[3], const int c1[3]) { return sweep_cells<MODE>(q, in, m, L, l2, base, c0, c1, lane); });
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
    L.cand[kBoxCand + rank] = v;
    L.entry[kBoxCand + rank] = e;
  }
  wave_sync_lds();
  for (uint32_t i = 0; i < n_cand; ++i) {
    if (!(uniform_f(L.entry[kBoxCand + i]) <= q.t)) break;
    if (sweep_instance<MODE>(a, q, uniform(L.cand[kBoxCand + i]), lane, L)) return true;
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
    const uint32_t n_cand = list_instances<MODE>(a, q.slo, q.shi, L.cand, lane);
    if (n_cand <= kBoxCand) {
      sweep_listed<MODE>(a, q, n_cand, lane, L);
    } else {
      // not listed: every instance box in id order, 64 per step; each skipped once the best t is earlier than its entry
      bool done = false;
      for (uint32_t s = 0; !done && s < a.n_instances; s += 64u) {
        float ent = INFINITY;
        if (s + lane < a.n_instances && instance_meets(a, s + lane, q.slo, q.shi)) ent = instance_entry(a, q, s + lane);
        uint64_t bal = __ballot(ent <= q.t);
        while (bal != 0ull && !done) {
          const uint32_t src = (uint32_t)__builtin_ctzll(bal);
          bal &= bal - 1ull;
          if (uniform_f(__shfl(ent, (int)src, 64)) <= q.t) done = sweep_instance<MODE>(a, q, s + src, lane, L);
        }
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

// MODE: launch_by_mode (box_query.hpp)
template <int MODE>
__global__ void __launch_bounds__(kSweepWaves * 64) k_sweep_boxes(const FrameArgs, const SweepArgs o) {
  ArgsRef a = launch_args();
  if (blockIdx.x == 0 && threadIdx.x == 0) *o.next_counter = 0ull;
  const uint32_t lane = threadIdx.x & 63u;
  SweepLds& L = g_sweep[threadIdx.x >> 6];
  for (;;) {  // the wave's next chunk of queries
    const unsigned long long k = next_chunk(o.counter, kSweepChunk, lane);
    if (k >= o.n) break;
    const uint32_t end = (uint32_t)min((unsigned long long)o.n, k + kSweepChunk);
    for (uint32_t qi = (uint32_t)k; qi < end; ++qi) sweep_query<MODE>(a, o, qi, lane, L);
  }
}

// grid, block: the host's choice (capi_scene.cpp sweep_boxes_impl); no dynamic LDS
hipError_t launch_sweep_boxes(const FrameArgs& a, const SweepArgs& o, uint32_t grid, uint32_t block, hipStream_t s) {
  return launch_by_mode(a, [&](auto mode) { hipLaunchKernelGGL(k_sweep_boxes<decltype(mode)::value>, dim3(grid), dim3(block), 0, s, a, o); });
}

}  // namespace dust
