// overlap.hip -- caller-supplied world-space boxes against the committed scene (dust_hip_scene_overlap_boxes / _async): every solid
// voxel inside a region -- collision, placement, area edits, trigger volumes. The region counterpart of query.hip's rays.
//
// One query per WAVE. Persistent workgroups of kOverlapWaves waves take kOverlapChunk queries at a time from the ray queries' device
// counter (same stream, same protocol). A query:
//  1. lists the instances whose conservative world box (DevBox) meets it, in ascending id order. With a usable grid: the cells the box
//     covers, an instance accepted in ONE cell only -- the component-wise max of the query's low cell and the instance's own block of
//     cells (DevBox.pad0 / pad1) --, the survivors ranked by id in LDS. A large scene without a grid, or a box over too many cells:
//     the 64-wide group boxes and their slots the same way. A list that does not fit the LDS: every instance box in id order, 64 per step.
//  2. per instance, in that order: the box's corners through w2o give a conservative voxel range (with a margin for the transform's
//     rounding); the root (-> l2 for 4096^3 trees) cells in the range are looked up a lane per 16-cell, the occupied ones taken in
//     ascending child order -- depth-first storage makes that ascending block order (dust_dev.h) -- and each mid node is tested a
//     lane per BRICK: the lane loads its DustHipBlock and makes the mask of its voxels that overlap the box.
//       Axis-aligned instances (one nonzero per row and column of the 3 x 3 part): the voxel's world box on world axis r depends on
//       ONE model coordinate, so the test is separable -- 4 voxel slabs per axis, exactly the header's float32 formula (no contraction:
//       -ffp-contract=off), and the 64-bit mask is their outer product.
//       Other instances: a separating-axis test of the voxel's world parallelepiped against the box grown by tau / 2 (15 axes: the
//       world axes, the voxel's face normals, the 9 edge cross products; the axes are the instance's, kept in LDS per wave), a brick
//       first, then its voxels.
//  3. slots come from a wave-wide exclusive prefix of the lanes' counts plus the query's running total: records leave in (instance,
//     block, voxel bit) order without atomics, the first `capacity` of them kept, nothing at or beyond n_records written.
#include "top.hpp"
#include "query.hpp"

namespace dust {
namespace {

constexpr uint32_t kOverlapCand = 256;       // a wave's candidate list in LDS (and as many slots to rank it into)
constexpr uint32_t kOverlapGridCells = 512;  // grid cells a box may cover for the grid path; more: the group boxes / the id-order scan
constexpr uint32_t kNoMid = 0xFFFFFFFFu;

struct OverlapLds {
  uint32_t cand[2 * kOverlapCand];  // [0, kOverlapCand): as found; [kOverlapCand, 2 kOverlapCand): ranked by id
  f32x4 axis[16];                   // the 15 separating axes of the instance being tested: {L, R = support of voxel + box}
  float axis_s[16];                 // ... and |L.x| + |L.y| + |L.z| (what the tolerance grows R by per unit)
};
__shared__ OverlapLds g_overlap[kOverlapWaves];

__device__ __forceinline__ void wave_sync_lds() {  // LDS written by some lanes of the wave, read by others
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ bool finite(float v) { return __builtin_isfinite(v); }

// one query, as the wave works on it
struct Query {
  float lo[3], hi[3];
  float big;                        // max |coordinate| of the box
  uint64_t first, cap, n_records;
  uint64_t total;                   // overlapping voxels so far
  bool any_hit;
};

// the exact per-axis rule of the header: v_lo < hi && lo < v_hi; lo == hi: v_lo <= lo < v_hi
__device__ __forceinline__ bool slab_overlap(float vlo, float vhi, float lo, float hi) {
  return lo < hi ? (vlo < hi && lo < vhi) : (vlo <= lo && lo < vhi);
}

// axis-aligned instance: the mask of a brick's voxels at (bx, by, bz) whose world box overlaps the query. col[r]: the model axis world
// axis r takes; w_r = ((m[r][0] px + m[r][1] py) + m[r][2] pz) + m[r][3] with the two zero entries' products +-0: the same value as
// fl(fl(m[r][c] p_c) + m[r][3]) (a +-0 term changes at most the sign of a zero result, which no comparison sees)
__device__ __forceinline__ uint64_t aligned_mask(DUST_RO(float) o2w, const int col[3], int bx, int by, int bz, const Query& q) {
  uint32_t m4x = 0u, m4y = 0u, m4z = 0u;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int c = col[r];
    const int b = c == 0 ? bx : (c == 1 ? by : bz);
    float w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float p = (float)(b + i);
      const float px = c == 0 ? p : 0.0f, py = c == 1 ? p : 0.0f, pz = c == 2 ? p : 0.0f;
      w[i] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(o2w[r * 4 + 0], px), __fmul_rn(o2w[r * 4 + 1], py)), __fmul_rn(o2w[r * 4 + 2], pz)), o2w[r * 4 + 3]);
    }
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) bits |= slab_overlap(fminf(w[i], w[i + 1]), fmaxf(w[i], w[i + 1]), q.lo[r], q.hi[r]) ? (1u << i) : 0u;
    m4x |= c == 0 ? bits : 0u; m4y |= c == 1 ? bits : 0u; m4z |= c == 2 ? bits : 0u;
  }
  uint32_t yz = 0;  // bit iy << 2 | iz
#pragma unroll
  for (int iy = 0; iy < 4; ++iy) yz |= ((m4y >> iy) & 1u) ? (m4z << (4 * iy)) : 0u;
  uint64_t all = 0;
#pragma unroll
  for (int ix = 0; ix < 4; ++ix) all |= ((m4x >> ix) & 1u) ? ((uint64_t)yz << (16 * ix)) : 0ull;
  return all;
}

// general instance: does the parallelepiped o2w([x, x + size]^3) overlap the box grown by tau / 2? (the axes and their supports for
// a UNIT voxel are in the wave's LDS; a brick of 4 scales the parallelepiped's part of R by 4)
__device__ __forceinline__ bool sat_overlap(const OverlapLds& L, DUST_RO(float) o2w, float x, float y, float z, float size, const Query& q,
                                            const float half[3], const float ctr[3], const float ext[3]) {
  const float hx = x + 0.5f * size, hy = y + 0.5f * size, hz = z + 0.5f * size;
  float c[3], big = q.big;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    c[r] = ((o2w[r * 4] * hx + o2w[r * 4 + 1] * hy) + o2w[r * 4 + 2] * hz) + o2w[r * 4 + 3];
    big = fmaxf(big, fabsf(c[r]) + ext[r] * size);   // the voxel's largest corner coordinate
  }
  const float slack = 0.5e-5f * (1.0f + big);
  const float d[3] = {c[0] - ctr[0], c[1] - ctr[1], c[2] - ctr[2]};
  bool ok = true;
  for (int k = 0; k < 15; ++k) {
    const f32x4 a = L.axis[k];
    const float dist = fabsf((a.x * d[0] + a.y * d[1]) + a.z * d[2]);
    // a.w = sum_k |L.e_k| (unit voxel) ; the box's support is added here (the same for every voxel)
    const float rq = (half[0] * fabsf(a.x) + half[1] * fabsf(a.y)) + half[2] * fabsf(a.z);
    ok = ok && !(dist > a.w * size + rq + slack * L.axis_s[k]);
  }
  return ok;
}

// the instance's 15 axes into the wave's LDS (lane k < 15 makes axis k): world axes, face normals col_i x col_j, world axis x col_k
__device__ __forceinline__ V3 column(DUST_RO(float) o2w, int k) {  // (selects, not a private array indexed at run time)
  return k == 0 ? mk(o2w[0], o2w[4], o2w[8]) : (k == 1 ? mk(o2w[1], o2w[5], o2w[9]) : mk(o2w[2], o2w[6], o2w[10]));
}
__device__ __forceinline__ void make_axes(OverlapLds& L, DUST_RO(float) o2w, uint32_t lane) {
  if (lane < 15u) {
    V3 l;
    if (lane < 3u) {
      l = mk(lane == 0u ? 1.0f : 0.0f, lane == 1u ? 1.0f : 0.0f, lane == 2u ? 1.0f : 0.0f);
    } else if (lane < 6u) {
      const V3 u = column(o2w, ((int)lane - 2) % 3), v = column(o2w, ((int)lane - 1) % 3);
      l = mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
    } else {
      const int r = ((int)lane - 6) / 3;
      const V3 e = column(o2w, ((int)lane - 6) % 3);  // (unit r) x e
      l = r == 0 ? mk(0.0f, -e.z, e.y) : (r == 1 ? mk(e.z, 0.0f, -e.x) : mk(-e.y, e.x, 0.0f));
    }
    float rp = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) rp += 0.5f * fabsf(dot3(l, column(o2w, k)));
    f32x4 a;
    a.x = l.x; a.y = l.y; a.z = l.z; a.w = rp * (1.0f + 1e-6f);
    L.axis[lane] = a;
    L.axis_s[lane] = (fabsf(l.x) + fabsf(l.y)) + fabsf(l.z);
  }
  wave_sync_lds();
}

// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// a voxel record: {instance, block, x | y << 16, z | palette << 16 | voxel << 24}
__device__ __forceinline__ void put_ref(const OverlapArgs& o, uint64_t at, uint32_t inst, uint32_t block, const DustHipBlock& b,
                                        DUST_RO(uint8_t) materials, uint32_t v) {
  const uint32_t m1 = (uint32_t)b.mask, m2 = (uint32_t)(b.mask >> 32);
  const uint32_t ma = v < 32u ? (m1 & ((1u << (v & 31u)) - 1u)) : m1;
  const uint32_t mb = v >= 32u ? (m2 & ((1u << ((v - 32u) & 31u)) - 1u)) : 0u;
  const uint32_t pal = materials[b.material_ptr + (uint32_t)__popc(ma) + (uint32_t)__popc(mb)];
  u32x4 r;
  r.x = inst; r.y = block;
  r.z = ((uint32_t)b.x + (v >> 4)) | (((uint32_t)b.y + ((v >> 2) & 3u)) << 16);
  r.w = ((uint32_t)b.z + (v & 3u)) | ((pal & 0xFFu) << 16) | (v << 24);
  reinterpret_cast<u32x4*>(o.records)[at] = r;
}

// per instance, what the brick tests need
struct Inst {
  uint32_t id;
  DUST_RO(float) o2w;
  bool aligned;
  int col[3];
  int vlo[3], vhi[3];               // the voxel range (inclusive)
  float half[3], ctr[3], ext[3];    // general instances: the box's half size and centre; per world axis,
                                    // the half extent of a unit voxel
};

// one mid node: a lane per brick. Returns true when the query is over (any-hit with a hit)
template <int MODE>
__device__ __forceinline__ bool visit_mid(const OverlapArgs& o, Query& q, const Inst& in, ModelRef m, const OverlapLds& L, uint32_t mid, int gx, int gy,
                                          int gz, uint32_t lane) {
  const u32x4 n = *(DUST_RO(u32x4))(m.mid + mid);
  const uint64_t mm = ((uint64_t)n.y << 32) | n.x;
  const int bx = gx + (int)((lane >> 4) & 3u) * 4, by = gy + (int)((lane >> 2) & 3u) * 4, bz = gz + (int)(lane & 3u) * 4;
  const bool in_range = bx <= in.vhi[0] && bx + 3 >= in.vlo[0] && by <= in.vhi[1] && by + 3 >= in.vlo[1] && bz <= in.vhi[2] && bz + 3 >= in.vlo[2];
  uint64_t pass = 0;
  uint32_t block = 0;
  DustHipBlock b;
  b.x = b.y = b.z = b.w = 0; b.mask = 0; b.material_ptr = 0; b.avg_albedo = 0;
  if (((mm >> lane) & 1ull) && in_range) {
    block = n.z + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
    b = load_block(m.blocks + block);
    if (in.aligned) {
      pass = aligned_mask(in.o2w, in.col, bx, by, bz, q) & b.mask;
    } else if (sat_overlap(L, in.o2w, (float)bx, (float)by, (float)bz, 4.0f, q, in.half, in.ctr, in.ext)) {
      uint64_t rest = b.mask;
      while (rest) {
        const uint32_t v = (uint32_t)__builtin_ctzll(rest);
        rest &= rest - 1ull;
        if (sat_overlap(L, in.o2w, (float)(bx + (int)(v >> 4)), (float)(by + (int)((v >> 2) & 3u)), (float)(bz + (int)(v & 3u)), 1.0f, q, in.half,
                        in.ctr, in.ext))
          pass |= 1ull << v;
      }
    }
  }
  const uint32_t cnt = (uint32_t)__popcll(pass);
  const uint64_t some = __ballot(cnt != 0u);
  if (some == 0ull) return false;
  if (q.any_hit) {  // one voxel of the first lane that has one
    if (lane == (uint32_t)__builtin_ctzll(some) && q.cap >= 1u && q.first < q.n_records)
      put_ref(o, q.first, in.id, block, b, m.materials, (uint32_t)__builtin_ctzll(pass));
    q.total = 1;
    return true;
  }
  const uint32_t incl = wave_scan(cnt, lane);
  const uint32_t sum = uniform((uint32_t)__shfl((int)incl, 63, 64));
  uint64_t slot = q.total + (incl - cnt);
  uint64_t rest = pass;
  while (rest != 0ull && slot < q.cap && q.first + slot < q.n_records) {
    const uint32_t v = (uint32_t)__builtin_ctzll(rest);
    rest &= rest - 1ull;
    put_ref(o, q.first + slot, in.id, block, b, m.materials, v);
    slot += 1u;
  }
  q.total += sum;
  return false;
}

// the occupied 16-cells in [c0, c1] (16-cell coordinates, inclusive) of one N16 node -- the root of a 256^3 tree (node = root,
// l2 < 0) or level-2 node l2 of a 4096^3 tree, whose 16-cells are found in l2_cells -- in ascending child order; base: the node's origin
template <int MODE>
__device__ __forceinline__ bool visit_cells(const OverlapArgs& o, Query& q, const Inst& in, ModelRef m, const OverlapLds& L, int l2, const int base[3],
                                            const int c0[3], const int c1[3], uint32_t lane) {
  const uint32_t nx = (uint32_t)(c1[0] - c0[0] + 1), ny = (uint32_t)(c1[1] - c0[1] + 1), nz = (uint32_t)(c1[2] - c0[2] + 1);
  const uint32_t cells = nx * ny * nz;
  for (uint32_t s = 0; s < cells; s += 64u) {
    const uint32_t j = s + lane;
    uint32_t mid = kNoMid, idx = 0;
    if (j < cells) {
      const uint32_t cz = j % nz, t = j / nz, cy = t % ny, cx = t / ny;
      idx = ((uint32_t)(c0[0] + (int)cx - base[0] / 16) << 8) | ((uint32_t)(c0[1] + (int)cy - base[1] / 16) << 4) | (uint32_t)(c0[2] + (int)cz - base[2] / 16);
      if (DEEP && l2 >= 0) {
        const u32x4 cell = *(DUST_RO(u32x4))(m.l2_cells + ((size_t)l2 * 4096u + idx));
        mid = cell.x;
      } else {
        uint32_t child;
        if (n16_child(m.root, -1, idx, child)) mid = child;
      }
    }
    uint64_t occ = __ballot(mid != kNoMid);
    while (occ != 0ull) {
      const uint32_t src = (uint32_t)__builtin_ctzll(occ);
      occ &= occ - 1ull;
      const uint32_t mu = uniform((uint32_t)__shfl((int)mid, (int)src, 64));
      const uint32_t iu = uniform((uint32_t)__shfl((int)idx, (int)src, 64));
      const int gx = base[0] + (int)(iu >> 8) * 16, gy = base[1] + (int)((iu >> 4) & 15u) * 16, gz = base[2] + (int)(iu & 15u) * 16;
      if (visit_mid<MODE>(o, q, in, m, L, mu, gx, gy, gz, lane)) return true;
    }
  }
  return false;
}

// one instance whose world box meets the query. Returns true when the query is over (any-hit with a hit)
template <int MODE>
__device__ bool visit_instance(ArgsRef a, const OverlapArgs& o, Query& q, uint32_t id, uint32_t lane, OverlapLds& L) {
  const DUST_CONST_AS DevVisit& v = a.visits[id];
  ModelRef m = v.m;
  Inst in;
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
  // the voxel range: the box (grown by tau / 2 of the box) through w2o, floored, with a margin for the rounding of w2o and its inverse
  const float grow = aligned ? 0.0f : 0.5e-5f * (1.0f + q.big);
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int c = 0; c < 8; ++c) {
    const V3 p = mk((c & 1) ? q.hi[0] + grow : q.lo[0] - grow, (c & 2) ? q.hi[1] + grow : q.lo[1] - grow, (c & 4) ? q.hi[2] + grow : q.lo[2] - grow);
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
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      in.half[r] = 0.5f * q.hi[r] - 0.5f * q.lo[r];
      in.ctr[r] = 0.5f * q.lo[r] + 0.5f * q.hi[r];
      in.ext[r] = 0.5f * ((fabsf(in.o2w[r * 4]) + fabsf(in.o2w[r * 4 + 1])) + fabsf(in.o2w[r * 4 + 2]));
    }
    make_axes(L, in.o2w, lane);
  } else {
#pragma unroll
    for (int r = 0; r < 3; ++r) in.half[r] = in.ctr[r] = in.ext[r] = 0.0f;
  }
  const int c0[3] = {in.vlo[0] >> 4, in.vlo[1] >> 4, in.vlo[2] >> 4}, c1[3] = {in.vhi[0] >> 4, in.vhi[1] >> 4, in.vhi[2] >> 4};
  if (!DEEP || m.n_levels == 2) {
    const int base[3] = {0, 0, 0};
    return visit_cells<MODE>(o, q, in, m, L, -1, base, c0, c1, lane);
  }
  // 4096^3: the root's 256-cells in ascending child order (x slowest), then each one's 16-cells
  for (int rx = in.vlo[0] >> 8; rx <= (in.vhi[0] >> 8); ++rx)
    for (int ry = in.vlo[1] >> 8; ry <= (in.vhi[1] >> 8); ++ry)
      for (int rz = in.vlo[2] >> 8; rz <= (in.vhi[2] >> 8); ++rz) {
        uint32_t l2;
        if (!n16_child(m.root, -1, ((uint32_t)rx << 8) | ((uint32_t)ry << 4) | (uint32_t)rz, l2)) continue;
        const int base[3] = {rx * 256, ry * 256, rz * 256};
        const int s0[3] = {max(c0[0], rx * 16), max(c0[1], ry * 16), max(c0[2], rz * 16)};
        const int s1[3] = {min(c1[0], rx * 16 + 15), min(c1[1], ry * 16 + 15), min(c1[2], rz * 16 + 15)};
        if (visit_cells<MODE>(o, q, in, m, L, (int)uniform(l2), base, s0, s1, lane)) return true;
      }
  return false;
}

__device__ __forceinline__ bool box_meets(const Query& q, f32x4 blo, f32x4 bhi) {
  return q.lo[0] <= bhi.x && blo.x <= q.hi[0] && q.lo[1] <= bhi.y && blo.y <= q.hi[1] && q.lo[2] <= bhi.z && blo.z <= q.hi[2];
}

// the candidates a wave listed in LDS (unique ids), ranked into ascending order and visited
template <int MODE>
__device__ bool visit_listed(ArgsRef a, const OverlapArgs& o, Query& q, uint32_t n_cand, uint32_t lane, OverlapLds& L) {
  wave_sync_lds();
  for (uint32_t j = lane; j < n_cand; j += 64u) {
    const uint32_t v = L.cand[j];
    uint32_t rank = 0;
    for (uint32_t i = 0; i < n_cand; ++i) rank += L.cand[i] < v ? 1u : 0u;
    L.cand[kOverlapCand + rank] = v;
  }
  wave_sync_lds();
  for (uint32_t i = 0; i < n_cand; ++i)
    if (visit_instance<MODE>(a, o, q, uniform(L.cand[kOverlapCand + i]), lane, L)) return true;
  return false;
}

template <int MODE>
__device__ void overlap_query(ArgsRef a, const OverlapArgs& o, uint32_t qi, uint32_t lane, OverlapLds& L) {
  const f32x4* bq = reinterpret_cast<const f32x4*>(o.boxes) + (size_t)qi * 2u;
  const f32x4 b0 = bq[0], b1 = bq[1];
  Query q;
  q.lo[0] = b0.x; q.lo[1] = b0.y; q.lo[2] = b0.z;
  q.hi[0] = b1.x; q.hi[1] = b1.y; q.hi[2] = b1.z;
  q.first = uniform(__float_as_uint(b0.w));
  q.cap = uniform(__float_as_uint(b1.w));
  q.n_records = o.n_records;
  q.total = 0;
  q.any_hit = o.any_hit != 0u;
  q.big = 0.0f;
  bool ok = a.n_instances != 0u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ok = ok && finite(q.lo[k]) && finite(q.hi[k]) && q.lo[k] <= q.hi[k];
    q.big = fmaxf(q.big, fmaxf(fabsf(q.lo[k]), fabsf(q.hi[k])));
  }
  if (ok) {
    bool done = false, listed = false;
    const uint64_t lower = (1ull << lane) - 1ull;
    // (1) the grid: the block of cells the box covers
    const DUST_CONST_AS DevGrid& g = a.grid;
    uint32_t cl[3] = {0, 0, 0}, ch[3] = {0, 0, 0};
    bool use_grid = g.cells != nullptr;
    if (use_grid) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        cl[k] = (uint32_t)f2i_clamp(floorf((q.lo[k] - g.lo[k]) * g.inv_cell[k]), 0, (int)g.dim[k] - 1);
        ch[k] = (uint32_t)f2i_clamp(floorf((q.hi[k] - g.lo[k]) * g.inv_cell[k]), 0, (int)g.dim[k] - 1);
      }
      use_grid = (ch[0] - cl[0] + 1u) * (ch[1] - cl[1] + 1u) * (ch[2] - cl[2] + 1u) <= kOverlapGridCells;
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
              if (keep && at < kOverlapCand) L.cand[at] = ii;
              n_cand += (uint32_t)__popcll(bal);
            }
          }
      if (n_cand <= kOverlapCand) { listed = true; done = visit_listed<MODE>(a, o, q, n_cand, lane, L); }
    } else if (LARGE) {
      // (2) a large scene: the group boxes, then the slots of the groups the box meets
      uint32_t n_cand = 0;
      for (uint32_t s = 0; s < a.n_groups && n_cand <= kOverlapCand; s += 64u) {
        bool meet = false;
        if (s + lane < a.n_groups) {
          const f32x4 glo = *(DUST_RO(f32x4))(&a.gboxes[s + lane].lo[0]), ghi = *(DUST_RO(f32x4))(&a.gboxes[s + lane].hi[0]);
          meet = box_meets(q, glo, ghi);
        }
        uint64_t groups = __ballot(meet);
        while (groups != 0ull && n_cand <= kOverlapCand) {
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
          if (keep && at < kOverlapCand) L.cand[at] = ii;
          n_cand += (uint32_t)__popcll(bal);
        }
      }
      if (n_cand <= kOverlapCand) { listed = true; done = visit_listed<MODE>(a, o, q, n_cand, lane, L); }
    }
    // (3) every instance box in id order, 64 per step (no grid, or a list longer than the LDS takes)
    for (uint32_t s = 0; !listed && !done && s < a.n_instances; s += 64u) {
      bool keep = false;
      if (s + lane < a.n_instances) {
        const f32x4 blo = *(DUST_RO(f32x4))(&a.boxes[s + lane].lo[0]), bhi = *(DUST_RO(f32x4))(&a.boxes[s + lane].hi[0]);
        keep = box_meets(q, blo, bhi);
      }
      uint64_t bal = __ballot(keep);
      while (bal != 0ull && !done) {
        const uint32_t id = s + (uint32_t)__builtin_ctzll(bal);
        bal &= bal - 1ull;
        done = visit_instance<MODE>(a, o, q, id, lane, L);
      }
    }
  }
  if (lane == 0u) o.counts[qi] = q.total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)q.total;
}

}  // namespace

// MODE: bit 1 = DEEP (the scene holds a 4096^3 model), bit 2 = LARGE (more than kFlatCullMax instances: the group boxes exist)
template <int MODE>
__global__ void __launch_bounds__(kOverlapWaves * 64) k_overlap_boxes(const FrameArgs, const OverlapArgs o) {
  ArgsRef a = launch_args();
  if (blockIdx.x == 0 && threadIdx.x == 0) *o.next_counter = 0ull;
  const uint32_t lane = threadIdx.x & 63u;
  OverlapLds& L = g_overlap[threadIdx.x >> 6];
  for (;;) {  // the wave's next chunk of queries
    unsigned long long k = 0;
    if (lane == 0) k = atomicAdd(o.counter, (unsigned long long)kOverlapChunk);
    k = ((unsigned long long)uniform((uint32_t)(k >> 32)) << 32) | uniform((uint32_t)k);
    if (k >= o.n) break;
    const uint32_t end = (uint32_t)min((unsigned long long)o.n, k + kOverlapChunk);
    for (uint32_t qi = (uint32_t)k; qi < end; ++qi) overlap_query<MODE>(a, o, qi, lane, L);
  }
}

// grid, block: the host's choice (capi_scene.cpp overlap_boxes_impl); no dynamic LDS
hipError_t launch_overlap_boxes(const FrameArgs& a, const OverlapArgs& o, uint32_t grid, uint32_t block, hipStream_t s) {
  switch ((a.deep ? 2 : 0) | (a.n_groups ? 4 : 0)) {
    case 0: hipLaunchKernelGGL(k_overlap_boxes<0>, dim3(grid), dim3(block), 0, s, a, o); break;
    case 2: hipLaunchKernelGGL(k_overlap_boxes<2>, dim3(grid), dim3(block), 0, s, a, o); break;
    case 4: hipLaunchKernelGGL(k_overlap_boxes<4>, dim3(grid), dim3(block), 0, s, a, o); break;
    default: hipLaunchKernelGGL(k_overlap_boxes<6>, dim3(grid), dim3(block), 0, s, a, o); break;
  }
  return hipGetLastError();
}

}  // namespace dust
