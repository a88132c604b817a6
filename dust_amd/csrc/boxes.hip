// boxes.hip -- model boxes (dust_hip_model_boxes): the solid voxels of a model merged into axis-aligned boxes under the canonical rule
// of boxes_rule.hpp -- runs along u, rects of identical runs along v (mesh_rule.hpp's quads with F = S), boxes of identical rects along
// the stacking axis n -- counted and listed on the device. One workgroup of 256 threads per slice of n: kBoxesSlices = 256 workgroups.
//   k_boxes_count  builds F, J and C of its slice s as mesh.hip does, with F = S: the brick's word, the slice's plane and
//                  surface_region_mask, no exposure term and no neighbour brick; grid bytes are read only under a filter and where two
//                  voxels might join, four to a load. Where s is not the region's first slice and neither slice is empty it builds the
//                  planes of slice s - 1 beside them (two sets of 3 x 9 KiB of LDS) and forms D, a thread per row
//                  (boxes_continued_word). EVERY slice of the region writes its whole D plane into the D volume, an empty slice and the
//                  region's first slice all clear: the volume is reused between calls and models, and a depth walk that arrives from the
//                  slice before must not read what an earlier call left. It folds rects, continued rects, popcount(F) and the bounds
//                  through LDS; thread 0 writes the slice's box starts (rects - continued) into a kLattice table (where not 0) and
//                  issues at most nine ordinary vector atomics.
//   k_boxes_list   after launch_table_scan over that table: builds F, J, C again and reads its D words back; a box start is a rect
//                  start whose D bit is clear; its rank is the slice's offset, plus the block_scan_inclusive of the starts per row
//                  before its row, plus the starts before it in its row. For every start below the capacity it walks u1 along J, v1
//                  down C and the depth through the D planes of the following slices up to hi[n] (single-word loads), and writes the
//                  8-byte record as one store. A slice whose offset is at or past the capacity ends before it builds anything.
// The slice builder is mesh.hip's with another F; mesh.hip itself is left as it is, so that its kernels keep their registers.
// Everything is integer: no order shows in any result. No fences, spins or waits BETWEEN workgroups (the list pass is a launch of its
// own behind the count pass and the scan), ordinary vector loads, stores and atomics.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "boxes.hpp"
#include "boxes_rule.hpp"
#include "scan.hpp"

namespace dust {

namespace {

constexpr uint32_t kStride = kMeshRowWords + 1u;         // words from row to row in LDS: odd, a thread per row hits 32 banks
constexpr uint32_t kPlaneWords = kMeshExtent * kStride;  // 2 304 words, 9 KiB a plane

__device__ __forceinline__ uint32_t slice_voxel(uint32_t n, uint32_t s, uint32_t u, uint32_t v) {
  return voxel_index(mesh_x(n, s, u, v), mesh_y(n, s, u, v), mesh_z(n, s, u, v));
}

// the grid bytes of the four voxels u4 .. u4 + 3 (u4 a multiple of 4) of row v, byte i the voxel at u4 + i: along z they are four
// consecutive bytes of a brick; along y (n = z) the brick's 16 bytes of one x hold them at a stride of 4
__device__ __forceinline__ uint32_t slice_bytes4(const uint8_t* grid, uint32_t n, uint32_t s, uint32_t u4, uint32_t v) {
  const uint32_t at = slice_voxel(n, s, u4, v);
  if (n != 2u) return *reinterpret_cast<const uint32_t*>(grid + at);  // (z & 3 == 0: aligned)
  const uint4 q = *reinterpret_cast<const uint4*>(grid + (at & ~15u));  // y = 0..3 (one word each) x z = 0..3
  const uint32_t shift = 8u * (s & 3u);
  return ((q.x >> shift) & 255u) | (((q.y >> shift) & 255u) << 8) | (((q.z >> shift) & 255u) << 16) | (((q.w >> shift) & 255u) << 24);
}

// F, J and C of slice s into LDS (C where K was); false: F is empty (uniform, and the planes are not complete). `free_joins`: two
// neighbours in F always join -- ANY_PALETTE, or a filter, under which every voxel of F holds the same byte
__device__ __forceinline__ bool build_planes(const BoxesArgs& a, uint32_t s, bool free_joins, uint32_t* F, uint32_t* J, uint32_t* K) {
  const uint32_t n = a.axis, c = s & 3u, bs = s >> 2;
  const uint64_t plane = mesh_slice_plane(n, c);
  uint32_t any = 0;
  for (uint32_t task = threadIdx.x; task < 64u * kMeshRowWords; task += 256u) {
    const uint32_t bv = task >> 3, w = task & 7u;
    uint32_t f0 = 0, f1 = 0, f2 = 0, f3 = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
      const uint32_t bu = w * 8u + k;
      const uint32_t bx = mesh_x(n, bs, bu, bv), by = mesh_y(n, bs, bu, bv), bz = mesh_z(n, bs, bu, bv);
      const uint32_t code = leaf_code(bx, by, bz);
      uint64_t e = a.brick_mask[code] & plane;
      if (e == 0ull) continue;
      e &= surface_region_mask(bx, by, bz, a.lo, a.hi);
      if (a.byte != 0u)  // (the host passes a grid whenever there is a filter)
        for (uint64_t rest = e; rest != 0ull; rest &= rest - 1ull) {
          const uint32_t bit = (uint32_t)__builtin_ctzll(rest);
          if (a.grid[(size_t)code * 64u + bit] != a.byte) e &= ~(1ull << bit);
        }
      f0 |= mesh_row_nibble(e, n, c, 0u) << (4u * k);
      f1 |= mesh_row_nibble(e, n, c, 1u) << (4u * k);
      f2 |= mesh_row_nibble(e, n, c, 2u) << (4u * k);
      f3 |= mesh_row_nibble(e, n, c, 3u) << (4u * k);
    }
    uint32_t* f = F + bv * 4u * kStride + w;
    f[0] = f0; f[kStride] = f1; f[2u * kStride] = f2; f[3u * kStride] = f3;
    any |= f0 | f1 | f2 | f3;
  }
  if (!__syncthreads_or((int)(any != 0u))) return false;
  for (uint32_t task = threadIdx.x; task < kMeshExtent * kMeshRowWords; task += 256u) {
    const uint32_t row = task >> 3, w = task & 7u;
    const uint32_t* f_row = F + row * kStride;
    const uint32_t f = f_row[w];
    uint32_t jw = mesh_join_any(f_row, w), kw = row ? f & (f_row - kStride)[w] : 0u;  // the candidates: both voxels are in F
    if (!free_joins && (jw | kw) != 0u) {                                              // ... of them, those whose bytes agree
      // the bytes of four voxels along u at a time; a brick is loaded when it holds a candidate or the voxel before the next one's
      uint32_t before = (w != 0u && (jw & 1u)) ? slice_bytes4(a.grid, n, s, (w << 5) - 4u, row) >> 24 : 0u;
      uint32_t j_same = 0, k_same = 0;
#pragma unroll
      for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t j4 = (jw >> (4u * k)) & 15u, k4 = (kw >> (4u * k)) & 15u, next = k < 7u ? (jw >> (4u * k + 4u)) & 1u : 0u;
        uint32_t own4 = 0, up4 = 0;
        if ((j4 | k4 | next) != 0u) own4 = slice_bytes4(a.grid, n, s, (w << 5) + 4u * k, row);
        if (k4 != 0u) up4 = slice_bytes4(a.grid, n, s, (w << 5) + 4u * k, row - 1u);
        const uint32_t left4 = (own4 << 8) | before;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
          const uint32_t g = (own4 >> (8u * i)) & 255u;
          j_same |= (uint32_t)(g == ((left4 >> (8u * i)) & 255u)) << (4u * k + i);
          k_same |= (uint32_t)(g == ((up4 >> (8u * i)) & 255u)) << (4u * k + i);
        }
        before = own4 >> 24;
      }
      jw &= j_same;
      kw &= k_same;
    }
    J[row * kStride + w] = jw;
    K[row * kStride + w] = kw;
  }
  __syncthreads();
  // C over K, a thread per row: only this thread reads or writes the row's K words, and F and J stay as they are
  {
    const uint32_t v = threadIdx.x;
    const uint32_t* f_row = F + v * kStride;
    const uint32_t* j_row = J + v * kStride;
    uint32_t* k_row = K + v * kStride;
    for (uint32_t w = 0; w < kMeshRowWords; ++w) k_row[w] = v ? mesh_continued_word(f_row, j_row, k_row, f_row - kStride, j_row - kStride, w) : 0u;
  }
  __syncthreads();
  return true;
}

// this workgroup's slice, or false: outside the region (uniform)
__device__ __forceinline__ bool boxes_slice(const BoxesArgs& a, uint32_t& s) {
  s = blockIdx.x;
  return s >= a.lo[a.axis] && s <= a.hi[a.axis];
}

}  // namespace

__global__ void __launch_bounds__(256) k_boxes_count(BoxesArgs a) {
  __shared__ uint32_t F[kPlaneWords], J[kPlaneWords], K[kPlaneWords];     // slice s
  __shared__ uint32_t PF[kPlaneWords], PJ[kPlaneWords], PK[kPlaneWords];  // slice s - 1
  __shared__ uint32_t fold[kBoxesAccWords];  // the slice's share of the accumulator, bounds along (n, u, v) at 3.. and 6..
  uint32_t s;
  if (!boxes_slice(a, s)) return;
  const uint32_t n = a.axis, v = threadIdx.x;
  const bool free_joins = a.any_palette != 0u || a.byte != 0u;
  uint32_t* d_row = a.dvol + size_t(s) * kBoxesPlaneWords + v * kMeshRowWords;  // (s < 256, v < 256: inside the 2 MiB)
  if (threadIdx.x < kBoxesAccWords) fold[threadIdx.x] = 0u;  // (the barriers of build_planes lie between this and the adds)
  if (!build_planes(a, s, free_joins, F, J, K)) {
    for (uint32_t w = 0; w < kMeshRowWords; ++w) d_row[w] = 0u;  // an empty slice stops every walk that reaches it
    return;
  }
  const bool stacked = s > a.lo[n] && build_planes(a, s - 1u, free_joins, PF, PJ, PK);  // (uniform)
  uint32_t rects = 0, continued = 0, voxels = 0, first = kMeshExtent, last = 0;
  for (uint32_t w = 0; w < kMeshRowWords; ++w) {
    const uint32_t f = F[v * kStride + w];
    uint32_t d = 0;
    if (stacked)
      d = boxes_continued_word(F, J, K, PF, PJ, PK, kStride, v, w, [&](uint32_t u0) {
        return free_joins || a.grid[slice_voxel(n, s, u0, v)] == a.grid[slice_voxel(n, s - 1u, u0, v)];
      });
    d_row[w] = d;
    rects += (uint32_t)__builtin_popcount(f & ~J[v * kStride + w] & ~K[v * kStride + w]);
    continued += (uint32_t)__builtin_popcount(d);
    voxels += (uint32_t)__builtin_popcount(f);
    if (f != 0u) {
      if (first == kMeshExtent) first = (w << 5) + mesh_ctz(f);
      last = (w << 5) + 31u - (uint32_t)__builtin_clz(f);
    }
  }
  if (voxels != 0u) {
    if (rects != 0u) atomicAdd(&fold[0], rects);
    if (continued != 0u) atomicAdd(&fold[1], continued);
    atomicAdd(&fold[2], voxels);
    atomicMax(&fold[4], 255u - first);
    atomicMax(&fold[7], last);
    atomicMax(&fold[5], 255u - v);
    atomicMax(&fold[8], v);
  }
  __syncthreads();
  if (threadIdx.x == 0u) {  // (F is not empty: the slice holds a voxel, so a rect)
    const uint32_t axis_u = n == 2u ? 1u : 2u, axis_v = n == 0u ? 1u : 0u;
    if (a.slice_count && fold[0] != fold[1]) a.slice_count[s] = fold[0] - fold[1];
    atomicAdd(&a.acc[0], fold[0]);
    if (fold[1] != 0u) atomicAdd(&a.acc[1], fold[1]);
    atomicAdd(&a.acc[2], fold[2]);
    atomicMax(&a.acc[3u + n], 255u - s);
    atomicMax(&a.acc[6u + n], s);
    atomicMax(&a.acc[3u + axis_u], fold[4]);
    atomicMax(&a.acc[6u + axis_u], fold[7]);
    atomicMax(&a.acc[3u + axis_v], fold[5]);
    atomicMax(&a.acc[6u + axis_v], fold[8]);
  }
}

__global__ void __launch_bounds__(256) k_boxes_list(BoxesArgs a) {
  __shared__ uint32_t F[kPlaneWords], J[kPlaneWords], K[kPlaneWords];
  __shared__ uint32_t scan[256];
  uint32_t s;
  if (!boxes_slice(a, s)) return;
  const uint32_t first = a.slice_count[s] + a.scan_tmp[s >> 10];  // exclusive scans: local + block base (uniform)
  if (first >= a.capacity) return;                                // (the later slices come later in the list)
  if (!build_planes(a, s, a.any_palette != 0u || a.byte != 0u, F, J, K)) return;
  const uint32_t n = a.axis, v = threadIdx.x;
  const uint32_t* d_row = a.dvol + size_t(s) * kBoxesPlaneWords + v * kMeshRowWords;
  uint32_t starts = 0;
  for (uint32_t w = 0; w < kMeshRowWords; ++w) starts += (uint32_t)__builtin_popcount(F[v * kStride + w] & ~J[v * kStride + w] & ~K[v * kStride + w] & ~d_row[w]);
  uint32_t rank = first + block_scan_inclusive<256>(scan, starts) - starts;
  if (starts == 0u || rank >= a.capacity) return;  // (no barrier follows)
  for (uint32_t w = 0; w < kMeshRowWords; ++w)
    for (uint32_t rest = F[v * kStride + w] & ~J[v * kStride + w] & ~K[v * kStride + w] & ~d_row[w]; rest != 0u; rest &= rest - 1u) {
      if (rank >= a.capacity) return;
      const uint32_t u0 = (w << 5) + mesh_ctz(rest);
      const uint32_t u1 = mesh_run_end(J + v * kStride, u0), v1 = boxes_rect_end(K, kStride, v, u0);
      const uint32_t depth = boxes_depth(a.dvol, s, a.hi[n], v, u0);
      a.boxes[rank++] = boxes_record(n, s, u0, u1, v, v1, depth, a.grid[slice_voxel(n, s, u0, v)] - 1u);
    }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_boxes_count(const BoxesArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_boxes_count, dim3(kBoxesSlices), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_boxes_list(const BoxesArgs& a, hipStream_t s) {
  if (a.capacity) hipLaunchKernelGGL(k_boxes_list, dim3(kBoxesSlices), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
