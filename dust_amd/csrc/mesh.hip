// mesh.hip -- model meshes (dust_hip_model_mesh): the exposed faces of a model's solid voxels, per direction, merged into axis-aligned
// rectangles under the canonical rule of mesh_rule.hpp, counted and listed on the device. One workgroup of 256 threads per
// (direction d, slice of d's normal axis): kMeshSlices = 1 536 workgroups. A workgroup
//   1. builds the slice's F plane from the brick masks (EditArgs::brick_mask, 2 MiB): a thread takes 8 bricks along u and writes one
//      word of four rows; exposure is mesh_exposure (surface_rule.hpp's E_d) of the brick's word and, on the brick's boundary plane
//      only, the word of the brick across d. The grid is read here only under a palette filter. A slice whose F is empty ends
//      there, on a workgroup-uniform branch (__syncthreads_or, which every thread reaches);
//   2. fills J and K, a thread per word: under ANY_PALETTE from F alone, otherwise from the grid bytes of the voxels in F that have a
//      neighbour in F before them or above them, four voxels along u to a load;
//   3. turns K into C, the run starts that continue the row above, a thread per row (mesh_continued_word);
//   4. walks the run starts that continue nothing, a thread per row (mesh_row_quads): a height is a walk down one bit column of C.
// The planes are rows of 8 words padded to 9 in LDS (27 KiB): with a thread per row an odd stride puts the 32 lanes of a half-wave on
// 32 different banks.
//   k_mesh_count  folds quads, area and the largest area through three LDS words; thread 0 writes the slice's quad count into a kLattice
//                 table (where not 0) and issues at most three ordinary vector atomics (two adds, one maximum).
//   k_mesh_list   after launch_table_scan over that table: builds the planes again; a quad's rank is the slice's offset, plus the
//                 block_scan_inclusive of the quads per row before its row, plus the quads before it in its row; it writes its
//                 8-byte record as one store when the rank is below the capacity. A slice whose offset is at or past the capacity
//                 ends before it builds anything.
// Everything is integer: no order shows in any result. No fences, spins or waits BETWEEN workgroups, ordinary vector stores.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "mesh.hpp"
#include "mesh_rule.hpp"
#include "scan.hpp"

namespace dust {

namespace {

constexpr uint32_t kStride = kMeshRowWords + 1u;         // words from row to row in LDS
constexpr uint32_t kPlaneWords = kMeshExtent * kStride;  // 2 304 words, 9 KiB a plane

// this workgroup's direction and slice, or false: the query does not look at it (uniform)
__device__ __forceinline__ bool mesh_slice(const MeshArgs& a, uint32_t& d, uint32_t& s) {
  d = blockIdx.x >> 8;
  s = blockIdx.x & 255u;
  const uint32_t n = d >> 1;
  return ((a.faces >> d) & 1u) && s >= a.lo[n] && s <= a.hi[n];
}

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

// F, J and C of slice s of direction d into LDS (C where K was); false: F is empty (uniform, and the planes are not complete)
__device__ __forceinline__ bool build_planes(const MeshArgs& a, uint32_t d, uint32_t s, uint32_t* F, uint32_t* J, uint32_t* K) {
  const uint32_t n = d >> 1, c = s & 3u, bs = s >> 2;
  const uint64_t plane = mesh_slice_plane(n, c);
  const bool edge = (d & 1u) ? c == 3u : c == 0u;           // the slice is its bricks' boundary plane towards d
  const uint32_t across_bs = (d & 1u) ? bs + 1u : bs - 1u;  // (-1 and 64 are above 63: off the tree)
  const uint64_t outside = a.walls ? ~0ull : 0ull;
  uint32_t any = 0;
  for (uint32_t task = threadIdx.x; task < 64u * kMeshRowWords; task += 256u) {
    const uint32_t bv = task >> 3, w = task & 7u;
    uint32_t f0 = 0, f1 = 0, f2 = 0, f3 = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
      const uint32_t bu = w * 8u + k;
      const uint32_t bx = mesh_x(n, bs, bu, bv), by = mesh_y(n, bs, bu, bv), bz = mesh_z(n, bs, bu, bv);
      const uint32_t code = leaf_code(bx, by, bz);
      const uint64_t own = a.brick_mask[code];
      if ((own & plane) == 0ull) continue;
      uint64_t across = 0ull;
      if (edge)
        across = across_bs > 63u ? outside : a.brick_mask[leaf_code(mesh_x(n, across_bs, bu, bv), mesh_y(n, across_bs, bu, bv), mesh_z(n, across_bs, bu, bv))];
      uint64_t e = mesh_exposure(own, across, d) & plane & surface_region_mask(bx, by, bz, a.lo, a.hi);
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
    if (!a.any_palette && (jw | kw) != 0u) {                                           // ... of them, those whose bytes agree
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

}  // namespace

__global__ void __launch_bounds__(256) k_mesh_count(MeshArgs a) {
  __shared__ uint32_t F[kPlaneWords], J[kPlaneWords], K[kPlaneWords];
  __shared__ uint32_t fold[3];  // the slice's quads, their area, the largest
  uint32_t d, s;
  if (!mesh_slice(a, d, s)) return;
  if (threadIdx.x < 3u) fold[threadIdx.x] = 0u;  // (the barriers of build_planes lie between this and the adds)
  if (!build_planes(a, d, s, F, J, K)) return;
  const uint32_t v = threadIdx.x;
  uint32_t area = 0, largest = 0;
  const uint32_t quads = mesh_row_quads(F, J, K, kStride, v, true, [&](uint32_t u0, uint32_t u1, uint32_t v1) {
    const uint32_t q = (u1 - u0 + 1u) * (v1 - v + 1u);
    area += q;
    largest = umax(largest, q);
  });
  if (quads != 0u) {
    atomicAdd(&fold[0], quads);
    atomicAdd(&fold[1], area);
    atomicMax(&fold[2], largest);
  }
  __syncthreads();
  if (threadIdx.x == 0u && fold[0] != 0u) {
    if (a.slice_count) a.slice_count[blockIdx.x] = fold[0];
    atomicAdd(&a.acc[d], fold[0]);
    atomicAdd(&a.acc[kSurfaceFaces + d], fold[1]);
    atomicMax(&a.acc[2u * kSurfaceFaces], fold[2]);
  }
}

__global__ void __launch_bounds__(256) k_mesh_list(MeshArgs a) {
  __shared__ uint32_t F[kPlaneWords], J[kPlaneWords], K[kPlaneWords];
  __shared__ uint32_t scan[256];
  uint32_t d, s;
  if (!mesh_slice(a, d, s)) return;
  const uint32_t first = a.slice_count[blockIdx.x] + a.scan_tmp[blockIdx.x >> 10];  // exclusive scans: local + block base (uniform)
  if (first >= a.capacity) return;                                                   // (the later slices come later in the list)
  if (!build_planes(a, d, s, F, J, K)) return;
  const uint32_t v = threadIdx.x, n = d >> 1;
  const uint32_t quads = mesh_row_quads(F, J, K, kStride, v, false, [](uint32_t, uint32_t, uint32_t) {});
  uint32_t rank = first + block_scan_inclusive<256>(scan, quads) - quads;
  if (quads == 0u || rank >= a.capacity) return;  // (no barrier follows)
  mesh_row_quads(F, J, K, kStride, v, true, [&](uint32_t u0, uint32_t u1, uint32_t v1) {
    if (rank < a.capacity) a.quads[rank] = mesh_record(d, s, u0, u1, v, v1, a.grid[slice_voxel(n, s, u0, v)] - 1u);
    ++rank;
  });
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_mesh_count(const MeshArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mesh_count, dim3(kMeshSlices), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_mesh_list(const MeshArgs& a, hipStream_t s) {
  if (a.capacity) hipLaunchKernelGGL(k_mesh_list, dim3(kMeshSlices), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
