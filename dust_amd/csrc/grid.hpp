// grid.hpp -- the dense voxel grid of an editable 256^3 model (EditArgs::grid) and every per-voxel array laid out like it, in one
// place: a 4^3 brick is 64 consecutive entries, entry leaf_code(bx, by, bz) * 64 + bit with bit = (x&3)<<4 | (y&3)<<2 | (z&3), so a
// wavefront per brick has lane = voxel bit. 64 consecutive bricks are one root cell (16^3 voxels, cell = code >> 6).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dust {

constexpr uint32_t kLattice = 64 * 64 * 64;  // bricks of a 256^3 model

// brick code in Tree::iter_leaf order: root child index (x>>4)<<8 | (y>>4)<<4 | (z>>4) (node/internal.rs:78-81), then the
// mid node's child bit ((x>>2)&3)<<4 | ((y>>2)&3)<<2 | ((z>>2)&3); bx, by, bz are brick coordinates (voxel >> 2)
__device__ __forceinline__ uint32_t leaf_code(uint32_t bx, uint32_t by, uint32_t bz) {
  return ((((bx >> 2) << 8) | ((by >> 2) << 4) | (bz >> 2)) << 6) | ((bx & 3u) << 4) | ((by & 3u) << 2) | (bz & 3u);
}
// brick c (the mid node's child bit, 0..63) of root cell `cell`: code cell * 64 + c
__device__ __forceinline__ void cell_brick(uint32_t cell, uint32_t c, uint32_t& bx, uint32_t& by, uint32_t& bz) {
  bx = ((cell >> 8) << 2) | (c >> 4);
  by = (((cell >> 4) & 15u) << 2) | ((c >> 2) & 3u);
  bz = ((cell & 15u) << 2) | (c & 3u);
}
__device__ __forceinline__ void leaf_decode(uint32_t code, uint32_t& bx, uint32_t& by, uint32_t& bz) {
  const uint32_t r = code >> 6, c = code & 63u;
  bx = ((r >> 8) << 2) | (c >> 4);
  by = (((r >> 4) & 15u) << 2) | ((c >> 2) & 3u);
  bz = ((r & 15u) << 2) | (c & 3u);
}

__device__ __forceinline__ uint32_t voxel_bit(uint32_t x, uint32_t y, uint32_t z) { return ((x & 3u) << 4) | ((y & 3u) << 2) | (z & 3u); }
// where voxel (x, y, z) lies in the grid and in a field
__device__ __forceinline__ uint32_t voxel_index(uint32_t x, uint32_t y, uint32_t z) { return leaf_code(x >> 2, y >> 2, z >> 2) * 64u + voxel_bit(x, y, z); }

// voxel `bit` of brick (bx, by, bz) / of brick `code`: its coordinates, and its PUBLIC key x << 16 | y << 8 | z
struct Voxel {
  uint32_t x, y, z;
  __device__ __forceinline__ uint32_t key() const { return (x << 16) | (y << 8) | z; }
};
__device__ __forceinline__ Voxel brick_voxel(uint32_t bx, uint32_t by, uint32_t bz, uint32_t bit) {
  return {bx * 4u + (bit >> 4), by * 4u + ((bit >> 2) & 3u), bz * 4u + (bit & 3u)};
}
__device__ __forceinline__ Voxel code_voxel(uint32_t code, uint32_t bit) {
  uint32_t bx, by, bz;
  leaf_decode(code, bx, by, bz);
  return brick_voxel(bx, by, bz, bit);
}
__device__ __forceinline__ uint32_t voxel_key(uint32_t bx, uint32_t by, uint32_t bz, uint32_t bit) { return brick_voxel(bx, by, bz, bit).key(); }

// an inclusive box of root cells (coordinates 0..15), walked x-major by the kernels that take a workgroup per cell
struct CellBox {
  uint32_t lo[3], hi[3];
  __host__ __device__ uint32_t count() const { return (hi[0] - lo[0] + 1u) * (hi[1] - lo[1] + 1u) * (hi[2] - lo[2] + 1u); }
  __device__ __forceinline__ uint32_t cell(uint32_t i) const {  // the root cell (x << 8 | y << 4 | z) of workgroup i < count()
    const uint32_t ny = hi[1] - lo[1] + 1u, nz = hi[2] - lo[2] + 1u;
    return ((lo[0] + i / (ny * nz)) << 8) | ((lo[1] + (i / nz) % ny) << 4) | (lo[2] + i % nz);
  }
};

__host__ __device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }  // v is the same in every lane: keep it in an SGPR
__device__ __forceinline__ uint64_t uniform64(uint64_t v) { return ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v); }
#endif

}  // namespace dust
