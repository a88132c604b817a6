// surface_rule.hpp -- the device-free half of the model surfaces (dust_hip_model_surface, _surface_apply): which faces of a 4^3 brick's
// voxels are exposed, as ONE function of seven 64-bit words -- the brick's occupancy and its six neighbours'. Bit x<<4 | y<<2 | z of a
// word is voxel (x, y, z) of the brick (grid.hpp voxel_bit; EditArgs::brick_mask). Integer work over values: no HIP call, no memory
// access, no array indexed by a runtime value. surface.hip calls it per brick, where every word is wave-uniform (scalar work);
// tests/cpp/surface_rule_test.cpp runs the same text on a CPU (tests/test_surface_rule.py).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define DUST_SURFACE_FN __host__ __device__ __forceinline__
#else
#define DUST_SURFACE_FN inline
#endif

namespace dust {

// directions, in the order of the DUST_HIP_FACE_* bits: -x, +x, -y, +y, -z, +z
constexpr uint32_t kSurfaceFaces = 6;
// the planes of a brick word: voxels with x == 0 / 3, y == 0 / 3, z == 0 / 3
constexpr uint64_t kSurfaceX0 = 0x000000000000FFFFull, kSurfaceX3 = 0xFFFF000000000000ull;
constexpr uint64_t kSurfaceY0 = 0x000F000F000F000Full, kSurfaceY3 = 0xF000F000F000F000ull;
constexpr uint64_t kSurfaceZ0 = 0x1111111111111111ull, kSurfaceZ3 = 0x8888888888888888ull;

struct SurfaceWords {
  uint64_t e[kSurfaceFaces];  // e[d] bit v: voxel v is solid and the voxel across its face d is empty
};

// own: the brick's word; nx, px, ny, py, nz, pz: the words of the bricks across its -x, +x, -y, +y, -z, +z faces (a neighbour off the
// tree: 0, or all ones when the outside of the tree counts as solid). N_d, the occupancy of every voxel's neighbour across d, is the
// brick's own word moved by one voxel along d (1, 4 or 16 bits) with the neighbour's facing plane moved in on the boundary plane;
// E_d = own & ~N_d.
DUST_SURFACE_FN SurfaceWords surface_exposure(uint64_t own, uint64_t nx, uint64_t px, uint64_t ny, uint64_t py, uint64_t nz, uint64_t pz) {
  SurfaceWords w;
  w.e[0] = own & ~((own << 16) | (nx >> 48));                                 // (the shift itself clears the x == 0 plane)
  w.e[1] = own & ~((own >> 16) | (px << 48));
  w.e[2] = own & ~(((own << 4) & ~kSurfaceY0) | ((ny >> 12) & kSurfaceY0));
  w.e[3] = own & ~(((own >> 4) & ~kSurfaceY3) | ((py << 12) & kSurfaceY3));
  w.e[4] = own & ~(((own << 1) & ~kSurfaceZ0) | ((nz >> 3) & kSurfaceZ0));
  w.e[5] = own & ~(((own >> 1) & ~kSurfaceZ3) | ((pz << 3) & kSurfaceZ3));
  return w;
}

// the voxels of brick coordinate b (voxels 4 b .. 4 b + 3 on the axis) that lie in lo..hi on an axis whose plane c == 0 is `plane0`
// and whose coordinate moves a bit by `shift`: the part of an inclusive region a brick holds is the AND of the three
DUST_SURFACE_FN uint64_t surface_axis_mask(uint32_t b, uint32_t lo, uint32_t hi, uint64_t plane0, uint32_t shift) {
  uint64_t m = 0;
#pragma unroll
  for (uint32_t c = 0; c < 4u; ++c)
    if (b * 4u + c >= lo && b * 4u + c <= hi) m |= plane0 << (shift * c);
  return m;
}
DUST_SURFACE_FN uint64_t surface_region_mask(uint32_t bx, uint32_t by, uint32_t bz, const uint32_t lo[3], const uint32_t hi[3]) {
  return surface_axis_mask(bx, lo[0], hi[0], kSurfaceX0, 16u) & surface_axis_mask(by, lo[1], hi[1], kSurfaceY0, 4u) &
         surface_axis_mask(bz, lo[2], hi[2], kSurfaceZ0, 1u);
}

}  // namespace dust
