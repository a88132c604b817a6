// flood.hip -- step distances through the empty or the solid voxels of an editable hierarchy!(4,2,2) model (dust_hip_model_flood,
// dust_hip_model_flood_at, dust_hip_model_flood_paths, dust_hip_model_flood_apply; the contract is in include/dust_hip.h).
//
// The field is a uint16 per voxel, brick-major like the grid (edit.hpp EditArgs::grid): a 4^3 brick is 128 contiguous bytes and one
// wavefront, lane = voxel bit x << 4 | y << 2 | z. steps(v) is the fixed point of v = min(v, min(passable face neighbours) + 1) with the
// seeds at 0, capped at max_steps; it is reached by chaotic relaxation, brick by brick:
//   k_flood_seed    a thread per seed: a passable seed inside the region takes 0 and puts its brick on the first worklist
//   k_flood_relax   one PASS: a wavefront per listed brick. The lane holds its voxel's value; the facing voxels of the six neighbour bricks
//                   are read from global memory once; the brick is then relaxed to ITS fixed point in registers (the six in-brick
//                   neighbours come by cross-lane moves, at most 64 rounds: a shortest path inside a brick has at most 63 edges). A brick
//                   that changed is written back, and for every face on which some lane's value dropped below what the facing voxel
//                   could make of its own the neighbour brick is put on the NEXT pass's worklist (a flag per brick keeps it there once; the list's length is one atomic counter)
//   k_flood_result  a workgroup per root cell of the region: count, maximum, zeros, region-face count and bounds of the reached voxels
//   k_flood_paths   a thread per start, descending the field  (dust_hip_model_flood_at and _flood_apply: field.hip)
// A pass is one launch; the host launches passes until one leaves an empty worklist (capi_model.cpp). An empty pass exits at once, and
// work per pass follows the listed bricks, not the lattice.
//
// DO NOT ADD FENCES OR WAITS. Correctness rests on visibility at kernel boundaries alone. Inside a pass a brick may read a neighbour's
// face while that neighbour is being relaxed: it then sees the old value or the new one (an aligned 16-bit store does not tear), both are
// lengths of real paths, i.e. upper bounds, and values only ever decrease. If it saw the old one, the writer's value dropped on that
// face, so the writer puts the reader on the next pass's list, and that pass starts with everything this one wrote visible. The field is
// therefore the unique fixed point whatever the scheduling: two runs give the same bytes. Nothing spins, no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "edit.hpp"
#include "field.hpp"
#include "flood.hpp"

namespace dust {

namespace {

constexpr uint32_t kEmptyMedium = 0, kSolidMedium = 1;  // DUST_HIP_FLOOD_EMPTY, _SOLID (2: _MATERIAL)

__device__ __forceinline__ bool passable(const FloodArgs& a, uint32_t g, uint32_t x, uint32_t y, uint32_t z) {
  const bool medium = a.medium == kEmptyMedium ? g == 0u : a.medium == kSolidMedium ? g != 0u : g == a.byte;
  return medium && x >= a.lo[0] && x <= a.hi[0] && y >= a.lo[1] && y <= a.hi[1] && z >= a.lo[2] && z <= a.hi[2];
}
// the root cells the region reaches
__host__ __device__ inline CellBox region_cells(const FloodArgs& a) {
  return {{a.lo[0] >> 4, a.lo[1] >> 4, a.lo[2] >> 4}, {a.hi[0] >> 4, a.hi[1] >> 4, a.hi[2] >> 4}};
}
// put brick `code` on a worklist unless it is there already (at most kLattice entries: one per flag)
__device__ __forceinline__ void wake(uint32_t* flag, uint32_t* list, uint32_t* count, uint32_t code) {
  if (atomicExch(flag + code, 1u) == 0u) list[atomicAdd(count, 1u)] = code;
}

}  // namespace

__global__ void __launch_bounds__(256) k_flood_seed(FloodArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n_seeds) return;
  const uint32_t x = a.seeds[i * 3], y = a.seeds[i * 3 + 1], z = a.seeds[i * 3 + 2];  // (the host has checked the coordinates)
  const uint32_t at = voxel_index(x, y, z);
  if (!passable(a, a.grid[at], x, y, z)) return;
  a.field[at] = 0;
  wake(a.next_flag, a.next_list, a.next_count, at >> 6);
}

__global__ void __launch_bounds__(256) k_flood_relax(FloodArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
  const uint32_t n_waves = gridDim.x * 4u;
  if (wave == 0u && lane == 0u) *a.zero_count = 0u;  // (nobody reads or appends to that one during this pass)
  const uint32_t n = *a.count;
  const Voxel in_brick = brick_voxel(0u, 0u, 0u, lane);
  const uint32_t lx = in_brick.x, ly = in_brick.y, lz = in_brick.z;
  for (uint32_t i = wave; i < n; i += n_waves) {
    const uint32_t code = uniform(a.list[i]);
    if (lane == 0u) a.flag[code] = 0u;  // (this pass wakes bricks on the OTHER flag array)
    uint32_t bx, by, bz;
    leaf_decode(code, bx, by, bz);
    const size_t at = (size_t)code * 64u + lane;
    const Voxel p = brick_voxel(bx, by, bz, lane);
    const bool open = passable(a, a.grid[at], p.x, p.y, p.z);
    const uint32_t v0 = open ? (uint32_t)a.field[at] : kFieldNone;
    // the facing voxels of the neighbour bricks, once (a stale value is harmless: see the head of the file). An impassable voxel holds
    // kFieldNone, so its passability need not be looked at
    uint32_t ext_x = kFieldNone, ext_y = kFieldNone, ext_z = kFieldNone;  // (a lane has at most one such neighbour per axis)
    if (open) {
      if (lx == 0u && bx > 0u) ext_x = a.field[(size_t)leaf_code(bx - 1u, by, bz) * 64u + lane + 48u];
      if (lx == 3u && bx < 63u) ext_x = a.field[(size_t)leaf_code(bx + 1u, by, bz) * 64u + lane - 48u];
      if (ly == 0u && by > 0u) ext_y = a.field[(size_t)leaf_code(bx, by - 1u, bz) * 64u + lane + 12u];
      if (ly == 3u && by < 63u) ext_y = a.field[(size_t)leaf_code(bx, by + 1u, bz) * 64u + lane - 12u];
      if (lz == 0u && bz > 0u) ext_z = a.field[(size_t)leaf_code(bx, by, bz - 1u) * 64u + lane + 3u];
      if (lz == 3u && bz < 63u) ext_z = a.field[(size_t)leaf_code(bx, by, bz + 1u) * 64u + lane - 3u];
    }
    const uint32_t ext = umin(ext_x, umin(ext_y, ext_z));
    uint32_t v = v0;
    if (open && ext + 1u <= a.max_steps) v = umin(v, ext + 1u);  // (kFieldNone + 1 is above every max_steps)
    // an entry from outside and at most 63 edges inside: after 63 rounds every lane is final, the 64th only confirms it
    for (int round = 0; round < 64; ++round) {
      uint32_t m = kFieldNone;
      const uint32_t zm = (uint32_t)__shfl((int)v, (int)((lane - 1u) & 63u)), zp = (uint32_t)__shfl((int)v, (int)((lane + 1u) & 63u));
      const uint32_t ym = (uint32_t)__shfl((int)v, (int)((lane - 4u) & 63u)), yp = (uint32_t)__shfl((int)v, (int)((lane + 4u) & 63u));
      const uint32_t xm = (uint32_t)__shfl((int)v, (int)((lane - 16u) & 63u)), xp = (uint32_t)__shfl((int)v, (int)((lane + 16u) & 63u));
      if (lz > 0u) m = umin(m, zm);
      if (lz < 3u) m = umin(m, zp);
      if (ly > 0u) m = umin(m, ym);
      if (ly < 3u) m = umin(m, yp);
      if (lx > 0u) m = umin(m, xm);
      if (lx < 3u) m = umin(m, xp);
      const bool lower = open && m + 1u <= a.max_steps && m + 1u < v;
      if (lower) v = m + 1u;
      if (!__any(lower)) break;
    }
    const bool dropped = v < v0;
    if (dropped) a.field[at] = (uint16_t)v;
    // Whom to wake: the brick behind a face on which some lane's value dropped AND would lower the facing voxel as it was read above.
    // (That read may be stale, but the voxel's value only decreases: if v + 1 does not beat what was read, it does not beat what is
    // there now. A facing voxel that is impassable reads kFieldNone and wakes its brick for nothing, once.)
    const bool news = (dropped || (a.first != 0u && v != kFieldNone)) && v + 1u <= a.max_steps;
    const uint64_t news_x = __ballot(news && v + 1u < ext_x), news_y = __ballot(news && v + 1u < ext_y), news_z = __ballot(news && v + 1u < ext_z);
    if ((news_x | news_y | news_z) != 0ull && lane < 6u) {  // lane f looks after face f: -x, +x, -y, +y, -z, +z
      const uint64_t x_face = 0xFFFFull, y_face = 0x000F000F000F000Full, z_face = 0x1111111111111111ull;
      const uint32_t axis = lane >> 1, up = lane & 1u;
      const uint64_t face = axis == 0u ? news_x & (x_face << (up ? 48 : 0)) : axis == 1u ? news_y & (y_face << (up ? 12 : 0)) : news_z & (z_face << (up ? 3 : 0));
      uint32_t b[3] = {bx, by, bz};
      const uint32_t c = axis == 0u ? bx : axis == 1u ? by : bz;
      const uint32_t lo = (axis == 0u ? a.lo[0] : axis == 1u ? a.lo[1] : a.lo[2]) >> 2, hi = (axis == 0u ? a.hi[0] : axis == 1u ? a.hi[1] : a.hi[2]) >> 2;
      const uint32_t to = up ? c + 1u : c - 1u;  // (c == 0 wraps above hi)
      if (face != 0ull && to >= lo && to <= hi) {  // hi <= 63: inside the lattice, and inside the region's bricks
        if (axis == 0u) b[0] = to; else if (axis == 1u) b[1] = to; else b[2] = to;
        wake(a.next_flag, a.next_list, a.next_count, leaf_code(b[0], b[1], b[2]));
      }
    }
  }
}

// a workgroup per root cell (16^3 voxels, 64 bricks contiguous in the field) of the region's cell box, a wave per 16 bricks
__global__ void __launch_bounds__(256) k_flood_result(FloodArgs a) {
  __shared__ uint32_t sum[kFloodAccWords];
  if (threadIdx.x < kFloodAccWords) sum[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t cell = region_cells(a).cell(blockIdx.x);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t reached = 0, farthest = 0, zeros = 0, boundary = 0, inv_lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t code = cell * 64u + wave * 16u + k;
    const uint32_t v = a.field[(size_t)code * 64u + lane];
    if (v == kFieldNone) continue;
    const Voxel at = code_voxel(code, lane);
    const uint32_t p[3] = {at.x, at.y, at.z};
    reached += 1u;
    farthest = v > farthest ? v : farthest;
    zeros += v == 0u ? 1u : 0u;
    bool on_face = false;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      on_face |= p[r] == a.lo[r] || p[r] == a.hi[r];
      inv_lo[r] = 255u - p[r] > inv_lo[r] ? 255u - p[r] : inv_lo[r];
      hi[r] = p[r] > hi[r] ? p[r] : hi[r];
    }
    boundary += on_face ? 1u : 0u;
  }
  if (reached) {
    atomicAdd(&sum[0], reached); atomicMax(&sum[1], farthest); atomicAdd(&sum[2], zeros); atomicAdd(&sum[3], boundary);
#pragma unroll
    for (int r = 0; r < 3; ++r) { atomicMax(&sum[4 + r], inv_lo[r]); atomicMax(&sum[7 + r], hi[r]); }
  }
  __syncthreads();
  if (sum[0] == 0u) return;
  if (threadIdx.x == 0u || threadIdx.x == 2u || threadIdx.x == 3u) atomicAdd(&a.acc[threadIdx.x], sum[threadIdx.x]);  // integer sums and maxima:
  else if (threadIdx.x < 10u) atomicMax(&a.acc[threadIdx.x], sum[threadIdx.x]);                                      // the order does not matter
}

// a thread per start: the first neighbour one step closer, in the order -x, +x, -y, +y, -z, +z, until a seed or the capacity
__global__ void __launch_bounds__(256) k_flood_paths(const uint16_t* field, const uint32_t* starts, uint32_t n, uint32_t capacity, uint32_t* keys, uint32_t* lengths) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t x = starts[i * 3], y = starts[i * 3 + 1], z = starts[i * 3 + 2];  // (the host has checked the coordinates)
  uint32_t d = field[voxel_index(x, y, z)];
  lengths[i] = d == kFieldNone ? 0u : d + 1u;
  if (d == kFieldNone) return;
  const uint32_t count = d + 1u < capacity ? d + 1u : capacity;
  uint32_t* out = keys + (size_t)i * capacity;
  for (uint32_t k = 0; k < count; ++k) {
    out[k] = Voxel{x, y, z}.key();
    if (k + 1u == count) break;
    const uint32_t want = d - 1u;  // (d >= 1 here: k + 1 < count <= d + 1)
    if (x > 0u && field[voxel_index(x - 1u, y, z)] == want) x -= 1u;
    else if (x < 255u && field[voxel_index(x + 1u, y, z)] == want) x += 1u;
    else if (y > 0u && field[voxel_index(x, y - 1u, z)] == want) y -= 1u;
    else if (y < 255u && field[voxel_index(x, y + 1u, z)] == want) y += 1u;
    else if (z > 0u && field[voxel_index(x, y, z - 1u)] == want) z -= 1u;
    else if (z < 255u && field[voxel_index(x, y, z + 1u)] == want) z += 1u;
    else break;  // (never taken on a converged field: a reached voxel that is no seed has a neighbour one step closer)
    d = want;
  }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_flood_seed(const FloodArgs& a, hipStream_t s) {
  hipError_t e = hipMemsetAsync(a.field, 0xFF, (size_t)kLattice * 64u * 2u, s);
  if (e != hipSuccess) return e;
  if (a.n_seeds) hipLaunchKernelGGL(k_flood_seed, dim3((a.n_seeds + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_flood_relax(const FloodArgs& a, uint32_t workgroups, hipStream_t s) {
  hipLaunchKernelGGL(k_flood_relax, dim3(workgroups ? workgroups : 1u), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_flood_result(const FloodArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_flood_result, dim3(region_cells(a).count()), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_flood_paths(const uint16_t* field, const uint32_t* starts, uint32_t n, uint32_t capacity, uint32_t* keys, uint32_t* lengths, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_flood_paths, dim3((n + 255u) / 256u), dim3(256), 0, s, field, starts, n, capacity, keys, lengths);
  return hipGetLastError();
}

}  // namespace dust
