// island.hip -- connected-component labelling of an editable hierarchy!(4,2,2) model's dense voxel grid (dust_hip_model_find_islands,
// dust_hip_model_island_of, dust_hip_model_detach_islands; the contract is in include/dust_hip.h).
//
// The grid (edit.hpp EditArgs::grid) is brick-major: a 4^3 brick is 64 contiguous bytes and one wavefront, lane = voxel bit
// x << 4 | y << 2 | z. The labels are a 32-bit word per voxel indexed by the PUBLIC key x << 16 | y << 8 | z, so the smallest
// label of an island is its name and a scan in index order is a scan in key order: nothing is translated at the end.
//   k_island_local    a wavefront per brick: the brick's occupancy is one ballot; every lane floods its own component inside the
//                     brick with shifts of that 64-bit mask (registers only) and points its voxel at the component's lowest bit
//   k_island_join     a wavefront per brick: every voxel pair across a brick boundary (the "forward" half of the 6 or 26 directions)
//                     is united in a lock-free union-find on the labels -- atomicMin only, a parent is always a smaller key
//   k_island_flatten  a thread per key: label = root; the roots of 64 consecutive keys are one ballot (root_mask, root_count)
//   scan              (scan.hpp) exclusive prefix sums of the 262 144 root counts: an island's rank in key order, and the number of islands
//   k_island_stats    a wavefront per 16 rows of 64 keys: voxels that share an island are reduced in the wave (one x, one y, z = lane)
//                     and across its rows before one lane adds them to the island's accumulator with integer atomics
//   k_island_emit     accumulator -> the 40-byte record
// No kernel waits for another workgroup; every loop is bounded by the data (a parent chain only descends). All arithmetic is
// integer, so the records do not depend on arrival order.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "edit.hpp"
#include "island.hpp"
#include "scan.hpp"

namespace dust {

namespace {

constexpr uint64_t kZ0 = 0x1111111111111111ull, kZ3 = 0x8888888888888888ull;  // voxel bits with z == 0 / z == 3
constexpr uint64_t kY0 = 0x000F000F000F000Full, kY3 = 0xF000F000F000F000ull;  // ... y == 0 / y == 3

__device__ __forceinline__ uint64_t grow_z(uint64_t m) { return m | ((m & ~kZ3) << 1) | ((m & ~kZ0) >> 1); }
__device__ __forceinline__ uint64_t grow_y(uint64_t m) { return m | ((m & ~kY3) << 4) | ((m & ~kY0) >> 4); }
__device__ __forceinline__ uint64_t grow_x(uint64_t m) { return m | (m << 16) | (m >> 16); }
// one step of the flood inside a brick: the face neighbours, or (three axes in turn) the whole 3^3 neighbourhood
__device__ __forceinline__ uint64_t grow(uint64_t m, bool corners) {
  return corners ? grow_x(grow_y(grow_z(m))) : (grow_z(m) | grow_y(m) | grow_x(m));
}

// Reads of the forest while other workgroups hook into it go to L2, where the atomics are performed. A stale parent would still be a
// member of the same final island (a replaced link is always re-established by the thread that replaced it), so this is about
// chain length, not correctness.
__device__ __forceinline__ uint32_t parent_of(const uint32_t* label, uint32_t i) {
  return __hip_atomic_load(label + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t find_root(const uint32_t* label, uint32_t i) {
  for (uint32_t p; (p = parent_of(label, i)) != i;) i = p;  // parents strictly descend: at most i steps
  return i;
}
// Unite the islands of a and b: hook the larger root under the smaller with atomicMin. If the word held something else (another
// thread hooked it first) the link it held is ours to re-establish: carry on with that node. Every iteration lowers max(a, b).
__device__ __forceinline__ void unite(uint32_t* label, uint32_t a, uint32_t b) {
  a = find_root(label, a);
  b = find_root(label, b);
  while (a != b) {
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicMin(label + a, b);
    if (old == a) break;
    a = old;
  }
}

}  // namespace

__global__ void __launch_bounds__(256) k_island_local(IslandArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t code = blockIdx.x * 4u + (threadIdx.x >> 6);  // iter_leaf order
  uint32_t bx, by, bz;
  leaf_decode(code, bx, by, bz);
  const bool solid = a.grid[(size_t)code * 64u + lane] != 0;
  const uint64_t occ = __ballot(solid);
  uint64_t comp = solid ? 1ull << lane : 0ull;
  if (occ != 0ull && occ != ~0ull) {
    // a path inside a brick has at most 63 steps and every round extends it by at least one: 64 rounds always suffice
    for (int round = 0; round < 64; ++round) {
      const uint64_t next = grow(comp, a.corners != 0u) & occ;
      const bool changed = next != comp;
      comp = next;
      if (!__any(changed)) break;
    }
  } else {
    comp = occ;
  }
  a.label[voxel_key(bx, by, bz, lane)] = solid ? voxel_key(bx, by, bz, (uint32_t)__builtin_ctzll(comp)) : kNoIsland;
}

__global__ void __launch_bounds__(256) k_island_join(IslandArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t code = blockIdx.x * 4u + (threadIdx.x >> 6);
  uint32_t bx, by, bz;
  leaf_decode(code, bx, by, bz);
  const uint32_t key = voxel_key(bx, by, bz, lane);
  const uint32_t mine = a.label[key];
  if (__ballot(mine != kNoIsland) == 0ull) return;
  const int x = (int)(key >> 16), y = (int)((key >> 8) & 255u), z = (int)(key & 255u);
  // the forward half of the neighbourhood: (dx, dy, dz) lexicographically above (0, 0, 0); the other half is some other voxel's forward
  const int n_dirs = a.corners ? 13 : 3;
  for (int d = 0; d < n_dirs; ++d) {
    int dx, dy, dz;
    if (!a.corners) {
      dx = d == 0; dy = d == 1; dz = d == 2;
    } else {
      const int t = d + 14;  // 14 .. 26 of the 27 offsets in (dx, dy, dz) order
      dx = t / 9 - 1; dy = (t / 3) % 3 - 1; dz = t % 3 - 1;
    }
    const int nx = x + dx, ny = y + dy, nz = z + dz;
    const bool inside = (unsigned)nx < 256u && (unsigned)ny < 256u && (unsigned)nz < 256u;
    const bool other_brick = (nx >> 2) != (x >> 2) || (ny >> 2) != (y >> 2) || (nz >> 2) != (z >> 2);  // (the same brick is k_island_local's)
    uint32_t theirs = kNoIsland;
    if (mine != kNoIsland && inside && other_brick) theirs = a.label[Voxel{(uint32_t)nx, (uint32_t)ny, (uint32_t)nz}.key()];
    bool todo = theirs != kNoIsland;
    // lanes that would unite the same two brick components (a whole face of a solid brick) leave it to the lowest of them
    const unsigned long long pair = ((unsigned long long)mine << 32) | theirs;
    bool leader = false;
    for (uint64_t open = __ballot(todo); open;) {
      const int first = __builtin_ctzll(open);
      const unsigned long long p = __shfl(pair, first);
      const uint64_t same = __ballot(todo && pair == p);
      leader |= lane == (uint32_t)first;
      open &= ~same;
    }
    if (leader) unite(a.label, mine, theirs);
  }
}

__global__ void __launch_bounds__(256) k_island_flatten(IslandArgs a) {
  const uint32_t key = blockIdx.x * 256u + threadIdx.x;
  const uint32_t p = a.label[key];
  bool root = false;
  if (p != kNoIsland) {
    uint32_t r = p;
    for (uint32_t q; (q = a.label[r]) != r;) r = q;  // (a word another thread has flattened already is a shorter way to the same root)
    if (r != p) a.label[key] = r;
    root = r == key;
  }
  const uint64_t m = __ballot(root);
  if ((threadIdx.x & 63u) == 0u) {
    a.root_mask[key >> 6] = m;
    a.root_count[key >> 6] = (uint32_t)__popcll(m);
  }
}

namespace {
// what one wave has gathered for the island it is currently looking at; every member is wave-uniform
struct Held {
  uint32_t root, voxels, lo[3], hi[3], anchored;
  unsigned long long sum[3];
};
__device__ __forceinline__ void flush(const IslandArgs& a, const Held& h, uint32_t lane) {
  if (h.voxels == 0u || lane != 0u) return;
  const uint32_t row = h.root >> 6;
  const uint32_t rank = a.root_count[row] + a.scan_tmp[row >> 10] + (uint32_t)__popcll(a.root_mask[row] & ((1ull << (h.root & 63u)) - 1ull));
  if (rank >= a.capacity) return;
  IslandAcc* acc = a.acc + rank;
  acc->key = h.root;  // (every contributor stores the same word)
  atomicAdd(&acc->voxels, h.voxels);
  for (int r = 0; r < 3; ++r) {
    atomicMax(&acc->inv_lo[r], 255u - h.lo[r]);
    atomicMax(&acc->hi[r], h.hi[r]);
    atomicAdd(&acc->sum[r], h.sum[r]);
  }
  if (h.anchored) atomicOr(&acc->flags, 1u);
}
// sum of the indices of the set bits of m
__device__ __forceinline__ uint32_t index_sum(uint64_t m) {
  return (uint32_t)__popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2u * (uint32_t)__popcll(m & 0xCCCCCCCCCCCCCCCCull) +
         4u * (uint32_t)__popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8u * (uint32_t)__popcll(m & 0xFF00FF00FF00FF00ull) +
         16u * (uint32_t)__popcll(m & 0xFFFF0000FFFF0000ull) + 32u * (uint32_t)__popcll(m & 0xFFFFFFFF00000000ull);
}
}  // namespace

constexpr uint32_t kStatsRows = 16;  // rows of 64 keys per wave: four y values, the whole z axis

__global__ void __launch_bounds__(256) k_island_stats(IslandArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
  Held h{};
  for (uint32_t k = 0; k < kStatsRows; ++k) {
    const uint32_t row = wave * kStatsRows + k;  // x << 10 | y << 2 | z >> 6
    const uint32_t x = row >> 10, y = (row >> 2) & 255u, z0 = (row & 3u) * 64u;
    const uint32_t label = a.label[row * 64u + lane];
    const bool xy_anchored = x >= a.anchor_lo[0] && x <= a.anchor_hi[0] && y >= a.anchor_lo[1] && y <= a.anchor_hi[1];
    const uint32_t z = z0 + lane;
    const uint64_t z_anchored = __ballot(z >= a.anchor_lo[2] && z <= a.anchor_hi[2]);
    for (uint64_t open = __ballot(label != kNoIsland); open;) {
      const uint32_t root = (uint32_t)__shfl((int)label, __builtin_ctzll(open));
      const uint64_t m = __ballot(label == root);
      open &= ~m;
      if (root != h.root || h.voxels == 0u) {
        flush(a, h, lane);
        h = Held{};
        h.root = root;
        h.lo[0] = h.hi[0] = x; h.lo[1] = h.hi[1] = y; h.lo[2] = 255u;
      }
      const uint32_t n = (uint32_t)__popcll(m);
      const uint32_t z_lo = z0 + (uint32_t)__builtin_ctzll(m), z_hi = z0 + 63u - (uint32_t)__builtin_clzll(m);
      h.voxels += n;
      h.lo[1] = y < h.lo[1] ? y : h.lo[1]; h.hi[1] = y > h.hi[1] ? y : h.hi[1];  // (x is the wave's)
      h.lo[2] = z_lo < h.lo[2] ? z_lo : h.lo[2]; h.hi[2] = z_hi > h.hi[2] ? z_hi : h.hi[2];
      h.sum[0] += (unsigned long long)n * x; h.sum[1] += (unsigned long long)n * y; h.sum[2] += (unsigned long long)n * z0 + index_sum(m);
      h.anchored |= (xy_anchored && (m & z_anchored) != 0ull) ? 1u : 0u;
    }
  }
  flush(a, h, lane);
}

__global__ void __launch_bounds__(256) k_island_emit(IslandArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.capacity) return;
  const IslandAcc s = a.acc[i];
  DevIsland r;
  r.key = s.key; r.voxels = s.voxels;
  r.lo_flags = (255u - s.inv_lo[0]) | ((255u - s.inv_lo[1]) << 8) | ((255u - s.inv_lo[2]) << 16) | (s.flags << 24);
  r.hi_reserved = s.hi[0] | (s.hi[1] << 8) | (s.hi[2] << 16);
  for (int k = 0; k < 3; ++k) { r.sum[2 * k] = (uint32_t)s.sum[k]; r.sum[2 * k + 1] = (uint32_t)(s.sum[k] >> 32); }
  a.records[i] = r;
}

__global__ void __launch_bounds__(256) k_island_select(const uint32_t* label, const uint32_t* keys, uint32_t n, uint64_t* selected, uint32_t* bad) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t key = keys[i];
  if (key < kIslandKeys && label[key] == key) atomicOr((unsigned long long*)&selected[key >> 6], 1ull << (key & 63u));
  else atomicAdd(bad, 1u);
}

// a wavefront per brick: the voxels of the selected islands go to dst (every other byte of dst is cleared) and, with `carve`, leave the
// source and its labelling
__global__ void __launch_bounds__(256) k_island_detach(IslandDetachArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t code = blockIdx.x * 4u + (threadIdx.x >> 6);
  uint32_t bx, by, bz;
  leaf_decode(code, bx, by, bz);
  const size_t at = (size_t)code * 64u + lane;
  const uint8_t g = a.src[at];
  bool moves = false;
  uint32_t key = 0;
  if (g != 0) {
    key = voxel_key(bx, by, bz, lane);
    const uint32_t root = a.label[key];
    moves = root != kNoIsland && ((a.selected[root >> 6] >> (root & 63u)) & 1ull) != 0ull;
  }
  if (a.dst) a.dst[at] = moves ? g : (uint8_t)0;
  if (a.carve && moves) {
    a.src[at] = 0;
    a.label[key] = kNoIsland;
  }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_island_label(const IslandArgs& a, bool relabel, hipStream_t s) {
  if (relabel) {
    hipLaunchKernelGGL(k_island_local, dim3(kLattice / 4), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_island_join, dim3(kLattice / 4), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(k_island_flatten, dim3(kIslandKeys / 256), dim3(256), 0, s, a);
  static_assert(kIslandRows == kLattice, "the root counts are a table of scan.hpp");
  return launch_table_scan(TableScan{{a.root_count, nullptr}, {a.scan_tmp + 256, nullptr}, a.scan_tmp}, 1, s);
}
hipError_t launch_island_records(const IslandArgs& a, hipStream_t s) {
  if (a.capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(k_island_stats, dim3(kIslandRows / kStatsRows / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_island_emit, dim3((a.capacity + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_island_select(const uint32_t* label, const uint32_t* keys, uint32_t n, uint64_t* selected, uint32_t* bad, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_island_select, dim3((n + 255u) / 256u), dim3(256), 0, s, label, keys, n, selected, bad);
  return hipGetLastError();
}
hipError_t launch_island_detach(const IslandDetachArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_island_detach, dim3(kLattice / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
