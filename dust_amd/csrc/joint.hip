// joint.hip -- model joints (dust_hip_model_joints): for every pair of distinct GROUPS of voxels -- palette indices, or the cells of the
// standing fracture with REST for the solid voxels beyond it -- that share at least one voxel face, one record: the faces, their six
// directions, the bounds and the sums of their centres. The model is only read. The arithmetic is joint_rule.hpp's; this file decides
// which faces go into which record and where a pair's record is kept while it is summed.
//
// k_joints has k_bodies' skeleton: a workgroup per root cell of the region's CellBox, four waves of 16 bricks, lane = voxel bit. A brick
// OWNS the faces whose lower voxel it holds, so it looks at three neighbour bricks, not six. Per axis the voxel pairs that both exist are
// one wave-uniform word made from the brick's mask and its neighbour's (the region's masks applied to both): a brick without such a pair
// loads no group at all, an axis without one is skipped. A lane's own group is one load (a grid byte, a uint16 of the cell field); its
// +r neighbour's comes from a cross-lane move, on the brick's upper face from the neighbour brick's facing plane. The distinct (pair,
// direction) words of an axis are taken as k_fracture_records and k_bodies take distinct groups: the first open lane's word, the ballot
// of its equals, clear; the ballot goes through joint_part as scalar work. A wave keeps ONE running part for the pair it is looking at
// (Held in k_bodies) and sends it off only when the pair changes or its bricks end: a flat cut between two cells is the same pair brick
// after brick. Sending is one lane's work: it finds the pair's slot in an open-addressing table (compare-and-swap on the key word
// against the free value, linear probing, bounded by joint_probe_limit) and adds with ordinary vector atomics into the slot, which was
// neutral before anyone claimed it -- nobody waits for anybody. Fields that hold the neutral element are skipped. A pair that finds no
// slot sets the overflow word and is given up: the host doubles the table and runs the kernel again. (Integer atomic rates on this chip
// are unmeasured: their number is kept small rather than budgeted.) All integer adds and maxima and the output sorted by key: neither
// arrival order nor slot placement shows, two runs give the same bytes. No fences, spins or waits BETWEEN workgroups, no barrier at all.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "joint.hpp"
#include "surface_rule.hpp"  // surface_region_mask

namespace dust {

namespace {

template <uint32_t kAxis>
struct AxisWords;
template <>
struct AxisWords<0> { static constexpr uint64_t plane0 = kBodyX0; static constexpr uint32_t shift = kBodyShiftX; };
template <>
struct AxisWords<1> { static constexpr uint64_t plane0 = kBodyY0; static constexpr uint32_t shift = kBodyShiftY; };
template <>
struct AxisWords<2> { static constexpr uint64_t plane0 = kBodyZ0; static constexpr uint32_t shift = kBodyShiftZ; };

// the group of voxel `bit` of brick `code` (code < kLattice, bit < 64: inside the grid and the field)
template <uint32_t kGroup>
__device__ __forceinline__ uint32_t load_group(const JointArgs& a, uint32_t code, uint32_t bit) {
  const size_t at = (size_t)code * 64u + bit;
  if constexpr (kGroup == kJointsMaterials) return (uint32_t)a.grid[at] - 1u;
  else return a.field[at];  // a cell index below 4096, or kFractureNoCell == kJointRest
}

// the lower voxels of the voxel pairs (p, p + e_axis) of brick (bx, by, bz) that both exist, `m` its existing voxels; `ncode` the
// neighbour brick toward +axis where the pairs across the brick's upper face live (none at the tree's face)
template <uint32_t kAxis>
__device__ __forceinline__ uint64_t axis_pairs(const JointArgs& a, uint64_t m, uint32_t bx, uint32_t by, uint32_t bz, uint32_t& ncode) {
  constexpr uint64_t plane0 = AxisWords<kAxis>::plane0;
  constexpr uint32_t shift = AxisWords<kAxis>::shift;
  const uint32_t nx = bx + (kAxis == 0u ? 1u : 0u), ny = by + (kAxis == 1u ? 1u : 0u), nz = bz + (kAxis == 2u ? 1u : 0u);
  uint64_t nm = 0;
  ncode = 0;
  if ((nx | ny | nz) < 64u) {
    ncode = leaf_code(nx, ny, nz);  // < kLattice
    nm = uniform64(a.brick_mask[ncode]) & surface_region_mask(nx, ny, nz, a.lo, a.hi);
  }
  const uint64_t inner = m & (m >> shift) & ~(plane0 << (3u * shift));
  const uint64_t cross = m & ((nm & plane0) << (3u * shift));
  return inner | cross;
}

// one wave sends what it holds for pair `key` (wave-uniform) to the pair's slot: one lane, an atomic per field that is not neutral
__device__ __forceinline__ void flush(const JointArgs& a, uint32_t key, const JointPart& h, uint32_t lane) {
  if (joint_is_neutral(h) || lane != 0u) return;
  // (a hint, not a wait: once the table is known to be too small the host runs the kernel again whatever is added from here on)
  if (__hip_atomic_load(&a.counters[kJointOverflow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
  const uint32_t word = joint_slot_word(key), hash = joint_hash(key, a.slots_log2), limit = joint_probe_limit(a.slots_log2);
  JointSlot* slot = nullptr;
  for (uint32_t step = 0; step < limit; ++step) {
    JointSlot* s = a.slots + joint_probe(hash, step, a.slots_log2);  // < 2^slots_log2
    const uint32_t before = atomicCAS(&s->key, kJointSlotEmpty, word);
    if (before == kJointSlotEmpty) atomicAdd(&a.counters[kJointClaims], 1u);
    if (before == kJointSlotEmpty || before == word) { slot = s; break; }
  }
  if (slot == nullptr) {
    atomicOr(&a.counters[kJointOverflow], 1u);
    return;
  }
#pragma unroll
  for (int d = 0; d < 6; ++d)
    if (h.by_face[d] != 0u) atomicAdd(&slot->by_face[d], h.by_face[d]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (h.inv_lo2[r] != 0u) atomicMax(&slot->bounds[r], h.inv_lo2[r]);
    if (h.hi2[r] != 0u) atomicMax(&slot->bounds[3 + r], h.hi2[r]);
    if (h.sum2[r] != 0ull) atomicAdd(&slot->sum2[r], (unsigned long long)h.sum2[r]);
  }
}

// the faces of one axis of one brick into the wave's running part: `pairs` from axis_pairs, `g` the lane's own group
template <uint32_t kGroup, uint32_t kAxis>
__device__ __forceinline__ void axis_faces(const JointArgs& a, uint64_t pairs, uint32_t ncode, uint32_t g, uint32_t lane, uint32_t bx, uint32_t by,
                                           uint32_t bz, JointPart& h, uint32_t& held) {
  constexpr uint64_t plane0 = AxisWords<kAxis>::plane0;
  constexpr uint32_t shift = AxisWords<kAxis>::shift;
  if (pairs == 0ull) return;
  const bool paired = ((pairs >> lane) & 1ull) != 0ull;
  uint32_t n = (uint32_t)__shfl((int)g, (int)((lane + shift) & 63u), 64);
  if ((pairs & (plane0 << (3u * shift))) != 0ull) {  // uniform: some pair crosses the brick's upper face
    const bool top = (((uint64_t)plane0 << (3u * shift)) >> lane) & 1ull;
    if (top && paired) n = load_group<kGroup>(a, ncode, lane - 3u * shift);  // the facing voxel: the same bit on the neighbour's plane 0
  }
  const bool face = paired && g != n;
  uint64_t open = __ballot(face);
  if (open == 0ull) return;
  bool flip;
  const uint32_t key = joint_face_key(g, n, flip);
  const uint32_t mine = (key << 1) | (flip ? 1u : 0u);
  while (open != 0ull) {
    const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)__builtin_ctzll(open));
    const uint64_t mg = __ballot(face && mine == word);  // holds the first open lane
    open &= ~mg;
    const JointPart p = joint_part(mg, kAxis, (word & 1u) != 0u, bx, by, bz);
    const uint32_t pair = word >> 1;
    if (pair != held && !joint_is_neutral(h)) {
      flush(a, held, h, lane);
      h = joint_neutral();
    }
    held = pair;
    joint_fold(h, p);
  }
}

}  // namespace

template <uint32_t kGroup>
__global__ void __launch_bounds__(256) k_joints(JointArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6);
  const uint32_t cell = a.box.cell(blockIdx.x);
  JointPart h = joint_neutral();  // what this wave holds for pair `held` (every member wave-uniform)
  uint32_t held = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint32_t c = wave * 16u + k, code = cell * 64u + c;  // < kLattice: the box's cells are below 4096
    const uint64_t own = uniform64(a.brick_mask[code]);
    if (own == 0ull) continue;
    uint32_t bx, by, bz;
    cell_brick(cell, c, bx, by, bz);
    const uint64_t m = own & surface_region_mask(bx, by, bz, a.lo, a.hi);
    if (m == 0ull) continue;
    uint32_t nx, ny, nz;
    const uint64_t px = axis_pairs<0>(a, m, bx, by, bz, nx), py = axis_pairs<1>(a, m, bx, by, bz, ny), pz = axis_pairs<2>(a, m, bx, by, bz, nz);
    if ((px | py | pz) == 0ull) continue;
    const uint32_t g = load_group<kGroup>(a, code, lane);  // (of a voxel that does not exist: not looked at)
    axis_faces<kGroup, 0>(a, px, nx, g, lane, bx, by, bz, h, held);
    axis_faces<kGroup, 1>(a, py, ny, g, lane, bx, by, bz, h, held);
    axis_faces<kGroup, 2>(a, pz, nz, g, lane, bx, by, bz, h, held);
  }
  flush(a, held, h, lane);
}

// a thread per slot: the claimed ones as (pair key, slot), ranked by one counter with one add per wave. The list's order is arrival
// order; the sort that follows is by unique keys
__global__ void __launch_bounds__(256) k_joints_compact(JointArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;  // < 2^slots_log2: the grid is slots / 256 workgroups
  const uint32_t word = a.slots[i].key;
  const bool claimed = word != kJointSlotEmpty;
  const uint64_t ballot = __ballot(claimed);
  if (ballot == 0ull) return;
  uint32_t base = 0;
  if (lane == (uint32_t)__builtin_ctzll(ballot)) base = atomicAdd(&a.counters[kJointRank], (uint32_t)__popcll(ballot));
  base = (uint32_t)__shfl((int)base, (int)__builtin_ctzll(ballot), 64);
  const uint32_t at = base + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
  if (claimed && at < a.n) {
    a.keys[at] = word - 1u;
    a.vals[at] = i;
  }
}

// a thread per record: slot -> the 80-byte record
__global__ void __launch_bounds__(256) k_joints_emit(JointArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n || i >= a.capacity) return;
  const uint32_t at = a.sorted_vals[i] & ((1u << a.slots_log2) - 1u);  // (a slot index already: the mask keeps a wrong one inside the table)
  const JointSlot s = a.slots[at];
  JointPart p;
#pragma unroll
  for (int d = 0; d < 6; ++d) p.by_face[d] = s.by_face[d];
#pragma unroll
  for (int r = 0; r < 3; ++r) { p.inv_lo2[r] = s.bounds[r]; p.hi2[r] = s.bounds[3 + r]; p.sum2[r] = s.sum2[r]; }
  a.records[i] = joint_emit(a.sorted_keys[i], p);
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_joints(const JointArgs& a, hipStream_t s) {
  switch (a.group) {
    case kJointsMaterials: hipLaunchKernelGGL(k_joints<kJointsMaterials>, dim3(a.box.count()), dim3(256), 0, s, a); break;
    case kJointsCells: hipLaunchKernelGGL(k_joints<kJointsCells>, dim3(a.box.count()), dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_joints_compact(const JointArgs& a, hipStream_t s) {
  static_assert(kJointMinSlotsLog2 >= 8u, "a thread per slot, whole workgroups");
  if (a.n) hipLaunchKernelGGL(k_joints_compact, dim3((1u << a.slots_log2) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_joints_emit(const JointArgs& a, hipStream_t s) {
  const uint32_t n = a.n < a.capacity ? a.n : a.capacity;
  if (n) hipLaunchKernelGGL(k_joints_emit, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
