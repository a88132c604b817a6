// joint.hpp -- interface between the host runtime (capi_model.cpp dust_hip_model_joints) and the joint kernels (joint.hip). The arithmetic
// itself is joint_rule.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "grid.hpp"
#include "joint_rule.hpp"

namespace dust {

// the kinds of groups, the values of DUST_HIP_JOINTS_*
constexpr uint32_t kJointsMaterials = 0, kJointsCells = 1;

// One slot of the open-addressing table: a pair while its record is being accumulated. The table is cleared with zeroes -- a free slot
// is already the neutral element, so whoever claims it (compare-and-swap on `key`) and whoever finds it claimed add at once, with integer
// atomics (adds and maxima: no order shows). joint_rule.hpp's JointPart behind the key word.
struct JointSlot {  // 80 bytes
  uint32_t key;  // joint_slot_word(pair key); kJointSlotEmpty: free
  uint32_t by_face[6];
  uint32_t pad;
  uint32_t bounds[6];  // 512 - lo2[3], then hi2[3]
  unsigned long long sum2[3];
};
static_assert(sizeof(JointSlot) == 80 && offsetof(JointSlot, sum2) == 56, "joint slot");

constexpr uint32_t kJointOverflow = 0, kJointClaims = 1, kJointRank = 2, kJointCounterWords = 4;  // JointArgs::counters

struct JointArgs {
  const uint64_t* brick_mask;  // EditArgs::brick_mask, or launch_cast_masks' array for a model that is not editable
  const uint8_t* grid;         // MATERIALS: EditArgs::grid or the expanded source grid, only read
  const uint16_t* field;       // CELLS: the cell field, brick-major
  uint32_t group;              // kJoints*
  uint32_t lo[3], hi[3];       // the inclusive region, lo <= hi
  CellBox box;                 // the root cells it reaches: one workgroup each
  JointSlot* slots;            // 2^slots_log2 slots, zeroed by the caller
  uint32_t slots_log2;
  uint32_t* counters;          // kJointCounterWords words, zeroed by the caller: table full, slots claimed, k_joints_compact's rank
  uint32_t* keys;              // k_joints_compact: the n claimed slots as (pair key, slot), in no order
  uint32_t* vals;
  const uint32_t* sorted_keys;  // k_joints_emit: the same in key order
  const uint32_t* sorted_vals;
  JointRecord* records;        // min(n, capacity) records
  uint32_t n, capacity;        // the pairs found; the records wanted
};

// radix.hip: the stable sort of (key, value) pairs the claimed slots go through, and the scratch it needs for n items
size_t radix_sort_scratch_bytes(uint32_t n);
hipError_t radix_sort_pairs(void* scratch, uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, uint32_t n,
                            uint32_t key_bits, bool* in_b, hipStream_t s);

// the region's faces into the table; counters[kJointOverflow] != 0 afterwards: the table was too small and holds nothing of use
hipError_t launch_joints(const JointArgs& a, hipStream_t s);
// the claimed slots as a list of a.n (key, slot) pairs
hipError_t launch_joints_compact(const JointArgs& a, hipStream_t s);
// the first min(a.n, a.capacity) slots of the sorted list -> records
hipError_t launch_joints_emit(const JointArgs& a, hipStream_t s);

}  // namespace dust
