// joint_rule.hpp -- the device-free half of the model joints (dust_hip_model_joints): the ONE text of everything that is arithmetic -- the
// order and the packing of a pair of groups, what the shared faces of one axis inside one 4^3 brick add to their pair's record, the fold,
// the emit, and the hash and probe sequence of the open-addressing table the pairs are collected in. Bit x<<4 | y<<2 | z of a word is
// voxel (x, y, z) of the brick (grid.hpp voxel_bit). Integer work over values: no HIP call, no memory access, no array indexed by a
// runtime value. joint.hip calls it per (brick, axis, pair, direction), where every word is wave-uniform (scalar work);
// tests/cpp/joint_rule_test.cpp runs the same text on a CPU (tests/test_joint_rule.py).
//
// A FACE is a pair of voxels p and p + e_r that both exist and whose groups differ; it is named by its LOWER voxel p and its axis r. Its
// centre in half voxels is 2 p + 1 + e_r: 2 p_r + 2 along r (2..510), 2 p + 1 on the other two axes (1..511). A part's sums stay far
// below 2^64: one pair holds at most 3 * 2^24 faces of coordinates up to 511.
#pragma once
#include <cstdint>

#include "body_rule.hpp"  // body_axis_counts, body_axis_bounds, the planes of a brick word

#ifdef __HIPCC__
#define DUST_JOINT_FN __host__ __device__ __forceinline__
#else
#define DUST_JOINT_FN inline
#endif

namespace dust {

constexpr uint32_t kJointRest = 0xFFFFu;      // DUST_HIP_JOINT_REST: the group of a solid voxel that answers DUST_HIP_NO_CELL
constexpr uint32_t kJointKeyBits = 25;        // a << 13 | b': a below 4096; b' = b below 4096, or 4096 for REST
constexpr uint32_t kJointRestField = 4096u;   // what stands for REST in a packed key: above every cell index, so REST sorts last
constexpr uint32_t kJointSlotEmpty = 0u;      // a slot's key word before anyone claims it: the table is cleared with zeroes
constexpr uint32_t kJointMaxProbes = 128u;    // a pair that finds no slot within this many probes (or the slot count) counts as overflow
constexpr uint32_t kJointMinSlotsLog2 = 10, kJointFirstMaxSlotsLog2 = 16, kJointMaxSlotsLog2 = 24;

// ---- the pair key. Groups are palette indices 0..254, cell indices 0..4095 or kJointRest; a < b numerically puts REST last.
DUST_JOINT_FN uint32_t joint_pack(uint32_t a, uint32_t b) { return (a << 13) | (b == kJointRest ? kJointRestField : b); }
DUST_JOINT_FN uint32_t joint_key_a(uint32_t key) { return key >> 13; }
DUST_JOINT_FN uint32_t joint_key_b(uint32_t key) { return (key & 8191u) == kJointRestField ? kJointRest : (key & 8191u); }
// the key of the face between a lower voxel of group g and an upper voxel of group n (g != n); `flip`: the lower voxel is b, so the
// direction from a to b is -r
DUST_JOINT_FN uint32_t joint_face_key(uint32_t g, uint32_t n, bool& flip) {
  flip = g > n;
  return flip ? joint_pack(n, g) : joint_pack(g, n);
}

// ---- what a set of faces adds to a record. The neutral element is all zeroes: the lower bounds are kept as 512 - lo2 (a face centre is
// at least 1), so that a zeroed slot is empty and both bounds fold with a maximum.
struct JointPart {
  uint32_t by_face[6];  // -x, +x, -y, +y, -z, +z: the direction from the a voxel to the b voxel
  uint32_t inv_lo2[3], hi2[3];
  uint64_t sum2[3];
};
struct JointRecord {  // DustHipJoint, 80 bytes
  uint32_t a, b, faces, reserved0;
  uint32_t by_face[6];
  uint16_t lo2[3], hi2[3];
  uint32_t reserved1;
  uint64_t sum2[3];
};
static_assert(sizeof(JointRecord) == 80, "DustHipJoint");

DUST_JOINT_FN JointPart joint_neutral() {
  JointPart p;
#pragma unroll
  for (int d = 0; d < 6; ++d) p.by_face[d] = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) { p.inv_lo2[r] = p.hi2[r] = 0; p.sum2[r] = 0; }
  return p;
}
DUST_JOINT_FN bool joint_is_neutral(const JointPart& p) {
  return (p.by_face[0] | p.by_face[1] | p.by_face[2] | p.by_face[3] | p.by_face[4] | p.by_face[5]) == 0u;
}

// one axis k of a part: the faces `word` (not 0; bit = the lower voxel) of the brick whose lowest voxel has coordinate `base` on this
// axis; `along`: k is the faces' own axis, where the centre lies half a voxel further
DUST_JOINT_FN void joint_axis(uint64_t word, uint32_t n, uint64_t plane0, uint32_t shift, uint32_t base, bool along, uint32_t& inv_lo2, uint32_t& hi2,
                              uint64_t& sum2) {
  const uint32_t off = along ? 2u : 1u;
  uint32_t first, second, inv_lo, hi;
  body_axis_counts(word, plane0, shift, first, second);
  body_axis_bounds(word, plane0, shift, base, inv_lo, hi);
  sum2 = uint64_t(n) * (2u * base + off) + 2u * first;
  inv_lo2 = 512u - (2u * (255u - inv_lo) + off);
  hi2 = 2u * hi + off;
}
// What the owned faces of ONE axis (0, 1, 2) add to their pair's record: `word` (not 0) holds the lower voxels p of the faces (p, p +
// e_axis) inside brick (bx, by, bz); `flip`: the lower voxels belong to b.
DUST_JOINT_FN JointPart joint_part(uint64_t word, uint32_t axis, bool flip, uint32_t bx, uint32_t by, uint32_t bz) {
  JointPart p;
  const uint32_t n = body_popcount(word), d = 2u * axis + (flip ? 0u : 1u);
#pragma unroll
  for (uint32_t k = 0; k < 6u; ++k) p.by_face[k] = k == d ? n : 0u;
  joint_axis(word, n, kBodyX0, kBodyShiftX, bx * 4u, axis == 0u, p.inv_lo2[0], p.hi2[0], p.sum2[0]);
  joint_axis(word, n, kBodyY0, kBodyShiftY, by * 4u, axis == 1u, p.inv_lo2[1], p.hi2[1], p.sum2[1]);
  joint_axis(word, n, kBodyZ0, kBodyShiftZ, bz * 4u, axis == 2u, p.inv_lo2[2], p.hi2[2], p.sum2[2]);
  return p;
}
DUST_JOINT_FN void joint_fold(JointPart& into, const JointPart& p) {
#pragma unroll
  for (int d = 0; d < 6; ++d) into.by_face[d] += p.by_face[d];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    into.inv_lo2[r] = into.inv_lo2[r] > p.inv_lo2[r] ? into.inv_lo2[r] : p.inv_lo2[r];
    into.hi2[r] = into.hi2[r] > p.hi2[r] ? into.hi2[r] : p.hi2[r];
    into.sum2[r] += p.sum2[r];
  }
}
// accumulator -> record (a pair without faces has no record: p is not neutral)
DUST_JOINT_FN JointRecord joint_emit(uint32_t key, const JointPart& p) {
  JointRecord r;
  r.a = joint_key_a(key);
  r.b = joint_key_b(key);
  r.faces = 0;
#pragma unroll
  for (int d = 0; d < 6; ++d) { r.by_face[d] = p.by_face[d]; r.faces += p.by_face[d]; }
  r.reserved0 = r.reserved1 = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.lo2[k] = (uint16_t)(512u - p.inv_lo2[k]);
    r.hi2[k] = (uint16_t)p.hi2[k];
    r.sum2[k] = p.sum2[k];
  }
  return r;
}

// ---- the table: 2^slots_log2 slots, linear probing from a multiplicative hash. A slot's key word holds key + 1 (kJointSlotEmpty: free).
DUST_JOINT_FN uint32_t joint_slot_word(uint32_t key) { return key + 1u; }
DUST_JOINT_FN uint32_t joint_hash(uint32_t key, uint32_t slots_log2) { return (joint_slot_word(key) * 0x9E3779B1u) >> (32u - slots_log2); }
DUST_JOINT_FN uint32_t joint_probe(uint32_t hash, uint32_t step, uint32_t slots_log2) { return (hash + step) & ((1u << slots_log2) - 1u); }
// how many probes a pair gets before the table counts as full: never more than the slot count; every slot of the largest table, which
// cannot be doubled and cannot be full
DUST_JOINT_FN uint32_t joint_probe_limit(uint32_t slots_log2) {
  return (slots_log2 < 7u || slots_log2 >= kJointMaxSlotsLog2) ? (1u << slots_log2) : kJointMaxProbes;
}
// The first table of a call over `cells` root cells: sixteen slots per root cell, between 2^10 and 2^16 -- the whole tree gets 65 536
// slots, which hold MATERIALS' 32 385 pairs at a load below one half. A table that overflows is doubled, up to 2^24 slots: more than
// twice the 8 390 656 pairs 4096 cells and REST can form.
DUST_JOINT_FN uint32_t joint_first_slots_log2(uint32_t cells) {
  uint32_t log2 = kJointMinSlotsLog2;
  while (log2 < kJointFirstMaxSlotsLog2 && (1u << log2) < 16u * cells) ++log2;
  return log2;
}

}  // namespace dust
