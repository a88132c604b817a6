// reduce_rule.hpp -- the device-free half of the model reductions (dust_hip_model_reduce): the vote of ONE coarse cell over its eight
// children, as a single function of values, and the host's arithmetic on the caller's records -- the query's validity, the plan of
// the levels (which grid each one reads and writes) and the result record. Integer work over values: no HIP call, no handle, no
// memory access, no array indexed by a runtime value (nothing goes to scratch). reduce.hip calls reduce_vote per lane;
// tests/cpp/reduce_rule_test.cpp runs the same text on a CPU (tests/test_reduce_rule.py).
#pragma once
#include <cstdint>

#include "../../include/dust_hip.h"

#ifdef __HIPCC__
#define DUST_REDUCE_FN __host__ __device__ __forceinline__
#else
#define DUST_REDUCE_FN inline
#endif

namespace dust {

// The coarse grid byte (0 = None, else palette index + 1) of a cell whose eight children's grid bytes are the bytes of `children`, in
// any order. Per solid child a key (children that carry its byte) << 8 | (255 - byte): the largest key names the byte most solid
// children carry, the LOWEST such byte among equals. The cell is solid when at least min_solid (1..8) children are.
DUST_REDUCE_FN uint32_t reduce_vote(uint64_t children, uint32_t min_solid) {
  uint32_t solid = 0, best = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t b = uint32_t(children >> (8 * i)) & 255u;
    uint32_t same = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) same += (uint32_t(children >> (8 * j)) & 255u) == b ? 1u : 0u;
    const uint32_t key = b != 0u ? (same << 8) | (255u - b) : 0u;
    best = key > best ? key : best;
    solid += b != 0u ? 1u : 0u;
  }
  return solid >= min_solid && solid != 0u ? 255u - (best & 255u) : 0u;
}

// ---- the host's half
constexpr uint32_t kReduceSource = 0, kReduceModel = 1, kReduceScratch = 2;  // ReduceLevel::from / to: the source's grid, the new model's, the context's scratch

// One launch. Level k of n reads the cube [0, 2 * extent)^3 and writes [0, extent)^3, extent = 256 >> k. The levels take turns between
// the new model's grid and the scratch so that the LAST one lands in the model's (never in place: a coarse cell would overwrite source
// cells another wave has not read yet). `cover` >= extent: the cube of the destination the launch writes every byte of, zero outside
// [0, extent)^3 -- on the last level what earlier levels left in the model's grid, which the rebuild must find empty. `fresh`: the
// destination is known to be zero wherever the launch would store a zero, so bricks that come out empty are not stored at all.
struct ReduceLevel {
  uint32_t from, to;
  uint32_t extent, cover;
  uint32_t fresh;
  uint32_t count_src, count_dst;  // the launch adds the solid voxels it reads / writes to the call's two counts
};
struct ReducePlan {
  uint32_t n;
  uint32_t min_solid;
  ReduceLevel level[DUST_HIP_REDUCE_MAX_LEVELS];
};

// false: a query the call refuses (after the struct_size and the model's kind have been looked at)
inline bool device_reduce(const DustHipReduce& q, ReducePlan& p) {
  if (q.levels < 1u || q.levels > DUST_HIP_REDUCE_MAX_LEVELS || q.min_solid < 1u || q.min_solid > 8u || q.flags != 0u) return false;
  p.n = q.levels;
  p.min_solid = q.min_solid;
  uint32_t written = 0;  // the largest cube of the model's grid an earlier level has written, 0: none yet
  for (uint32_t k = 1; k <= p.n; ++k) {
    ReduceLevel& l = p.level[k - 1];
    const bool last = k == p.n;
    l.from = k == 1u ? kReduceSource : p.level[k - 2].to;
    l.to = (p.n - k) % 2u == 0u ? kReduceModel : kReduceScratch;
    l.extent = 256u >> k;
    l.cover = last && written != 0u ? written : l.extent;
    l.fresh = l.to == kReduceModel && written == 0u ? 1u : 0u;
    l.count_src = k == 1u ? 1u : 0u;
    l.count_dst = last ? 1u : 0u;
    if (l.to == kReduceModel && written == 0u) written = l.extent;
  }
  return true;
}
inline bool reduce_needs_scratch(const ReducePlan& p) { return p.n >= 2u; }

// What the caller gets from the call's two counts
inline DustHipReduceResult reduce_result(const ReducePlan& p, uint32_t src_voxels, uint32_t voxels) {
  DustHipReduceResult r{};
  r.src_voxels = src_voxels;
  r.voxels = voxels;
  r.extent = 256u >> p.n;
  return r;
}

}  // namespace dust
