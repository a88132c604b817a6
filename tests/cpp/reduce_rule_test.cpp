// dust_amd/csrc/reduce_rule.hpp on a CPU (tests/test_reduce_rule.py compiles this with g++ under AddressSanitizer and UBSan): one
// line of standard input per question, one line of output per answer.
//   v <children> <min_solid>       -> v <the coarse byte>                      (children: the eight grid bytes packed in 64 bits, decimal)
//   q <levels> <min_solid> <flags> -> q <valid> [<n> <extent of the result> then per level: from to extent cover fresh count_src count_dst]
//   r <levels> <src> <dst>         -> r <src_voxels> <voxels> <extent> <reserved>
#include <cinttypes>
#include <cstdio>

#include "reduce_rule.hpp"

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 'v') {
      uint64_t children;
      unsigned min_solid;
      if (std::scanf("%" SCNu64 " %u", &children, &min_solid) != 2) return 2;
      std::printf("v %u\n", dust::reduce_vote(children, min_solid));
    } else if (kind == 'q') {
      DustHipReduce q{};
      q.struct_size = sizeof(q);
      if (std::scanf("%u %u %u", &q.levels, &q.min_solid, &q.flags) != 3) return 2;
      dust::ReducePlan p{};
      if (!dust::device_reduce(q, p)) { std::printf("q 0\n"); continue; }
      std::printf("q 1 %u %u", p.n, dust::reduce_result(p, 0, 0).extent);
      for (uint32_t k = 0; k < p.n; ++k) {
        const dust::ReduceLevel& l = p.level[k];
        std::printf(" %u %u %u %u %u %u %u", l.from, l.to, l.extent, l.cover, l.fresh, l.count_src, l.count_dst);
      }
      std::printf("\n");
    } else if (kind == 'r') {
      DustHipReduce q{};
      unsigned src, dst;
      q.min_solid = 1;
      if (std::scanf("%u %u %u", &q.levels, &src, &dst) != 3) return 2;
      dust::ReducePlan p{};
      if (!dust::device_reduce(q, p)) return 3;
      const DustHipReduceResult r = dust::reduce_result(p, src, dst);
      std::printf("r %u %u %u %u\n", r.src_voxels, r.voxels, r.extent, r.reserved);
    } else {
      return 2;
    }
  }
  return 0;
}
