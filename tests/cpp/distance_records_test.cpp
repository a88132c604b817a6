// distance_records_test.cpp -- the distance half of dust_amd/csrc/model_records.hpp driven on a CPU (tests/test_distance_records.py
// builds this with g++ under AddressSanitizer and UBSan; no HIP compiler, not linked against the library).
//   distance_records_test < lines
// "q target metric flags palette max_radius"  ->  "q ok target metric byte radius limit walls"   (device_distance)
// "r best targets far"                        ->  "r targets near far largest largest_key"       (distance_result)
#include <cinttypes>
#include <cstdio>

#include "model_records.hpp"

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 'q') {
      DustHipDistanceQuery q{};
      q.struct_size = sizeof(q);
      if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd32 " %" SCNu32, &q.target, &q.metric, &q.flags, &q.palette, &q.max_radius) != 5) return 2;
      dust::DistanceArgs a{};
      const bool ok = dust::device_distance(q, a);
      std::printf("q %d %u %u %u %u %u %u\n", int(ok), a.target, a.metric, a.byte, a.radius, a.limit, a.walls);
    } else if (kind == 'r') {
      dust::DistanceAcc acc{};
      uint64_t best = 0;
      if (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu32, &best, &acc.targets, &acc.far) != 3) return 2;
      acc.best = best;
      const DustHipDistanceResult r = dust::distance_result(acc);
      std::printf("r %u %u %u %u %u\n", r.targets, r.near, r.far, r.largest, r.largest_key);
    } else {
      return 2;
    }
  }
  return 0;
}
