// dust_amd/csrc/resample_rule.hpp (the text k_resample of resample.hip runs) and the resample records of model_records.hpp
// (resample_op_refusal, resample_map_refusal, device_resample, the cell binning) as a CPU program of its own, built under AddressSanitizer and UBSan by
// tests/test_resample_rule.py. Cases on stdin, one per line, every number a decimal integer; M = the 9 matrix entries row by row and
// the 3 translations, in 1 / 65536:
//   s M x y z                          -> "s s0 s1 s2": the source coordinates of destination voxel (x, y, z)
//   b M lo[3] hi[3] src_lo[3] src_hi[3] -> "b min0 max0 min1 max1 min2 max2 meets any": resample_box_range over the box, the interval
//                                         test, and whether a loop over the box finds a voxel whose s lies inside the sub-box. The
//                                         program itself compares the range with the loop's minimum and maximum and a rejected box
//                                         with `any`, and exits 1 where they disagree
//   r M dst_lo[3] dst_hi[3] src_lo[3] src_hi[3] op
//                                      -> "r refused live lo hi src_lo src_hi table n cells...": what the two refusals and device_resample
//                                         make of the record and the root cells CellLists::bin lists for it. The program itself
//                                         loops over the clipped box and exits 1 if a cell that holds a voxel of the image is not listed
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "model_records.hpp"

using namespace dust;

static void die(const char* why, const std::string& line) {
  std::fprintf(stderr, "%s: %s\n", why, line.c_str());
  std::exit(1);
}

static void read_map(std::istringstream& in, DustHipResample& r) {
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) in >> r.m[k][a];
  for (int k = 0; k < 3; ++k) in >> r.t[k];
}
static ResampleMap rule_map(const DustHipResample& r) {
  ResampleMap m{};
  for (int k = 0; k < 3; ++k) {
    for (int a = 0; a < 3; ++a) m.m[k][a] = r.m[k][a];
    m.t2[k] = 2 * r.t[k];
  }
  return m;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    char kind;
    in >> kind;
    DustHipResample r{};
    read_map(in, r);
    if (kind == 's') {
      int32_t x, y, z;
      in >> x >> y >> z;
      const ResampleMap m = rule_map(r);
      std::printf("s %d %d %d\n", resample_floor(resample_q(m, 0, x, y, z)), resample_floor(resample_q(m, 1, x, y, z)), resample_floor(resample_q(m, 2, x, y, z)));
    } else if (kind == 'b') {
      int32_t lo[3], hi[3], sl[3], sh[3];
      for (int& v : lo) in >> v;
      for (int& v : hi) in >> v;
      for (int& v : sl) in >> v;
      for (int& v : sh) in >> v;
      const ResampleMap m = rule_map(r);
      ResampleRange q[3];
      resample_box_range(m, lo, hi, q);
      const bool meets = resample_box_meets(m, lo, hi, sl, sh);
      int64_t least[3], most[3];
      bool any = false, first = true;
      for (int32_t x = lo[0]; x <= hi[0]; ++x)
        for (int32_t y = lo[1]; y <= hi[1]; ++y)
          for (int32_t z = lo[2]; z <= hi[2]; ++z) {
            bool inside = true;
            for (int k = 0; k < 3; ++k) {
              const int32_t v = resample_q(m, k, x, y, z);
              if (first || v < least[k]) least[k] = v;
              if (first || v > most[k]) most[k] = v;
              inside = inside && resample_inside(resample_floor(v), sl[k], sh[k]);
            }
            first = false;
            any = any || inside;
          }
      for (int k = 0; k < 3; ++k)
        if (q[k].lo != least[k] || q[k].hi != most[k]) die("resample_box_range is not the loop's minimum and maximum", line);
      if (!meets && any) die("the interval test rejected a box that holds a voxel of the image", line);
      std::printf("b %d %d %d %d %d %d %d %d\n", q[0].lo, q[0].hi, q[1].lo, q[1].hi, q[2].lo, q[2].hi, int(meets), int(any));
    } else if (kind == 'r') {
      int v;
      for (int k = 0; k < 3; ++k) in >> r.dst_lo[k];
      for (int k = 0; k < 3; ++k) in >> r.dst_hi[k];
      for (int k = 0; k < 3; ++k) { in >> v; r.src_lo[k] = uint8_t(v); }
      for (int k = 0; k < 3; ++k) { in >> v; r.src_hi[k] = uint8_t(v); }
      in >> r.op;
      if (resample_op_refusal(r) || resample_map_refusal(r)) {
        std::printf("r 1\n");
        continue;
      }
      std::vector<DevResample> dev;
      std::vector<uint32_t> index;
      live_records<device_resample>(&r, 1, dev, index);
      if (dev.empty()) {
        std::printf("r 0 0\n");
        continue;
      }
      const DevResample& d = dev[0];
      CellLists lists;
      lists.bin(dev, 0, 1);
      if (lists.ids.size() != lists.cells.size() || lists.starts.size() != lists.cells.size() + 1) die("one record, one id per listed cell", line);
      std::vector<char> listed(4096, 0);
      for (uint32_t c : lists.cells) listed[c] = 1;
      const ResampleMap m = rule_map(r);
      for (int32_t x = int32_t(d.lo & 255u); x <= int32_t(d.hi & 255u); ++x)
        for (int32_t y = int32_t((d.lo >> 8) & 255u); y <= int32_t((d.hi >> 8) & 255u); ++y)
          for (int32_t z = int32_t(d.lo >> 16); z <= int32_t(d.hi >> 16); ++z) {
            bool inside = true;
            for (int k = 0; k < 3; ++k) inside = inside && resample_inside(resample_floor(resample_q(m, k, x, y, z)), r.src_lo[k], r.src_hi[k]);
            if (inside && !listed[((x >> 4) << 8) | ((y >> 4) << 4) | (z >> 4)]) die("a cell that holds a voxel of the image is not listed", line);
          }
      std::printf("r 0 1 %u %u %u %u %u %zu", d.lo, d.hi, d.src_lo, d.src_hi, d.table, lists.cells.size());
      for (uint32_t c : lists.cells) std::printf(" %u", c);
      std::printf("\n");
    } else {
      die("unknown case", line);
    }
  }
  return 0;
}
