// fracture_rule_test.cpp -- the device-free half of the model fracture driven on a CPU (tests/test_fracture_rule.py builds this with
// g++ under AddressSanitizer and UBSan and checks what it prints): fracture_d2, fracture_min_d2 / fracture_max_d2, fracture_before,
// fracture_candidate and fracture_label of dust_amd/csrc/fracture_rule.hpp -- the text k_fracture_label of fracture.hip runs per lane --
// held to loops over the voxels written here, and device_fracture / fracture_seeds / fracture_apply_arguments / fracture_selection /
// fracture_result / fracture_empty_cell of dust_amd/csrc/model_records.hpp. One line per request of stdin:
//   b SCALE[3] LIMIT LO[3] HI[3] N SEEDS[3 N] -> b CANDIDATES U LABELS[voxels of the box, x slowest] MIN_D2[N] MAX_D2[N]
//        (checked here: min / max against the loops over the box; the candidates hold every voxel's brute-force winner; the winner over
//        the candidates, in reversed order, is the winner over all seeds)
//   q PALETTE SCALE[3] FLAGS RESERVED0 RESERVED LIMIT LO[3] HI[3] -> q 0 | q 1 EMPTY BYTE LIMIT SCALE[3] [LO[3] HI[3] BOX_LO[3] BOX_HI[3]]
//   s X Y Z RESERVED                                            -> s 0 | s 1     refused or not
//   a WHERE VALUE                                               -> a 0 | a 1
//   d N_SEEDS N CELLS[N]                                        -> d 0 | d 1 WORDS[64]
//   r ACC[16]  |  r                                             -> r SOLID LABELLED CELLS LARGEST_CELL LARGEST_VOXELS CUT_FACES MAX_D2 LO[3] HI[3] NONZERO
//   e                                                           -> e VOXELS CUT_FACES LO[3] HI[3] SUM[3] NONZERO     the empty cell
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "fracture_rule.hpp"
#include "model_records.hpp"

namespace {

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(3);                                                       \
    }                                                                     \
  } while (0)

struct Seed { int32_t x, y, z; };

int run() {
  std::string line;
  std::vector<char> buf(1 << 20);
  while (std::fgets(buf.data(), int(buf.size()), stdin)) {
    line = buf.data();
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "b") {
      uint32_t scale[3], limit, n;
      dust::FractureBox box;
      for (uint32_t& v : scale) in >> v;
      in >> limit;
      for (int32_t& v : box.lo) in >> v;
      for (int32_t& v : box.hi) in >> v;
      in >> n;
      std::vector<Seed> seeds(n);
      for (Seed& s : seeds) in >> s.x >> s.y >> s.z;
      if (!in) return 2;
      // min and max against the loops over the box
      std::vector<uint32_t> lo_d2(n), hi_d2(n);
      uint32_t u = dust::kFractureNoLimit;
      for (uint32_t i = 0; i < n; ++i) {
        uint32_t mn = 0xFFFFFFFFu, mx = 0;
        for (int32_t x = box.lo[0]; x <= box.hi[0]; ++x)
          for (int32_t y = box.lo[1]; y <= box.hi[1]; ++y)
            for (int32_t z = box.lo[2]; z <= box.hi[2]; ++z) {
              const int64_t dx = x - seeds[i].x, dy = y - seeds[i].y, dz = z - seeds[i].z;
              const int64_t want = int64_t(scale[0]) * dx * dx + int64_t(scale[1]) * dy * dy + int64_t(scale[2]) * dz * dz;
              const uint32_t d2 = dust::fracture_d2(scale, int32_t(dx), int32_t(dy), int32_t(dz));
              CHECK(int64_t(d2) == want && want < (int64_t(1) << 27));
              mn = std::min(mn, d2); mx = std::max(mx, d2);
            }
        lo_d2[i] = dust::fracture_min_d2(scale, seeds[i].x, seeds[i].y, seeds[i].z, box);
        hi_d2[i] = dust::fracture_max_d2(scale, seeds[i].x, seeds[i].y, seeds[i].z, box);
        CHECK(lo_d2[i] == mn && hi_d2[i] == mx);
        u = std::min(u, hi_d2[i]);
      }
      std::vector<uint32_t> candidates;
      for (uint32_t i = 0; i < n; ++i)
        if (dust::fracture_candidate(lo_d2[i], u, limit)) candidates.push_back(i);
      std::printf("b %zu %u", candidates.size(), u);
      for (int32_t x = box.lo[0]; x <= box.hi[0]; ++x)
        for (int32_t y = box.lo[1]; y <= box.hi[1]; ++y)
          for (int32_t z = box.lo[2]; z <= box.hi[2]; ++z) {
            uint32_t all_d2 = dust::kFractureNoLimit, all_i = dust::kFractureNoCell;  // the brute-force winner, over every seed
            for (uint32_t i = 0; i < n; ++i) {
              const uint32_t d2 = dust::fracture_d2(scale, x - seeds[i].x, y - seeds[i].y, z - seeds[i].z);
              if (d2 < all_d2) { all_d2 = d2; all_i = i; }  // (ascending: strictly less keeps the lowest index)
            }
            uint32_t best = dust::kFractureNoLimit, best_i = dust::kFractureNoCell;  // the kernel's walk, the list backwards
            for (size_t k = candidates.size(); k-- > 0;) {
              const uint32_t i = candidates[k];
              const uint32_t d2 = dust::fracture_d2(scale, x - seeds[i].x, y - seeds[i].y, z - seeds[i].z);
              if (dust::fracture_before(d2, i, best, best_i)) { best = d2; best_i = i; }
            }
            const uint32_t want = dust::fracture_label(all_d2, all_i, limit), got = dust::fracture_label(best, best_i, limit);
            CHECK(want == got);
            if (want != dust::kFractureNoCell) {  // the winner of a labelled voxel survived the pruning, and is the winner of the walk
              bool held = false;
              for (uint32_t i : candidates) held |= i == all_i;
              CHECK(held && best_i == all_i && best == all_d2);
            }
            std::printf(" %u", got);
          }
      for (uint32_t v : lo_d2) std::printf(" %u", v);
      for (uint32_t v : hi_d2) std::printf(" %u", v);
      std::printf("\n");
    } else if (what == "q") {
      DustHipFractureQuery q{};
      q.struct_size = sizeof(q);
      uint32_t scale[3], reserved0 = 0;
      in >> q.palette >> scale[0] >> scale[1] >> scale[2] >> q.flags >> reserved0 >> q.reserved >> q.max_distance2;
      for (uint32_t& v : q.lo) in >> v;
      for (uint32_t& v : q.hi) in >> v;
      if (!in) return 2;
      for (int r = 0; r < 3; ++r) q.scale[r] = uint8_t(scale[r]);
      q.reserved0 = uint8_t(reserved0);
      dust::FractureArgs a{};
      bool empty = false;
      if (dust::device_fracture(q, a, empty) != nullptr) {
        std::printf("q 0\n");
        continue;
      }
      std::printf("q 1 %u %u %u %u %u %u", empty ? 1u : 0u, a.byte, a.limit, a.scale[0], a.scale[1], a.scale[2]);
      if (!empty)
        std::printf(" %u %u %u %u %u %u %u %u %u %u %u %u", a.lo[0], a.lo[1], a.lo[2], a.hi[0], a.hi[1], a.hi[2], a.box.lo[0], a.box.lo[1], a.box.lo[2], a.box.hi[0],
                    a.box.hi[1], a.box.hi[2]);
      std::printf("\n");
    } else if (what == "s") {
      DustHipFractureSeed s{};
      in >> s.x >> s.y >> s.z >> s.reserved;
      if (!in) return 2;
      std::printf("s %u\n", dust::fracture_seeds(&s, 1) == nullptr ? 1u : 0u);
    } else if (what == "a") {
      uint32_t where = 0;
      int32_t value = 0;
      in >> where >> value;
      if (!in) return 2;
      std::printf("a %u\n", dust::fracture_apply_arguments(where, value) == nullptr ? 1u : 0u);
    } else if (what == "d") {
      uint32_t n_seeds = 0, n = 0;
      in >> n_seeds >> n;
      std::vector<uint32_t> cells(n);
      for (uint32_t& v : cells) in >> v;
      if (!in) return 2;
      uint64_t selected[dust::kFractureSelectWords];
      if (dust::fracture_selection(cells.data(), n, n_seeds, selected) != nullptr) {
        std::printf("d 0\n");
        continue;
      }
      std::printf("d 1");
      for (uint64_t w : selected) std::printf(" %" PRIu64, w);
      std::printf("\n");
    } else if (what == "r") {
      uint32_t acc[dust::kFractureAccWords] = {};
      uint32_t n = 0;
      while (n < dust::kFractureAccWords && (in >> acc[n])) ++n;
      if (n != 0 && n != dust::kFractureAccWords) return 2;
      DustHipFractureResult r;
      std::memset(&r, 0xEE, sizeof(r));  // (every byte of the output must be written)
      r = dust::fracture_result(n ? acc : nullptr);
      uint32_t rest = r.reserved0 | r.reserved1;
      for (uint32_t v : r.reserved) rest |= v;
      std::printf("r %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", r.solid, r.labelled, r.cells, r.largest_cell, r.largest_voxels, r.cut_faces, r.max_d2, r.lo[0],
                  r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2], rest);
    } else if (what == "e") {
      const DustHipFractureCell c = dust::fracture_empty_cell();
      std::printf("e %u %u %u %u %u %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", c.voxels, c.cut_faces, c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1], c.hi[2], c.sum[0],
                  c.sum[1], c.sum[2], unsigned(c.reserved0 | c.reserved1));
    } else {
      return 2;
    }
  }
  return 0;
}

}  // namespace

int main() { return run(); }
