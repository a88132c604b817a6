// neighbour_rule_test.cpp -- the device-free half of the model neighbourhoods driven on a CPU (tests/test_neighbour_rule.py builds this
// with g++ under AddressSanitizer and UBSan and checks what it prints): neighbour_count, neighbour_change and surface_region_mask of
// dust_amd/csrc/neighbour_rule.hpp -- the text the kernels of neighbour.hip run per brick -- and device_neighbours /
// neighbours_apply_arguments / neighbours_result / neighbours_applied of dust_amd/csrc/model_records.hpp. One request per line of stdin,
// one answer per line of stdout:
//   c NB BIRTH SURVIVE LO[3] HI[3] BX BY BZ W[27] -> c PLANE[5] BORN DIED REGION     (W[(dx + 1) * 9 + (dy + 1) * 3 + dz + 1]: the brick at that offset)
//   q NB FLAGS PALETTE BIRTH SURVIVE LO[3] HI[3]  -> q 0        a refused query
//                                                   q 1 EMPTY NB WALLS BIRTH SURVIVE BYTE MAJORITY [LO[3] HI[3] CELL_LO[3] CELL_HI[3]]
//   a GENERATIONS                                 -> a 0 | a 1  refused or not
//   r ACC[10]   |   r                             -> r VOXELS SOLID BORN DIED LO[3] HI[3] NONZERO   (NONZERO: pad and reserved bytes set)
//   p G SOLID SLOT[G * 8]   |   p G               -> p GENERATIONS SOLID_BEFORE SOLID_AFTER BORN DIED LO[3] HI[3] NONZERO ROW[2 * G]
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "model_records.hpp"
#include "neighbour_rule.hpp"

int main() {
  std::string line;
  static char buf[1 << 16];
  while (std::fgets(buf, sizeof(buf), stdin)) {
    line = buf;
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "c") {
      uint32_t nb = 0, birth = 0, survive = 0, lo[3], hi[3], b[3];
      dust::NeighbourBricks n{};
      in >> nb >> birth >> survive;
      for (uint32_t& v : lo) in >> v;
      for (uint32_t& v : hi) in >> v;
      for (uint32_t& v : b) in >> v;
      for (uint64_t& w : n.w) in >> w;
      if (!in) return 2;
      const uint64_t region = dust::surface_region_mask(b[0], b[1], b[2], lo, hi);
      const dust::NeighbourCount c = dust::neighbour_count(n, nb);
      const dust::NeighbourChange g = dust::neighbour_change(n.w[dust::kNeighbourOwn], c, birth, survive, region);
      std::printf("c %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", c.b[0], c.b[1], c.b[2], c.b[3], c.b[4],
                  g.born, g.died, region);
    } else if (what == "q") {
      DustHipNeighboursQuery q{};
      q.struct_size = sizeof(q);
      in >> q.neighbourhood >> q.flags >> q.palette >> q.birth >> q.survive;
      for (uint32_t& v : q.lo) in >> v;
      for (uint32_t& v : q.hi) in >> v;
      if (!in) return 2;
      dust::NeighbourArgs a{};
      bool empty = false;
      uint32_t byte = 777, majority = 777;
      if (dust::device_neighbours(q, a, byte, majority, empty) != nullptr) {
        std::printf("q 0\n");
        continue;
      }
      std::printf("q 1 %u %u %u %u %u %u %u", empty ? 1u : 0u, a.neighbourhood, a.walls, a.birth, a.survive, byte, majority);
      if (!empty)
        std::printf(" %u %u %u %u %u %u %u %u %u %u %u %u", a.lo[0], a.lo[1], a.lo[2], a.hi[0], a.hi[1], a.hi[2], a.box.lo[0], a.box.lo[1], a.box.lo[2], a.box.hi[0],
                    a.box.hi[1], a.box.hi[2]);
      std::printf("\n");
    } else if (what == "a") {
      uint32_t generations = 0;
      in >> generations;
      if (!in) return 2;
      std::printf("a %u\n", dust::neighbours_apply_arguments(generations) == nullptr ? 1u : 0u);
    } else if (what == "r") {
      uint32_t acc[dust::kNeighbourAccWords] = {};
      uint32_t n = 0;
      while (n < dust::kNeighbourAccWords && (in >> acc[n])) ++n;
      if (n != 0 && n != dust::kNeighbourAccWords) return 2;
      DustHipNeighboursResult r;
      std::memset(&r, 0xEE, sizeof(r));  // (every byte of the output must be written)
      r = dust::neighbours_result(n ? acc : nullptr);
      uint32_t rest = r.pad0 | r.pad1;
      for (uint32_t v : r.reserved) rest |= v;
      std::printf("r %u %u %u %u %u %u %u %u %u %u %u\n", r.voxels, r.solid, r.born, r.died, r.lo[0], r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2], rest);
    } else if (what == "p") {
      uint32_t generations = 0, solid = 0;
      in >> generations;
      if (!in || generations == 0 || generations > dust::kNeighbourMaxGenerations) return 2;
      const bool given = bool(in >> solid);
      std::vector<uint32_t> slots(size_t(generations) * dust::kNeighbourSlotWords, 0u);
      if (given)
        for (uint32_t& v : slots) in >> v;
      if (!in && given) return 2;
      std::vector<uint32_t> rows(size_t(generations) * 2, 0xEEEEEEEEu);
      DustHipNeighboursApplied r;
      std::memset(&r, 0xEE, sizeof(r));
      r = dust::neighbours_applied(given ? slots.data() : nullptr, generations, solid, rows.data());
      uint32_t rest = r.pad0 | r.pad1 | r.reserved0;
      for (uint32_t v : r.reserved) rest |= v;
      std::printf("p %u %u %u %" PRIu64 " %" PRIu64 " %u %u %u %u %u %u %u", r.generations, r.solid_before, r.solid_after, uint64_t(r.born), uint64_t(r.died), r.lo[0],
                  r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2], rest);
      for (uint32_t v : rows) std::printf(" %u", v);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
