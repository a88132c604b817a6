// delta_rule_test.cpp -- the device-free half of the model deltas driven on a CPU (tests/test_delta_rule.py builds this with g++ under
// AddressSanitizer and UBSan and checks what it prints): delta_words and delta_listed of dust_amd/csrc/delta_rule.hpp -- the text the
// kernels of delta.hip run per brick -- and device_delta / delta_result / delta_apply_records of dust_amd/csrc/model_records.hpp. One
// request per line of stdin, one answer per line of stdout:
//   w MA MB BX BY BZ LO[3] HI[3] KINDS DIFFERS FILTER -> w SOLID_BEFORE SOLID_AFTER ADDED REMOVED CANDIDATES L_ADDED L_REMOVED L_REPAINTED LISTED
//   q KINDS FLAGS PALETTE LO[3] HI[3]    -> q 0                   a refused query
//                                           q 1 EMPTY KINDS BYTE [LO[3] HI[3] BOXLO[3] BOXHI[3]]   (the rest unless EMPTY)
//   r ACC[11]   |   r                    -> r VOXELS ADDED REMOVED REPAINTED SOLID_BEFORE SOLID_AFTER LO[3] HI[3] NONZERO   (NONZERO: pad and reserved bytes set)
//   a N (KEY KIND BEFORE AFTER) * N      -> a 0                   refused records
//                                           a 1 M WORD * M        the surviving records as the kernel's words, in the order it gets them
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "delta_rule.hpp"
#include "model_records.hpp"

int main() {
  std::string line;
  char buf[1 << 16];
  while (std::fgets(buf, sizeof(buf), stdin)) {
    line = buf;
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "w") {
      uint64_t mA = 0, mB = 0, differs = 0, filter = 0;
      uint32_t b[3] = {}, lo[3] = {}, hi[3] = {}, kinds = 0;
      in >> mA >> mB;
      for (uint32_t& v : b) in >> v;
      for (uint32_t& v : lo) in >> v;
      for (uint32_t& v : hi) in >> v;
      in >> kinds >> differs >> filter;
      const dust::DeltaWords w = dust::delta_words(mA, mB, dust::surface_region_mask(b[0], b[1], b[2], lo, hi), kinds);
      const dust::DeltaListed l = dust::delta_listed(w, differs, filter);
      std::printf("w %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", w.solid_before,
                  w.solid_after, w.added, w.removed, w.candidates, l.added, l.removed, l.repainted, l.listed);
    } else if (what == "q") {
      DustHipDeltaQuery q{};
      q.struct_size = sizeof(q);
      in >> q.kinds >> q.flags >> q.palette;
      for (uint32_t& v : q.lo) in >> v;
      for (uint32_t& v : q.hi) in >> v;
      dust::DeltaArgs a{};
      bool empty = false;
      if (dust::device_delta(q, a, empty) != nullptr) {
        std::printf("q 0\n");
        continue;
      }
      std::printf("q 1 %u %u %u", empty ? 1u : 0u, a.kinds, a.byte);
      if (!empty) {
        for (uint32_t v : a.lo) std::printf(" %u", v);
        for (uint32_t v : a.hi) std::printf(" %u", v);
        for (uint32_t v : a.box.lo) std::printf(" %u", v);
        for (uint32_t v : a.box.hi) std::printf(" %u", v);
      }
      std::printf("\n");
    } else if (what == "r") {
      uint32_t acc[dust::kDeltaAccWords] = {};
      uint32_t n = 0;
      while (n < dust::kDeltaAccWords && (in >> acc[n])) ++n;
      if (n != 0 && n != dust::kDeltaAccWords) return 2;
      DustHipDeltaResult r;
      std::memset(&r, 0xEE, sizeof(r));  // (every byte of the output must be written)
      r = dust::delta_result(n ? acc : nullptr);
      std::printf("r %u %u %u %u %u %u %u %u %u %u %u %u", r.voxels, r.added, r.removed, r.repainted, r.solid_before, r.solid_after, r.lo[0], r.lo[1],
                  r.lo[2], r.hi[0], r.hi[1], r.hi[2]);
      uint32_t rest = r.pad0 | r.pad1;
      for (uint32_t v : r.reserved) rest |= v;
      std::printf(" %u\n", rest);
    } else if (what == "a") {
      uint32_t n = 0;
      in >> n;
      std::vector<DustHipDeltaVoxel> records(n);  // (exactly n: a read past the end is the sanitizer's to find)
      for (DustHipDeltaVoxel& v : records) {
        uint32_t kind = 0, before = 0, after = 0;
        in >> v.key >> kind >> before >> after;
        v.kind = uint8_t(kind); v.before = uint8_t(before); v.after = uint8_t(after); v.reserved = 0;
      }
      if (!in) return 2;
      std::vector<uint64_t> words;
      if (dust::delta_apply_records(records.data(), n, words) != nullptr) {
        std::printf("a 0\n");
        continue;
      }
      std::printf("a 1 %zu", words.size());
      for (uint64_t w : words) std::printf(" %" PRIu64, w);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
