// surface_rule_test.cpp -- the device-free half of the model surfaces driven on a CPU (tests/test_surface_rule.py builds this with g++
// under AddressSanitizer and UBSan and checks what it prints): surface_exposure and surface_region_mask of
// dust_amd/csrc/surface_rule.hpp -- the text the kernels of surface.hip run per brick -- and device_surface / surface_result of
// dust_amd/csrc/model_records.hpp. One request per line of stdin, one answer per line of stdout:
//   e OWN NX PX NY PY NZ PZ              -> e E0 .. E5            the six exposure words
//   m BX BY BZ LO[3] HI[3]               -> m MASK                the part of an inclusive region brick (BX, BY, BZ) holds
//   q FACES FLAGS PALETTE LO[3] HI[3]    -> q 0                   a refused query
//                                           q 1 EMPTY FACES WALLS BYTE [LO[3] HI[3] BOXLO[3] BOXHI[3]]   (the rest unless EMPTY)
//   r ACC[14]   |   r                    -> r VOXELS FACES BY_FACE[6] SOLID LO[3] HI[3] NONZERO   (NONZERO: pad and reserved bytes set)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

#include "model_records.hpp"
#include "surface_rule.hpp"

int main() {
  char line[1024];
  while (std::fgets(line, sizeof(line), stdin)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "e") {
      uint64_t w[7] = {};
      for (uint64_t& v : w) in >> v;
      const dust::SurfaceWords s = dust::surface_exposure(w[0], w[1], w[2], w[3], w[4], w[5], w[6]);
      std::printf("e");
      for (uint64_t v : s.e) std::printf(" %" PRIu64, v);
      std::printf("\n");
    } else if (what == "m") {
      uint32_t b[3] = {}, lo[3] = {}, hi[3] = {};
      for (uint32_t& v : b) in >> v;
      for (uint32_t& v : lo) in >> v;
      for (uint32_t& v : hi) in >> v;
      std::printf("m %" PRIu64 "\n", dust::surface_region_mask(b[0], b[1], b[2], lo, hi));
    } else if (what == "q") {
      DustHipSurfaceQuery q{};
      q.struct_size = sizeof(q);
      in >> q.faces >> q.flags >> q.palette;
      for (uint32_t& v : q.lo) in >> v;
      for (uint32_t& v : q.hi) in >> v;
      dust::SurfaceArgs a{};
      bool empty = false;
      if (dust::device_surface(q, a, empty) != nullptr) {
        std::printf("q 0\n");
        continue;
      }
      std::printf("q 1 %u %u %u %u", empty ? 1u : 0u, a.faces, a.walls, a.byte);
      if (!empty) {
        for (uint32_t v : a.lo) std::printf(" %u", v);
        for (uint32_t v : a.hi) std::printf(" %u", v);
        for (uint32_t v : a.box.lo) std::printf(" %u", v);
        for (uint32_t v : a.box.hi) std::printf(" %u", v);
      }
      std::printf("\n");
    } else if (what == "r") {
      uint32_t acc[dust::kSurfaceAccWords] = {};
      uint32_t n = 0;
      while (n < dust::kSurfaceAccWords && (in >> acc[n])) ++n;
      if (n != 0 && n != dust::kSurfaceAccWords) return 2;
      DustHipSurfaceResult r;
      std::memset(&r, 0xEE, sizeof(r));  // (every byte of the output must be written)
      r = dust::surface_result(n ? acc : nullptr);
      std::printf("r %u %u", r.voxels, r.faces);
      for (uint32_t v : r.by_face) std::printf(" %u", v);
      std::printf(" %u %u %u %u %u %u %u", r.solid, r.lo[0], r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2]);
      uint32_t rest = r.pad0 | r.pad1;
      for (uint32_t v : r.reserved) rest |= v;
      std::printf(" %u\n", rest);
    } else {
      return 2;
    }
  }
  return 0;
}
