// mesh_rule_test.cpp -- the device-free half of the model meshes driven on a CPU (tests/test_mesh_rule.py builds this with g++ under
// AddressSanitizer and UBSan and checks what it prints): the row functions of dust_amd/csrc/mesh_rule.hpp -- the text the kernels of
// mesh.hip run out of LDS -- and device_mesh / mesh_result of dust_amd/csrc/model_records.hpp. Requests on stdin, answers on stdout:
//   slice ROWS STRIDE HEIGHTS, then ROWS lines of F[8] J[8] K[8]
//                                        -> one line "q V0 U0 U1 V1" per quad in the order of the walk (row by row), then "end N".
//                                           The planes are heap arrays of exactly 256 * STRIDE words (ASan sees a step past them), the
//                                           rows past ROWS clear, the pad words of a row set to a pattern the walk must not read as bits
//   j F[8]                               -> j J[8]               mesh_join_any of every word
//   e U0 J[8]                            -> e U1                 mesh_run_end
//   n WORD N C                           -> n NIBBLE[4]          mesh_row_nibble of rows 0..3
//   p N C                                -> p PLANE              mesh_slice_plane
//   x OWN ACROSS D                       -> x E                  mesh_exposure
//   a N S U V                            -> a X Y Z              mesh_x, mesh_y, mesh_z
//   c D S U0 U1 V0 V1 PALETTE            -> c RECORD             mesh_record
//   m FACES FLAGS PALETTE LO[3] HI[3]    -> m 0                  a refused query
//                                           m 1 EMPTY FACES WALLS BYTE ANY [LO[3] HI[3]]   (the rest unless EMPTY)
//   r ACC[13]   |   r                    -> r QUADS FACES QUADS_BY_FACE[6] FACES_BY_FACE[6] LARGEST RESERVED
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "mesh_rule.hpp"
#include "model_records.hpp"

int main() {
  char line[4096];
  while (std::fgets(line, sizeof(line), stdin)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "slice") {
      uint32_t rows = 0, stride = 0, heights = 0;
      in >> rows >> stride >> heights;
      if (rows > dust::kMeshExtent || stride < dust::kMeshRowWords || stride > 16u) return 2;
      const size_t words = size_t(dust::kMeshExtent) * stride;
      std::vector<uint32_t> f(words, 0u), j(words, 0u), k(words, 0u);
      for (uint32_t v = 0; v < dust::kMeshExtent; ++v)
        for (uint32_t w = dust::kMeshRowWords; w < stride; ++w) f[v * stride + w] = j[v * stride + w] = k[v * stride + w] = 0xA5A5A5A5u;
      for (uint32_t v = 0; v < rows; ++v) {
        if (!std::fgets(line, sizeof(line), stdin)) return 2;
        std::istringstream row(line);
        for (uint32_t w = 0; w < dust::kMeshRowWords; ++w) row >> f[v * stride + w];
        for (uint32_t w = 0; w < dust::kMeshRowWords; ++w) row >> j[v * stride + w];
        for (uint32_t w = 0; w < dust::kMeshRowWords; ++w) row >> k[v * stride + w];
        if (!row) return 2;
      }
      std::vector<uint32_t> c(words, 0u);  // the continued run starts, row by row as the kernels make them (they write them over K)
      for (uint32_t v = 0; v < dust::kMeshExtent; ++v)
        for (uint32_t w = 0; w < stride; ++w)
          c[v * stride + w] = w >= dust::kMeshRowWords ? 0xA5A5A5A5u
                              : v == 0u ? 0u
                                        : dust::mesh_continued_word(&f[v * stride], &j[v * stride], &k[v * stride], &f[(v - 1u) * stride], &j[(v - 1u) * stride], w);
      uint32_t total = 0;
      for (uint32_t v = 0; v < dust::kMeshExtent; ++v)
        total += dust::mesh_row_quads(f.data(), j.data(), c.data(), stride, v, heights != 0u,
                                      [&](uint32_t u0, uint32_t u1, uint32_t v1) { std::printf("q %u %u %u %u\n", v, u0, u1, v1); });
      std::printf("end %u\n", total);
    } else if (what == "j") {
      uint32_t f[dust::kMeshRowWords] = {};
      for (uint32_t& v : f) in >> v;
      std::printf("j");
      for (uint32_t w = 0; w < dust::kMeshRowWords; ++w) std::printf(" %u", dust::mesh_join_any(f, w));
      std::printf("\n");
    } else if (what == "e") {
      uint32_t u0 = 0, j[dust::kMeshRowWords] = {};
      in >> u0;
      for (uint32_t& v : j) in >> v;
      std::printf("e %u\n", dust::mesh_run_end(j, u0));
    } else if (what == "n") {
      uint64_t word = 0;
      uint32_t n = 0, c = 0;
      in >> word >> n >> c;
      std::printf("n %u %u %u %u\n", dust::mesh_row_nibble(word, n, c, 0), dust::mesh_row_nibble(word, n, c, 1), dust::mesh_row_nibble(word, n, c, 2),
                  dust::mesh_row_nibble(word, n, c, 3));
    } else if (what == "p") {
      uint32_t n = 0, c = 0;
      in >> n >> c;
      std::printf("p %" PRIu64 "\n", dust::mesh_slice_plane(n, c));
    } else if (what == "x") {
      uint64_t own = 0, across = 0;
      uint32_t d = 0;
      in >> own >> across >> d;
      std::printf("x %" PRIu64 "\n", dust::mesh_exposure(own, across, d));
    } else if (what == "a") {
      uint32_t n = 0, s = 0, u = 0, v = 0;
      in >> n >> s >> u >> v;
      std::printf("a %u %u %u\n", dust::mesh_x(n, s, u, v), dust::mesh_y(n, s, u, v), dust::mesh_z(n, s, u, v));
    } else if (what == "c") {
      uint32_t v[7] = {};
      for (uint32_t& x : v) in >> x;
      std::printf("c %" PRIu64 "\n", dust::mesh_record(v[0], v[1], v[2], v[3], v[4], v[5], v[6]));
    } else if (what == "m") {
      DustHipMeshQuery q{};
      q.struct_size = sizeof(q);
      in >> q.faces >> q.flags >> q.palette;
      for (uint32_t& v : q.lo) in >> v;
      for (uint32_t& v : q.hi) in >> v;
      dust::MeshArgs a{};
      bool empty = false;
      if (dust::device_mesh(q, a, empty) != nullptr) {
        std::printf("m 0\n");
        continue;
      }
      std::printf("m 1 %u %u %u %u %u", empty ? 1u : 0u, a.faces, a.walls, a.byte, a.any_palette);
      if (!empty) {
        for (uint32_t v : a.lo) std::printf(" %u", v);
        for (uint32_t v : a.hi) std::printf(" %u", v);
      }
      std::printf("\n");
    } else if (what == "r") {
      uint32_t acc[dust::kMeshAccWords] = {};
      uint32_t n = 0;
      while (n < dust::kMeshAccWords && (in >> acc[n])) ++n;
      if (n != 0 && n != dust::kMeshAccWords) return 2;
      DustHipMeshResult r;
      std::memset(&r, 0xEE, sizeof(r));  // (every byte of the output must be written)
      r = dust::mesh_result(n ? acc : nullptr);
      std::printf("r %u %u", r.quads, r.faces);
      for (uint32_t v : r.quads_by_face) std::printf(" %u", v);
      for (uint32_t v : r.faces_by_face) std::printf(" %u", v);
      std::printf(" %u %u\n", r.largest, r.reserved);
    } else {
      return 2;
    }
  }
  return 0;
}
