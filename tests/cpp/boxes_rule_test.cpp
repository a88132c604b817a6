// boxes_rule_test.cpp -- the device-free half of the model boxes driven on a CPU (tests/test_boxes_rule.py builds this with g++ under
// AddressSanitizer and UBSan and checks what it prints): the functions of dust_amd/csrc/boxes_rule.hpp -- the text the kernels of
// boxes.hip run out of LDS and the D volume -- and device_boxes / boxes_result of dust_amd/csrc/model_records.hpp. Requests on stdin,
// answers on stdout:
//   pair ROWS STRIDE, then ROWS lines of F[8] J[8] K[8] PF[8] PJ[8] PK[8] SAME[8]
//                                        -> one line "q V0 U0 U1 V1 D" per rect start of the slice in the order of the walk (row by row),
//                                           D its bit of the D plane, then "end RECTS CONTINUED". F, J, K are the slice's planes, PF, PJ,
//                                           PK those of the slice before, SAME the voxels whose bytes agree across the two slices. The
//                                           planes are heap arrays of exactly 256 * STRIDE words (ASan sees a step past them), the rows
//                                           past ROWS clear, the pad words of a row set to a pattern that must not be read as bits.
//                                           Exit 3: the rule asked about the bytes of a voxel that is not a rect start of both slices
//   stack SLICES ROWS, then per slice ROWS lines of F[8] J[8] K[8] SAME[8] (SAME against the slice before)
//                                        -> one line "b S V0 U0 U1 V1 DEPTH" per box in ascending (s0, v0, u0), then "end BOXES": the
//                                           count pass and the list pass of boxes.hip in their order, over a D volume of exactly
//                                           SLICES planes that starts out with every bit set
//   depth LAST S V0 U0 N, then N triples T V U
//                                        -> depth DEPTH          boxes_depth over a D volume of exactly LAST + 1 planes (ASan sees a
//                                           walk past the region's last slice) in which the bits (T, V, U) are set
//   c N S U0 U1 V0 V1 DEPTH PALETTE      -> c RECORD             boxes_record
//   m AXIS FLAGS PALETTE LO[3] HI[3]     -> m 0                  a refused query
//                                           m 1 EMPTY AXIS BYTE ANY [LO[3] HI[3]]   (the rest unless EMPTY)
//   r ACC[9]   |   r                     -> r BOXES RECTS VOXELS LO[3] PAD0 HI[3] PAD1 RESERVED[11]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "boxes_rule.hpp"
#include "model_records.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "pair") {
      uint32_t rows = 0, stride = 0;
      in >> rows >> stride;
      if (rows > dust::kMeshExtent || stride < dust::kMeshRowWords || stride > 16u) return 2;
      const size_t words = size_t(dust::kMeshExtent) * stride;
      std::vector<uint32_t> plane[7];  // F J K PF PJ PK SAME
      for (auto& p : plane) {
        p.assign(words, 0u);
        for (uint32_t v = 0; v < dust::kMeshExtent; ++v)
          for (uint32_t w = dust::kMeshRowWords; w < stride; ++w) p[v * stride + w] = 0xA5A5A5A5u;
      }
      for (uint32_t v = 0; v < rows; ++v) {
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream row(line);
        for (auto& p : plane)
          for (uint32_t w = 0; w < dust::kMeshRowWords; ++w) row >> p[v * stride + w];
        if (!row) return 2;
      }
      // the continued run starts of both slices, row by row as the kernels make them (they write them over K)
      auto continued = [&](const std::vector<uint32_t>& f, const std::vector<uint32_t>& j, const std::vector<uint32_t>& k) {
        std::vector<uint32_t> c(words, 0u);
        for (uint32_t v = 0; v < dust::kMeshExtent; ++v)
          for (uint32_t w = 0; w < stride; ++w)
            c[v * stride + w] = w >= dust::kMeshRowWords ? 0xA5A5A5A5u
                                : v == 0u ? 0u
                                          : dust::mesh_continued_word(&f[v * stride], &j[v * stride], &k[v * stride], &f[(v - 1u) * stride], &j[(v - 1u) * stride], w);
        return c;
      };
      const std::vector<uint32_t>&f = plane[0], &j = plane[1], &pf = plane[3], &pj = plane[4], &same = plane[6];
      const std::vector<uint32_t> c = continued(f, j, plane[2]), pc = continued(pf, pj, plane[5]);
      uint32_t rects = 0, stacked = 0;
      for (uint32_t v = 0; v < dust::kMeshExtent; ++v)
        for (uint32_t w = 0; w < dust::kMeshRowWords; ++w) {
          const uint32_t at = v * stride + w;
          const uint32_t d = dust::boxes_continued_word(f.data(), j.data(), c.data(), pf.data(), pj.data(), pc.data(), stride, v, w, [&](uint32_t u0) {
            if ((u0 >> 5) != w || !dust::mesh_bit(&f[v * stride], u0) || !dust::mesh_bit(&pf[v * stride], u0)) std::exit(3);
            if (dust::mesh_bit(&j[v * stride], u0) || dust::mesh_bit(&c[v * stride], u0) || dust::mesh_bit(&pj[v * stride], u0) || dust::mesh_bit(&pc[v * stride], u0)) std::exit(3);
            return dust::mesh_bit(&same[v * stride], u0);
          });
          if ((d & ~(f[at] & ~j[at] & ~c[at])) != 0u) return 3;  // (D has bits at rect starts only)
          for (uint32_t starts = f[at] & ~j[at] & ~c[at]; starts != 0u; starts &= starts - 1u) {
            const uint32_t u0 = (w << 5) + dust::mesh_ctz(starts);
            std::printf("q %u %u %u %u %u\n", v, u0, dust::mesh_run_end(&j[v * stride], u0), dust::boxes_rect_end(c.data(), stride, v, u0), (d >> (u0 & 31u)) & 1u);
            ++rects;
          }
          stacked += uint32_t(__builtin_popcount(d));
        }
      std::printf("end %u %u\n", rects, stacked);
    } else if (what == "stack") {
      // the two passes of boxes.hip in their order: every slice's D plane into a volume of exactly SLICES planes (the first all clear),
      // then per slice the box starts -- rect starts whose D bit is clear -- with their run end, rect end and depth
      uint32_t slices = 0, rows = 0;
      in >> slices >> rows;
      if (slices == 0u || slices > dust::kMeshExtent || rows > dust::kMeshExtent) return 2;
      const uint32_t stride = dust::kMeshRowWords;
      const size_t words = dust::kBoxesPlaneWords;
      std::vector<std::vector<uint32_t>> f(slices), j(slices), c(slices);
      std::vector<uint32_t> dvol(size_t(slices) * words, 0xFFFFFFFFu);  // (stale bits everywhere: every plane must be written)
      for (uint32_t s = 0; s < slices; ++s) {
        std::vector<uint32_t> k(words, 0u), same(words, 0u);
        f[s].assign(words, 0u); j[s].assign(words, 0u); c[s].assign(words, 0u);
        for (uint32_t v = 0; v < rows; ++v) {
          if (!std::getline(std::cin, line)) return 2;
          std::istringstream row(line);
          for (std::vector<uint32_t>* p : {&f[s], &j[s], &k, &same})
            for (uint32_t w = 0; w < stride; ++w) row >> (*p)[v * stride + w];
          if (!row) return 2;
        }
        for (uint32_t v = 1; v < dust::kMeshExtent; ++v)
          for (uint32_t w = 0; w < stride; ++w)
            c[s][v * stride + w] = dust::mesh_continued_word(&f[s][v * stride], &j[s][v * stride], &k[v * stride], &f[s][(v - 1u) * stride], &j[s][(v - 1u) * stride], w);
        for (uint32_t v = 0; v < dust::kMeshExtent; ++v)
          for (uint32_t w = 0; w < stride; ++w)
            dvol[s * words + v * stride + w] =
                s == 0u ? 0u
                        : dust::boxes_continued_word(f[s].data(), j[s].data(), c[s].data(), f[s - 1u].data(), j[s - 1u].data(), c[s - 1u].data(), stride, v, w,
                                                     [&](uint32_t u0) { return dust::mesh_bit(&same[v * stride], u0); });
      }
      uint32_t boxes = 0;
      for (uint32_t s = 0; s < slices; ++s)
        for (uint32_t v = 0; v < dust::kMeshExtent; ++v)
          for (uint32_t w = 0; w < stride; ++w) {
            const uint32_t at = v * stride + w;
            for (uint32_t rest = f[s][at] & ~j[s][at] & ~c[s][at] & ~dvol[s * words + at]; rest != 0u; rest &= rest - 1u) {
              const uint32_t u0 = (w << 5) + dust::mesh_ctz(rest);
              std::printf("b %u %u %u %u %u %u\n", s, v, u0, dust::mesh_run_end(&j[s][v * stride], u0), dust::boxes_rect_end(c[s].data(), stride, v, u0),
                          dust::boxes_depth(dvol.data(), s, slices - 1u, v, u0));
              ++boxes;
            }
          }
      std::printf("end %u\n", boxes);
    } else if (what == "depth") {
      uint32_t last = 0, s = 0, v0 = 0, u0 = 0, n = 0;
      in >> last >> s >> v0 >> u0 >> n;
      if (last >= dust::kMeshExtent || s > last || v0 >= dust::kMeshExtent || u0 >= dust::kMeshExtent) return 2;
      std::vector<uint32_t> dvol(size_t(last + 1u) * dust::kBoxesPlaneWords, 0u);
      for (uint32_t k = 0; k < n; ++k) {
        uint32_t t = 0, v = 0, u = 0;
        in >> t >> v >> u;
        if (!in || t > last || v >= dust::kMeshExtent || u >= dust::kMeshExtent) return 2;
        dvol[size_t(t) * dust::kBoxesPlaneWords + v * dust::kMeshRowWords + (u >> 5)] |= 1u << (u & 31u);
      }
      std::printf("depth %u\n", dust::boxes_depth(dvol.data(), s, last, v0, u0));
    } else if (what == "c") {
      uint32_t v[8] = {};
      for (uint32_t& x : v) in >> x;
      std::printf("c %" PRIu64 "\n", dust::boxes_record(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]));
    } else if (what == "m") {
      DustHipBoxesQuery q{};
      q.struct_size = sizeof(q);
      in >> q.axis >> q.flags >> q.palette;
      for (uint32_t& v : q.lo) in >> v;
      for (uint32_t& v : q.hi) in >> v;
      dust::BoxesArgs a{};
      bool empty = false;
      if (dust::device_boxes(q, a, empty) != nullptr) {
        std::printf("m 0\n");
        continue;
      }
      std::printf("m 1 %u %u %u %u", empty ? 1u : 0u, a.axis, a.byte, a.any_palette);
      if (!empty) {
        for (uint32_t v : a.lo) std::printf(" %u", v);
        for (uint32_t v : a.hi) std::printf(" %u", v);
      }
      std::printf("\n");
    } else if (what == "r") {
      uint32_t acc[dust::kBoxesAccWords] = {};
      uint32_t n = 0;
      while (n < dust::kBoxesAccWords && (in >> acc[n])) ++n;
      if (n != 0 && n != dust::kBoxesAccWords) return 2;
      DustHipBoxesResult r;
      std::memset(&r, 0xEE, sizeof(r));  // (every byte of the output must be written)
      r = dust::boxes_result(n ? acc : nullptr);
      std::printf("r %u %u %u %u %u %u %u %u %u %u %u", r.boxes, r.rects, r.voxels, r.lo[0], r.lo[1], r.lo[2], r.pad0, r.hi[0], r.hi[1], r.hi[2], r.pad1);
      for (uint32_t v : r.reserved) std::printf(" %u", v);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
