// column_rule_test.cpp -- the device-free half of the model columns driven on a CPU (tests/test_column_rule.py builds this with g++ under
// AddressSanitizer and UBSan and checks what it prints): column_turn, column_run, column_span, column_cell, column_nibble and the key
// words of dust_amd/csrc/column_rule.hpp -- the text the kernels of column.hip run per lane -- and device_columns /
// columns_apply_arguments / columns_result of dust_amd/csrc/model_records.hpp. One request per line of stdin, one answer per line of
// stdout:
//   c W[4] LO HI FROM_HIGH LAYER WHERE DEPTH -> c AT LENGTH GAP RUNS COORD CELL FIRST COUNT   (W: the column in coordinate order; AT 256: a miss)
//   n WORD OFF STRIDE                        -> n NIBBLE
//   k DEPTH KEY                              -> k NEAR_WORD FAR_WORD NEAR_KEY FAR_KEY
//   q FACE FLAGS PALETTE LO[3] HI[3] LAYER RESERVED -> q 0        a refused query
//                                               q 1 EMPTY AXIS FROM_HIGH BYTE LAYER NU NV [LO_N HI_N LO_U HI_U LO_V HI_V CELL_U CELL_V CELLS_U CELLS_V]
//   a WHERE DEPTH VALUE                      -> a 0 | a 1         refused or not
//   r NU NV ACC[12]   |   r                  -> r COLUMNS HIT VOXELS RUNS DEPTH_SUM NEAREST FARTHEST LO[3] HI[3] NONZERO   (NONZERO: pad and reserved bytes set)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

#include "column_rule.hpp"
#include "model_records.hpp"

int main() {
  std::string line;
  char buf[1 << 12];
  while (std::fgets(buf, sizeof(buf), stdin)) {
    line = buf;
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "c") {
      dust::Column raw{};
      uint32_t lo = 0, hi = 0, from_high = 0, layer = 0, where = 0, depth = 0;
      for (uint64_t& w : raw.w) in >> w;
      in >> lo >> hi >> from_high >> layer >> where >> depth;
      if (!in) return 2;
      const dust::Column occ = dust::column_turn(raw, lo, hi, from_high != 0);
      const dust::ColumnRun r = dust::column_run(occ, layer);
      const dust::ColumnSpan s = dust::column_span(r, where, depth);
      const uint32_t coord = r.at == dust::kColumnBits ? 0u : dust::column_coord(r.at, lo, hi, from_high != 0);
      std::printf("c %u %u %u %u %u %u %u %u\n", r.at, r.length, r.gap, r.runs, coord, dust::column_cell(coord, 7u, r), s.first, s.count);
    } else if (what == "n") {
      uint64_t word = 0;
      uint32_t off = 0, stride = 0;
      in >> word >> off >> stride;
      if (!in) return 2;
      std::printf("n %u\n", dust::column_nibble(word, off, stride));
    } else if (what == "k") {
      uint32_t depth = 0, key = 0;
      in >> depth >> key;
      if (!in) return 2;
      const uint32_t near = dust::column_near_word(depth, key), far = dust::column_far_word(depth, key);
      std::printf("k %u %u %u %u\n", near, far, dust::column_near_key(near), dust::column_far_key(far));
    } else if (what == "q") {
      DustHipColumnsQuery q{};
      q.struct_size = sizeof(q);
      in >> q.face >> q.flags >> q.palette;
      for (uint32_t& v : q.lo) in >> v;
      for (uint32_t& v : q.hi) in >> v;
      in >> q.layer >> q.reserved;
      if (!in) return 2;
      dust::ColumnArgs a{};
      bool empty = false;
      uint32_t nu = 77, nv = 77;
      if (dust::device_columns(q, a, empty, nu, nv) != nullptr) {
        std::printf("q 0\n");
        continue;
      }
      std::printf("q 1 %u %u %u %u %u %u %u", empty ? 1u : 0u, a.axis, a.from_high, a.byte, a.layer, nu, nv);
      if (!empty) std::printf(" %u %u %u %u %u %u %u %u %u %u", a.lo_n, a.hi_n, a.lo_u, a.hi_u, a.lo_v, a.hi_v, a.cell_u, a.cell_v, a.cells_u, a.cells_v);
      std::printf("\n");
    } else if (what == "a") {
      uint32_t where = 0, depth = 0;
      int32_t value = 0;
      in >> where >> depth >> value;
      if (!in) return 2;
      std::printf("a %u\n", dust::columns_apply_arguments(where, depth, value) == nullptr ? 1u : 0u);
    } else if (what == "r") {
      uint32_t nu = 0, nv = 0, acc[dust::kColumnAccWords] = {};
      uint32_t n = 0;
      const bool given = bool(in >> nu >> nv);
      while (given && n < dust::kColumnAccWords && (in >> acc[n])) ++n;
      if (given && n != dust::kColumnAccWords) return 2;
      DustHipColumnsResult r;
      std::memset(&r, 0xEE, sizeof(r));  // (every byte of the output must be written)
      r = dust::columns_result(given ? acc : nullptr, nu, nv);
      std::printf("r %u %u %u %u %u %u %u %u %u %u %u %u %u", r.columns, r.hit, r.voxels, r.runs, r.depth_sum, r.nearest_key, r.farthest_key, r.lo[0], r.lo[1],
                  r.lo[2], r.hi[0], r.hi[1], r.hi[2]);
      uint32_t rest = r.pad0 | r.pad1;
      for (uint32_t v : r.reserved) rest |= v;
      std::printf(" %u\n", rest);
    } else {
      return 2;
    }
  }
  return 0;
}
