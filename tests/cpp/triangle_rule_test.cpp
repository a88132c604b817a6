// triangle_rule_test.cpp -- the device-free half of model voxelisation driven on a CPU (tests/test_triangle_rule.py builds this with
// g++ under AddressSanitizer and UBSan and checks what it prints): dust_amd/csrc/triangle_rule.hpp -- the text k_edit_triangles and
// k_fill_columns run -- and device_triangle / device_fill_triangle / device_fill_mesh / fill_mesh_result of
// dust_amd/csrc/model_records.hpp. UBSan is the overflow check of the int64 arithmetic. Requests on stdin, answers on stdout; V[9] is
// the three vertices, x y z each:
//   s V[9] LO[3] HI[3]                   -> s N BITS...          triangle_covers of every voxel of the inclusive box, x slowest, as 0 / 1,
//                                                               behind their number; the coordinates may be negative. Where the 4^3
//                                                               brick test (triangle_touches_brick) says no and a voxel of the brick
//                                                               says yes the program fails: the early-out must never change an answer
//   c V[9] PX PY                         -> c CROSSED COUNT      column_crossed, and crossing_count (0 where n.z == 0)
//   t V[9] OP PALETTE                    -> t 0 | t 1 LO[3] HI[3] SOLID_TO EMPTY_TO      device_triangle
//   f V[9] LO[2] HI[2]                   -> f OK LIVE CROSSING [LO[2] HI[2]]             device_fill_triangle (the bounds when OK)
//   q OP PALETTE FLAGS R0 R1 LO[3] HI[3] -> q 0                  a refused query
//                                           q 1 EMPTY SOLID_TO EMPTY_TO [LO[3] HI[3] BOX_LO[3] BOX_HI[3]]   (the rest unless EMPTY)
//   r ACC[8] LIVE CROSSING   |   r       -> r COVERED CHANGED LIVE CROSSING LO[3] HI[3] RESERVED[2]
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "model_records.hpp"
#include "triangle_rule.hpp"

static bool read_vertices(std::istringstream& in, int32_t (&v)[3][3]) {
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) in >> v[k][r];
  return bool(in);
}
static int32_t floor_div4(int32_t v) { return v >= 0 ? v / 4 : -((-v + 3) / 4); }

int main() {
  char buffer[1 << 16];
  while (std::fgets(buffer, sizeof(buffer), stdin)) {
    std::istringstream in(buffer);
    std::string what;
    if (!(in >> what)) continue;
    DustHipTriangle tri{};
    if (what == "s") {
      int32_t lo[3], hi[3];
      if (!read_vertices(in, tri.v)) return 2;
      for (int r = 0; r < 3; ++r) in >> lo[r];
      for (int r = 0; r < 3; ++r) in >> hi[r];
      if (!in || !dust::triangle_in_range(tri.v)) return 2;
      const dust::TriangleSetup t = dust::triangle_setup(tri.v);
      if (dust::triangle_degenerate(t)) return 2;
      std::string bits;
      for (int32_t x = lo[0]; x <= hi[0]; ++x)
        for (int32_t y = lo[1]; y <= hi[1]; ++y)
          for (int32_t z = lo[2]; z <= hi[2]; ++z) {
            const bool in_voxel = dust::triangle_covers(t, x, y, z);
            if (in_voxel && !dust::triangle_touches_brick(t, floor_div4(x), floor_div4(y), floor_div4(z))) {
              std::fprintf(stderr, "the brick test rejects a brick with a covered voxel at %d %d %d\n", x, y, z);
              return 3;
            }
            bits += in_voxel ? " 1" : " 0";
          }
      std::printf("s %zu%s\n", bits.size() / 2, bits.c_str());
    } else if (what == "c") {
      int32_t px = 0, py = 0;
      if (!read_vertices(in, tri.v)) return 2;
      in >> px >> py;
      if (!in || !dust::triangle_in_range(tri.v)) return 2;
      const dust::TriangleColumn t = dust::triangle_column(tri.v);
      std::printf("c %d %u\n", dust::column_crossed(t, px, py) ? 1 : 0, t.s != 0 ? dust::crossing_count(t, px, py) : 0u);
    } else if (what == "t") {
      if (!read_vertices(in, tri.v)) return 2;
      in >> tri.op >> tri.palette;
      if (!in) return 2;
      dust::DevTriangle d{};
      if (!dust::device_triangle(tri, d)) { std::printf("t 0\n"); continue; }
      if (std::memcmp(d.v, tri.v, sizeof(d.v)) != 0) return 3;
      std::printf("t 1 %u %u %u %u %u %u %u %u\n", d.lo & 255u, (d.lo >> 8) & 255u, d.lo >> 16, d.hi & 255u, (d.hi >> 8) & 255u, d.hi >> 16, d.solid_to, d.empty_to);
    } else if (what == "f") {
      uint32_t lo[2], hi[2];
      if (!read_vertices(in, tri.v)) return 2;
      in >> lo[0] >> lo[1] >> hi[0] >> hi[1];
      if (!in) return 2;
      dust::DevTriangle d{};
      bool live = false, crossing = false;
      const bool ok = dust::device_fill_triangle(tri, lo, hi, d, live, crossing);
      std::printf("f %d %d %d", ok ? 1 : 0, live ? 1 : 0, crossing ? 1 : 0);
      if (ok) std::printf(" %u %u %u %u", d.lo & 255u, d.lo >> 8, d.hi & 255u, d.hi >> 8);
      std::printf("\n");
    } else if (what == "q") {
      DustHipFillMeshQuery q{};
      q.struct_size = sizeof(q);
      in >> q.op >> q.palette >> q.flags >> q.reserved[0] >> q.reserved[1];
      for (int r = 0; r < 3; ++r) in >> q.lo[r];
      for (int r = 0; r < 3; ++r) in >> q.hi[r];
      if (!in) return 2;
      dust::FillApplyArgs a{};
      bool empty = false;
      if (dust::device_fill_mesh(q, a, empty)) { std::printf("q 0\n"); continue; }
      std::printf("q 1 %d %u %u", empty ? 1 : 0, a.solid_to, a.empty_to);
      if (!empty) {
        for (int r = 0; r < 3; ++r) std::printf(" %u", a.lo[r]);
        for (int r = 0; r < 3; ++r) std::printf(" %u", a.hi[r]);
        for (int r = 0; r < 3; ++r) std::printf(" %u", a.box.lo[r]);
        for (int r = 0; r < 3; ++r) std::printf(" %u", a.box.hi[r]);
      }
      std::printf("\n");
    } else if (what == "r") {
      uint32_t acc[dust::kFillAccWords] = {}, live = 0, crossing = 0;
      bool given = true;
      for (uint32_t k = 0; k < dust::kFillAccWords; ++k) given = given && bool(in >> acc[k]);
      given = given && bool(in >> live >> crossing);
      const DustHipFillMeshResult r = dust::fill_mesh_result(given ? acc : nullptr, live, crossing);
      std::printf("r %u %u %u %u %u %u %u %u %u %u %u %u\n", r.covered, r.changed, r.live, r.crossing, r.lo[0], r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2],
                  r.reserved[0], r.reserved[1]);
    } else {
      return 2;
    }
  }
  return 0;
}
