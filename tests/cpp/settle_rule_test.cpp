// settle_rule_test.cpp -- the device-free half of the model settling driven on a CPU (tests/test_settle_rule.py builds this with g++
// under AddressSanitizer and UBSan and checks what it prints): settle_fall, settle_destination, settle_walk and settle_slide of
// dust_amd/csrc/settle_rule.hpp -- the text the kernels of settle.hip run per lane and per brick -- held to bit loops written here, and
// device_settle / settle_apply_arguments / settle_result / settle_applied / settle_at_rest of dust_amd/csrc/model_records.hpp.
//   settle_rule_test fall SEED    -> fall COLUMNS MOVED      hand-made and random columns against a loop over the 256 positions
//   settle_rule_test slide SEED   -> slide BRICKS SLID       random 12^3 worlds, every direction pair, against a loop over the voxels
//   settle_rule_test records      -> one line per request of stdin:
//     q TOWARD FLAGS RESERVED LO[3] HI[3] LOOSE[8] -> q 0  a refused query
//                                                     q 1 EMPTY ALL_LOOSE AXIS FROM_HIGH NU NV [LO_N HI_N LO_U HI_U LO_V HI_V CELL_U CELL_V CELLS_U CELLS_V BOX_LO[3] BOX_HI[3]]
//     g GENERATIONS                                -> g 0 | g 1     refused or not
//     d AXIS K                                     -> d D_AXIS D_UP
//     r NU NV ACC[14]   |   r                      -> r COLUMNS LOOSE FIXED MOVED CHANGED FALL_MAX FALL_SUM LO[3] HI[3] CHANGED_COLUMNS NONZERO
//     a GENERATIONS N WORDS[N]  |  a GENERATIONS   -> a GENERATIONS FIRST_MOVED LOOSE SLID FELL FALL_SUM LO[3] HI[3] NONZERO AT_REST ROWS[2 * GENERATIONS]
//                                                     (the first N words of the record array, the rest 0; AT_REST: settle_at_rest of all generations)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "model_records.hpp"
#include "settle_rule.hpp"

namespace {

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(3);                                                       \
    }                                                                     \
  } while (0)

bool bit(const dust::Column& c, uint32_t p) { return (c.w[p >> 6] >> (p & 63u)) & 1ull; }
void set(dust::Column& c, uint32_t p) { c.w[p >> 6] |= 1ull << (p & 63u); }

// one column against the loop over its positions; returns the loose voxels moved
uint32_t check_column(const dust::Column& loose, const dust::Column& fixed) {
  dust::Column now{};
  uint32_t to[256];
  uint32_t next = 0, n_loose = 0, n_fixed = 0, moved = 0, fall_sum = 0, fall_max = 0;
  for (uint32_t p = 0; p < 256u; ++p) {
    to[p] = 256u;
    if (bit(fixed, p)) { next = p + 1u; ++n_fixed; continue; }
    if (!bit(loose, p)) continue;
    ++n_loose;
    to[p] = next;
    set(now, next);
    if (next != p) { ++moved; fall_sum += p - next; fall_max = std::max(fall_max, p - next); }
    ++next;
  }
  const dust::SettleFall f = dust::settle_fall(loose, fixed);
  for (int k = 0; k < 4; ++k) CHECK(f.now.w[k] == now.w[k]);
  CHECK(f.loose == n_loose && f.fixed == n_fixed && f.moved == moved && f.fall_sum == fall_sum && f.fall_max == fall_max);
  uint32_t sum = 0, first = 256u, last = 256u;
  for (uint32_t p = 0; p < 256u; ++p)
    if (bit(loose, p)) { sum += p; if (first == 256u) first = p; last = p; }
  CHECK(dust::column_position_sum(loose) == sum && dust::column_first(loose) == first && dust::column_last(loose) == last);
  for (uint32_t p = 0; p < 256u; ++p)
    if (bit(loose, p)) CHECK(dust::settle_destination(loose, fixed, p) == to[p]);
  // the walk: ascending, every moved voxel once, a destination never above a voxel not yet visited -- played on bytes in place
  uint8_t bytes[256], want[256];
  for (uint32_t p = 0; p < 256u; ++p) { bytes[p] = bit(loose, p) ? uint8_t(1u + p % 200u) : (bit(fixed, p) ? 255 : 0); want[p] = bit(fixed, p) ? 255 : 0; }
  for (uint32_t p = 0; p < 256u; ++p)
    if (bit(loose, p)) want[to[p]] = uint8_t(1u + p % 200u);
  uint32_t walked = 0, previous = 0;
  dust::settle_walk(loose, fixed, [&](uint32_t from, uint32_t dest) {
    CHECK(from < 256u && dest < from && to[from] == dest && (walked == 0u || from > previous));
    bytes[dest] = bytes[from];
    bytes[from] = 0;
    previous = from;
    ++walked;
  });
  CHECK(walked == moved && std::memcmp(bytes, want, 256) == 0);
  return moved;
}

int run_fall(uint32_t seed) {
  std::mt19937_64 rng(seed);
  uint32_t columns = 0, moved = 0;
  auto both = [&](const dust::Column& solid, const dust::Column& loose_of) {  // loose = solid & loose_of
    dust::Column loose = dust::column_and(solid, loose_of), fixed = dust::column_xor(solid, loose);
    moved += check_column(loose, fixed);
    ++columns;
  };
  const dust::Column none{}, all{{~0ull, ~0ull, ~0ull, ~0ull}};
  dust::Column even{}, odd{};
  for (uint32_t p = 0; p < 256u; p += 2u) { set(even, p); set(odd, p + 1u); }
  const dust::Column hand[4] = {none, all, even, odd};
  for (const dust::Column& solid : hand)
    for (const dust::Column& loose : hand) both(solid, loose);
  for (uint32_t edge : {0u, 1u, 62u, 63u, 64u, 65u, 126u, 127u, 128u, 129u, 190u, 191u, 192u, 193u, 254u, 255u}) {  // a fixed voxel at every word edge
    dust::Column fixed{}, loose = all;
    set(fixed, edge);
    loose.w[edge >> 6] &= ~(1ull << (edge & 63u));
    moved += check_column(loose, fixed);
    moved += check_column(dust::column_and(loose, even), fixed);
    moved += check_column(dust::column_and(loose, odd), fixed);
    dust::Column high{};  // a loose run high above the fixed voxel, across the word edges
    for (uint32_t p = 0; p < 256u; ++p)
      if (p > edge + 40u) set(high, p);
    moved += check_column(high, fixed);
    columns += 4;
  }
  for (uint32_t a = 0; a <= 256u; a += 37u)
    for (uint32_t b = a; b <= 256u; b += 29u) {
      const dust::Column r = dust::column_range(a, b);
      for (uint32_t p = 0; p < 256u; ++p) CHECK(bit(r, p) == (p >= a && p < b));
    }
  for (uint32_t n = 0; n < 4000u; ++n) {
    const uint32_t density = uint32_t(rng() % 5u), share = uint32_t(rng() % 4u);
    dust::Column solid{}, loose_of{};
    for (int k = 0; k < 4; ++k) {
      solid.w[k] = rng(); loose_of.w[k] = rng();
      for (uint32_t d = 0; d < density; ++d) solid.w[k] &= rng();
      for (uint32_t d = 0; d < share; ++d) loose_of.w[k] |= rng();
    }
    both(solid, loose_of);
  }
  std::printf("fall %u %u\n", columns, moved);
  return 0;
}

// ---- slides: a world of 3^3 bricks (12^3 voxels); what lies off it is off the tree
constexpr int kWorld = 12;
struct World {
  uint8_t solid[kWorld][kWorld][kWorld], loose[kWorld][kWorld][kWorld];
  int lo[3], hi[3];
  bool inside(const int p[3]) const { return p[0] >= lo[0] && p[0] <= hi[0] && p[1] >= lo[1] && p[1] <= hi[1] && p[2] >= lo[2] && p[2] <= hi[2]; }
  uint64_t word(const uint8_t (&f)[kWorld][kWorld][kWorld], int bx, int by, int bz) const {
    if (bx < 0 || by < 0 || bz < 0 || bx > 2 || by > 2 || bz > 2) return 0ull;
    uint64_t w = 0;
    for (int v = 0; v < 64; ++v)
      if (f[bx * 4 + (v >> 4)][by * 4 + ((v >> 2) & 3)][bz * 4 + (v & 3)]) w |= 1ull << v;
    return w;
  }
  uint64_t region(int bx, int by, int bz) const {
    if (bx < 0 || by < 0 || bz < 0 || bx > 2 || by > 2 || bz > 2) return 0ull;
    const uint32_t l[3] = {uint32_t(lo[0]), uint32_t(lo[1]), uint32_t(lo[2])}, h[3] = {uint32_t(hi[0]), uint32_t(hi[1]), uint32_t(hi[2])};
    return dust::surface_region_mask(uint32_t(bx), uint32_t(by), uint32_t(bz), l, h);
  }
};

int run_slide(uint32_t seed) {
  std::mt19937_64 rng(seed);
  uint32_t bricks = 0, slid = 0;
  World w;
  for (int round = 0; round < 24; ++round) {
    const uint32_t density = 2u + uint32_t(rng() % 6u);
    for (auto& plane : w.solid) for (auto& row : plane) for (uint8_t& v : row) v = rng() % 10u < density ? 1 : 0;
    for (int x = 0; x < kWorld; ++x) for (int y = 0; y < kWorld; ++y) for (int z = 0; z < kWorld; ++z) w.loose[x][y][z] = w.solid[x][y][z] && rng() % 4u != 0u;
    for (int r = 0; r < 3; ++r) {
      w.lo[r] = round % 3 == 0 ? 0 : int(rng() % 6u);
      w.hi[r] = round % 3 == 0 ? kWorld - 1 : w.lo[r] + int(rng() % uint32_t(kWorld - w.lo[r]));
    }
    for (uint32_t g_axis = 0; g_axis < 3u; ++g_axis)
      for (uint32_t g_up = 0; g_up < 2u; ++g_up)
        for (uint32_t k = 0; k < 4u; ++k) {
          uint32_t d_axis = 0, d_up = 0;
          dust::settle_slide_direction(g_axis, k, d_axis, d_up);
          CHECK(d_axis != g_axis && d_axis < 3u && d_up < 2u);
          int d[3] = {0, 0, 0}, g[3] = {0, 0, 0};
          d[d_axis] = d_up ? 1 : -1;
          g[g_axis] = g_up ? 1 : -1;
          // the loop: who leaves, who arrives
          static uint8_t leave[kWorld][kWorld][kWorld], arrive[kWorld][kWorld][kWorld];
          std::memset(leave, 0, sizeof(leave)); std::memset(arrive, 0, sizeof(arrive));
          for (int x = 0; x < kWorld; ++x) for (int y = 0; y < kWorld; ++y) for (int z = 0; z < kWorld; ++z) {
            const int p[3] = {x, y, z};
            if (!w.loose[x][y][z] || !w.inside(p)) continue;
            const int above[3] = {x - g[0], y - g[1], z - g[2]}, beside[3] = {x + d[0], y + d[1], z + d[2]};
            const int below[3] = {beside[0] + g[0], beside[1] + g[1], beside[2] + g[2]};
            auto in_world = [](const int q[3]) { return q[0] >= 0 && q[1] >= 0 && q[2] >= 0 && q[0] < kWorld && q[1] < kWorld && q[2] < kWorld; };
            if (in_world(above) && w.inside(above) && w.solid[above[0]][above[1]][above[2]]) continue;
            if (!in_world(beside) || !in_world(below) || !w.inside(beside) || !w.inside(below)) continue;
            if (w.solid[beside[0]][beside[1]][beside[2]] || w.solid[below[0]][below[1]][below[2]]) continue;
            leave[x][y][z] = 1;
            CHECK(!arrive[below[0]][below[1]][below[2]]);
            arrive[below[0]][below[1]][below[2]] = 1;
          }
          dust::SettleDirs dirs;
          dirs.d = dust::settle_axis(d_axis); dirs.g = dust::settle_axis(g_axis);
          dirs.d_up = d_up != 0u; dirs.g_up = g_up != 0u;
          for (int bx = 0; bx < 3; ++bx) for (int by = 0; by < 3; ++by) for (int bz = 0; bz < 3; ++bz) {
            dust::SettleBricks n;
            for (int i = -1; i <= 1; ++i)
              for (int j = -1; j <= 1; ++j) {
                const int nx = bx + i * d[0] + j * g[0], ny = by + i * d[1] + j * g[1], nz = bz + i * d[2] + j * g[2];
                n.occ[i + 1][j + 1] = w.word(w.solid, nx, ny, nz);
                n.loose[i + 1][j + 1] = w.word(w.loose, nx, ny, nz);
                n.region[i + 1][j + 1] = w.region(nx, ny, nz);
              }
            const dust::SettleSlide s = dust::settle_slide(n, dirs);
            uint64_t want_leave = 0, want_arrive = 0;
            for (int v = 0; v < 64; ++v) {
              if (leave[bx * 4 + (v >> 4)][by * 4 + ((v >> 2) & 3)][bz * 4 + (v & 3)]) want_leave |= 1ull << v;
              if (arrive[bx * 4 + (v >> 4)][by * 4 + ((v >> 2) & 3)][bz * 4 + (v & 3)]) want_arrive |= 1ull << v;
            }
            CHECK(s.leave == want_leave && s.arrive == want_arrive);
            CHECK((s.leave & s.arrive) == 0ull && (s.arrive & n.occ[1][1]) == 0ull && (s.leave & ~n.loose[1][1]) == 0ull);
            slid += uint32_t(__builtin_popcountll(s.arrive));
            ++bricks;
          }
        }
  }
  std::printf("slide %u %u\n", bricks, slid);
  return 0;
}

int run_records() {
  std::string line;
  char buf[1 << 16];
  while (std::fgets(buf, sizeof(buf), stdin)) {
    line = buf;
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "q") {
      DustHipSettleQuery q{};
      q.struct_size = sizeof(q);
      in >> q.toward >> q.flags >> q.reserved;
      for (uint32_t& v : q.lo) in >> v;
      for (uint32_t& v : q.hi) in >> v;
      for (uint32_t& v : q.loose) in >> v;
      if (!in) return 2;
      dust::SettleArgs a{};
      dust::CellBox box{};
      bool all_loose = false, empty = false;
      uint32_t nu = 77, nv = 77;
      if (dust::device_settle(q, a, box, all_loose, empty, nu, nv) != nullptr) {
        std::printf("q 0\n");
        continue;
      }
      std::printf("q 1 %u %u %u %u %u %u", empty ? 1u : 0u, all_loose ? 1u : 0u, a.axis, a.from_high, nu, nv);
      if (!empty)
        std::printf(" %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", a.lo_n, a.hi_n, a.lo_u, a.hi_u, a.lo_v, a.hi_v, a.cell_u, a.cell_v, a.cells_u, a.cells_v,
                    box.lo[0], box.lo[1], box.lo[2], box.hi[0], box.hi[1], box.hi[2]);
      std::printf("\n");
    } else if (what == "g") {
      uint32_t generations = 0;
      in >> generations;
      if (!in) return 2;
      std::printf("g %u\n", dust::settle_apply_arguments(generations) == nullptr ? 1u : 0u);
    } else if (what == "d") {
      uint32_t axis = 0, k = 0, d_axis = 9, d_up = 9;
      in >> axis >> k;
      if (!in) return 2;
      dust::settle_slide_direction(axis, k, d_axis, d_up);
      std::printf("d %u %u\n", d_axis, d_up);
    } else if (what == "r") {
      uint32_t nu = 0, nv = 0, acc[dust::kSettleAccWords] = {};
      uint32_t n = 0;
      const bool given = bool(in >> nu >> nv);
      while (given && n < dust::kSettleAccWords && (in >> acc[n])) ++n;
      if (given && n != dust::kSettleAccWords) return 2;
      DustHipSettleResult r;
      std::memset(&r, 0xEE, sizeof(r));  // (every byte of the output must be written)
      r = dust::settle_result(given ? acc : nullptr, nu, nv);
      std::printf("r %u %u %u %u %u %u %" PRIu64 " %u %u %u %u %u %u %u", r.columns, r.loose, r.fixed, r.moved, r.changed, r.fall_max, r.fall_sum, r.lo[0], r.lo[1],
                  r.lo[2], r.hi[0], r.hi[1], r.hi[2], r.changed_columns);
      uint32_t rest = r.pad0 | r.pad1;
      for (uint32_t v : r.reserved) rest |= v;
      std::printf(" %u\n", rest);
    } else if (what == "a") {
      uint32_t generations = 0, n = 0;
      in >> generations;
      if (!in || generations > dust::kSettleMaxGenerations) return 2;
      const bool given = bool(in >> n);
      std::vector<uint32_t> slots(dust::kSettleApplyWords, 0u), rows(size_t(generations) * 2 + 1, 0xEEEEEEEEu);
      if (given && n > slots.size()) return 2;
      for (uint32_t i = 0; given && i < n; ++i)
        if (!(in >> slots[i])) return 2;
      DustHipSettleApplied r;
      std::memset(&r, 0xEE, sizeof(r));
      r = dust::settle_applied(given ? slots.data() : nullptr, generations, rows.data());
      CHECK(rows[size_t(generations) * 2] == 0xEEEEEEEEu);  // (not a word past the rows)
      std::printf("a %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u %u %u", r.generations, r.first_moved, r.loose, r.slid, r.fell, r.fall_sum, r.lo[0], r.lo[1],
                  r.lo[2], r.hi[0], r.hi[1], r.hi[2]);
      uint32_t rest = r.pad0 | r.pad1 | r.reserved0;
      for (uint32_t v : r.reserved) rest |= v;
      std::printf(" %u %u", rest, given && dust::settle_at_rest(slots.data(), generations) ? 1u : 0u);
      for (uint32_t i = 0; i < generations * 2u; ++i) std::printf(" %u", rows[i]);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  const uint32_t seed = argc > 2 ? uint32_t(std::strtoul(argv[2], nullptr, 10)) : 1u;
  if (mode == "fall") return run_fall(seed);
  if (mode == "slide") return run_slide(seed);
  if (mode == "records") return run_records();
  return 2;
}
