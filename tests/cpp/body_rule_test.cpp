// Drives dust_amd/csrc/body_rule.hpp -- the one text of the model bodies' arithmetic, which body.hip runs per (brick, group) -- and
// device_bodies of dust_amd/csrc/model_records.hpp on a CPU (tests/test_body_rule.py). No HIP compiler, not linked against the library.
//   in:  u32 n_bricks, n_folds, n_queries, pad; n_bricks x { u64 mask; u32 bx, by, bz, key; u16 w[64] }; n_queries x DustHipBodyQuery
//   out: per brick: u32 unweighted[10], weighted[10], unit[10] (the weighted path with every weight 1); the 96-byte record of the
//        brick's weighted part; then the record of all bricks folded (key 7); then the record of brick 0 folded n_folds times (key 9);
//        per query: u32 refused, empty, group, byte, lo[3], hi[3], box_lo[3], box_hi[3]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "body_rule.hpp"
#include "model_records.hpp"

namespace {

struct BrickCase {
  uint64_t mask;
  uint32_t bx, by, bz, key;
  uint16_t w[64];
};
static_assert(sizeof(BrickCase) == 152, "brick case");

template <class T>
void put(std::vector<uint8_t>& out, const T& v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
  out.insert(out.end(), p, p + sizeof(T));
}

// the weighted path as the wave runs it: every voxel of the mask adds its ten values
dust::BodyLocal weighted(uint64_t mask, const uint16_t* w, bool unit) {
  dust::BodyLocal l{};
  for (uint32_t bit = 0; bit < 64u; ++bit) {
    if (!((mask >> bit) & 1ull)) continue;
    const dust::BodyLocal v = dust::body_local_voxel(unit ? 1u : w[bit], bit);
    for (uint32_t k = 0; k < dust::kBodySums; ++k) l.v[k] += v.v[k];
  }
  return l;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[4];
  if (std::fread(head, 4, 4, f) != 4) return 2;
  std::vector<BrickCase> bricks(head[0]);
  if (head[0] && std::fread(bricks.data(), sizeof(BrickCase), head[0], f) != head[0]) return 2;
  std::vector<DustHipBodyQuery> queries(head[2]);
  if (head[2] && std::fread(queries.data(), sizeof(DustHipBodyQuery), head[2], f) != head[2]) return 2;
  std::fclose(f);

  std::vector<uint8_t> out;
  dust::BodyPart all = dust::body_neutral();
  for (const BrickCase& b : bricks) {
    const dust::BodyLocal fast = dust::body_local_unweighted(b.mask), slow = weighted(b.mask, b.w, false), unit = weighted(b.mask, b.w, true);
    put(out, fast); put(out, slow); put(out, unit);
    dust::BodyPart p = dust::body_neutral();
    if (b.mask != 0ull) p = dust::body_brick_part(b.mask, slow, b.bx, b.by, b.bz);
    put(out, dust::body_emit(b.key, p));
    dust::body_fold(all, p);
  }
  put(out, dust::body_emit(7u, all));
  dust::BodyPart many = dust::body_neutral();
  if (!bricks.empty() && bricks[0].mask != 0ull) {
    const dust::BodyPart p = dust::body_brick_part(bricks[0].mask, weighted(bricks[0].mask, bricks[0].w, false), bricks[0].bx, bricks[0].by, bricks[0].bz);
    for (uint32_t i = 0; i < head[1]; ++i) dust::body_fold(many, p);
  }
  put(out, dust::body_emit(9u, many));
  for (const DustHipBodyQuery& q : queries) {
    dust::BodyArgs a{};
    bool empty = false;
    const char* why = dust::device_bodies(q, a, empty);
    const uint32_t words[4] = {why ? 1u : 0u, empty ? 1u : 0u, a.group, a.byte};
    put(out, words); put(out, a.lo); put(out, a.hi); put(out, a.box.lo); put(out, a.box.hi);
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  if (!out.empty() && std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
  std::fclose(f);
  return 0;
}
