// Drives dust_amd/csrc/joint_rule.hpp -- the one text of the model joints' arithmetic, which joint.hip runs per (brick, axis, pair,
// direction) -- and device_joints of dust_amd/csrc/model_records.hpp on a CPU (tests/test_joint_rule.py). No HIP compiler, not linked
// against the library.
//   in:  u32 n_parts, n_folds, n_pairs, n_queries; n_parts x { u64 word; u32 axis, flip, bx, by, bz, key }; n_pairs x { u32 lower, upper };
//        n_queries x DustHipJointQuery
//   out: per part the 80-byte record of the part alone; then the record of all parts folded (the key of part 0); then the record of part
//        0 folded n_folds times; per pair u32 key, flip, a, b; per query u32 refused, empty, group, pad, lo[3], hi[3], box_lo[3],
//        box_hi[3]; then the table: u32 first slots_log2 of the whole tree, keys, inserted, found again, full reports, longest probe,
//        then the same five for 1200 keys into the smallest table
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "joint_rule.hpp"
#include "model_records.hpp"

namespace {

struct PartCase {
  uint64_t word;
  uint32_t axis, flip, bx, by, bz, key;
};
static_assert(sizeof(PartCase) == 32, "part case");

template <class T>
void put(std::vector<uint8_t>& out, const T& v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
  out.insert(out.end(), p, p + sizeof(T));
}

// the table as k_joints' flush walks it, one key after the other: the slot of `key`, claimed when it was free; -1: full
struct Table {
  uint32_t log2;
  std::vector<uint32_t> words;
  uint32_t longest = 0;
  explicit Table(uint32_t slots_log2) : log2(slots_log2), words(size_t(1) << slots_log2, dust::kJointSlotEmpty) {}
  int64_t find(uint32_t key, bool claim) {
    const uint32_t word = dust::joint_slot_word(key), hash = dust::joint_hash(key, log2), limit = dust::joint_probe_limit(log2);
    for (uint32_t step = 0; step < limit; ++step) {
      const uint32_t at = dust::joint_probe(hash, step, log2);
      if (words.at(at) == dust::kJointSlotEmpty && claim) words.at(at) = word;
      if (words.at(at) == word) { longest = step > longest ? step : longest; return at; }
      if (words.at(at) == dust::kJointSlotEmpty) return -1;  // (a lookup: the key was never inserted)
    }
    return -1;
  }
};
void run_table(std::vector<uint8_t>& out, uint32_t log2, const std::vector<uint32_t>& keys) {
  Table t(log2);
  uint32_t inserted = 0, found = 0, full = 0;
  std::vector<int64_t> where(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) {
    where[i] = t.find(keys[i], true);
    if (where[i] < 0) ++full; else ++inserted;
  }
  for (size_t i = 0; i < keys.size(); ++i)
    if (where[i] >= 0 && t.find(keys[i], false) == where[i]) ++found;
  const uint32_t words[5] = {uint32_t(keys.size()), inserted, found, full, t.longest};
  put(out, words);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[4];
  if (std::fread(head, 4, 4, f) != 4) return 2;
  std::vector<PartCase> parts(head[0]);
  if (head[0] && std::fread(parts.data(), sizeof(PartCase), head[0], f) != head[0]) return 2;
  std::vector<uint32_t> pairs(size_t(head[2]) * 2);
  if (head[2] && std::fread(pairs.data(), 8, head[2], f) != head[2]) return 2;
  std::vector<DustHipJointQuery> queries(head[3]);
  if (head[3] && std::fread(queries.data(), sizeof(DustHipJointQuery), head[3], f) != head[3]) return 2;
  std::fclose(f);

  std::vector<uint8_t> out;
  dust::JointPart all = dust::joint_neutral();
  if (!dust::joint_is_neutral(all)) return 3;
  for (const PartCase& c : parts) {
    const dust::JointPart p = dust::joint_part(c.word, c.axis, c.flip != 0u, c.bx, c.by, c.bz);  // (word != 0: the caller's rule)
    put(out, dust::joint_emit(c.key, p));
    dust::joint_fold(all, p);
  }
  put(out, dust::joint_emit(parts.empty() ? 0u : parts[0].key, all));
  dust::JointPart many = dust::joint_neutral();
  if (!parts.empty()) {
    const dust::JointPart p = dust::joint_part(parts[0].word, parts[0].axis, parts[0].flip != 0u, parts[0].bx, parts[0].by, parts[0].bz);
    for (uint32_t i = 0; i < head[1]; ++i) dust::joint_fold(many, p);
  }
  put(out, dust::joint_emit(parts.empty() ? 0u : parts[0].key, many));
  for (uint32_t i = 0; i < head[2]; ++i) {
    bool flip = false;
    const uint32_t key = dust::joint_face_key(pairs[2 * i], pairs[2 * i + 1], flip);
    const uint32_t words[4] = {key, flip ? 1u : 0u, dust::joint_key_a(key), dust::joint_key_b(key)};
    put(out, words);
  }
  for (const DustHipJointQuery& q : queries) {
    dust::JointArgs a{};
    bool empty = false;
    const char* why = dust::device_joints(q, a, empty);
    const uint32_t words[4] = {why ? 1u : 0u, empty ? 1u : 0u, a.group, 0u};
    put(out, words); put(out, a.lo); put(out, a.hi); put(out, a.box.lo); put(out, a.box.hi);
  }
  // every MATERIALS pair into the first table of a whole-tree call; then more keys than slots into the smallest table
  std::vector<uint32_t> keys;
  for (uint32_t a = 0; a < 255u; ++a)
    for (uint32_t b = a + 1u; b < 255u; ++b) keys.push_back(dust::joint_pack(a, b));
  const uint32_t first = dust::joint_first_slots_log2(4096u);
  put(out, first);
  run_table(out, first, keys);
  keys.clear();
  for (uint32_t c = 0; c < 1200u; ++c) keys.push_back(dust::joint_pack(c, c % 7u == 0u ? dust::kJointRest : c + 1u + c % 5u));
  run_table(out, dust::joint_first_slots_log2(1u), keys);
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  if (!out.empty() && std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
  std::fclose(f);
  return 0;
}
