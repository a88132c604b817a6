// hierarchy_test.cpp -- dust_amd/csrc/hierarchy.hpp driven on a CPU (tests/test_hierarchy.py builds this with g++ under AddressSanitizer
// and UBSan, without a HIP compiler or the library, and holds what it writes to tests/hierarchy_witness.py): blocks in, every array of
// the upper levels, or the refusal, out.
//   hierarchy_test IN OUT
// IN : u32 extent_log2, n_blocks; DustHipBlock[n_blocks]
// OUT: i32 status; refused: u32 length, the message. Accepted: u32 n_mid, n_l2, n_dense, n_cells; f32 bmin[3], bmax[3]; root (656 B);
//      l2 (n_l2 x 656 B); DevN4[n_mid]; u64 dense_mask[n_dense]; DevL2Cell[n_cells]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hierarchy.hpp"

namespace {
std::vector<unsigned char> out;
void put_bytes(const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  out.insert(out.end(), b, b + n);
}
template <class T>
void put(const T& v) { put_bytes(&v, sizeof(T)); }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::vector<unsigned char> in;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    unsigned char buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
  } else {
    return 2;
  }
  uint32_t head[2];
  if (in.size() < sizeof(head)) { std::fprintf(stderr, "input too short\n"); return 2; }
  std::memcpy(head, in.data(), sizeof(head));
  const uint32_t extent_log2 = head[0], n = head[1];
  if (in.size() != sizeof(head) + size_t(n) * sizeof(DustHipBlock)) { std::fprintf(stderr, "input length\n"); return 2; }
  std::vector<DustHipBlock> blocks(n);  // exactly n records on the heap: a read past them is the sanitizer's to report
  if (n) std::memcpy(blocks.data(), in.data() + sizeof(head), size_t(n) * sizeof(DustHipBlock));

  dust::Hierarchy h;
  const char* message = nullptr;
  const DustStatus s = dust::build_hierarchy(blocks.data(), n, extent_log2, h, &message);
  put(int32_t(s));
  if (s != DUST_OK) {
    const uint32_t len = message ? uint32_t(std::strlen(message)) : 0u;
    put(len);
    put_bytes(message, len);
  } else {
    if (extent_log2 == 12) dust::build_l2_cells(h);
    put(uint32_t(h.mid.size())); put(uint32_t(h.l2.count())); put(uint32_t(h.dense_mask.size())); put(uint32_t(h.l2_cells.size()));
    put_bytes(h.bmin, sizeof(h.bmin)); put_bytes(h.bmax, sizeof(h.bmax));
    put_bytes(h.root.bytes.data(), h.root.bytes.size());
    put_bytes(h.l2.bytes.data(), h.l2.bytes.size());
    put_bytes(h.mid.data(), h.mid.size() * sizeof(dust::DevN4));
    put_bytes(h.dense_mask.data(), h.dense_mask.size() * 8);
    put_bytes(h.l2_cells.data(), h.l2_cells.size() * sizeof(dust::DevL2Cell));
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  const bool ok = out.empty() || std::fwrite(out.data(), 1, out.size(), f) == out.size();
  return (std::fclose(f) == 0 && ok) ? 0 : 2;
}
