// hierarchy.hpp -- the device-free half of dust_hip_model_create (capi_model.cpp): the upper levels of a model -- root and l2 N16 nodes,
// mid nodes, dense_mask, the DEEP kernels' per-cell table and the tight bounds (dust_dev.h "HBM layout of one model") -- built from the
// caller's blocks. No HIP call, no handle, no error state: a refusal comes back as a status and a message, which the caller turns into
// fail(...). tests/cpp/hierarchy_test.cpp drives it on a CPU (tests/test_hierarchy.py holds it to tests/hierarchy_witness.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dust_hip.h"
#include "dust_dev.h"
#include "vdb.hpp"

namespace dust {

struct N16Builder {
  std::vector<uint8_t> bytes;  // kN16Bytes per node
  uint8_t* node(size_t i) { return bytes.data() + i * kN16Bytes; }
  const uint8_t* node(size_t i) const { return bytes.data() + i * kN16Bytes; }
  size_t count() const { return bytes.size() / kN16Bytes; }
  size_t add() {
    bytes.resize(bytes.size() + kN16Bytes, 0);
    return bytes.size() / kN16Bytes - 1;
  }
  void finish(size_t i, uint32_t child_base) {  // rank prefix per 64-bit word + base of the first child
    uint64_t* mask = reinterpret_cast<uint64_t*>(node(i));
    uint16_t* pre = reinterpret_cast<uint16_t*>(node(i) + 512);
    uint32_t run = 0;
    for (int w = 0; w < 64; ++w) {
      pre[w] = static_cast<uint16_t>(run);
      run += static_cast<uint32_t>(__builtin_popcountll(mask[w]));
    }
    std::memcpy(node(i) + 640, &child_base, 4);
  }
};

struct Hierarchy {
  N16Builder root, l2;
  std::vector<DevN4> mid;
  std::vector<uint64_t> dense_mask;   // 64 per mid node
  std::vector<DevL2Cell> l2_cells;    // 4096 per l2 node (4096^3 trees only; build_l2_cells)
  float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
};

// Builds root / l2 / mid arrays from blocks given in Tree::iter_leaf order (depth-first, ascending bits). A refusal returns its status
// and leaves its text in *message; `h` is then not to be used.
inline DustStatus build_hierarchy(const DustHipBlock* blocks, uint32_t n, uint32_t extent_log2, Hierarchy& h, const char** message) {
  N16Builder& root = h.root;
  N16Builder& l2 = h.l2;
  std::vector<DevN4>& mid = h.mid;
  std::vector<uint64_t>& dense_mask = h.dense_mask;
  float* bmin = h.bmin;
  float* bmax = h.bmax;
  auto refuse = [&](const char* text) { *message = text; return DUST_ERR_INVALID_ARGUMENT; };
  const bool deep = extent_log2 == 12;
  const uint32_t extent = 1u << extent_log2;
  root.add();
  uint64_t prev_key = 0;
  int64_t cur_l2 = -1, cur_mid = -1;
  uint32_t cur_l2_cell = 0xFFFFFFFFu, cur_mid_cell = 0xFFFFFFFFu;
  for (int a = 0; a < 3; ++a) { bmin[a] = 1e30f; bmax[a] = -1e30f; }
  auto idx16 = [](uint32_t x, uint32_t y, uint32_t z) { return (x << 8) | (y << 4) | z; };
  for (uint32_t i = 0; i < n; ++i) {
    const DustHipBlock& b = blocks[i];
    if ((b.x & 3) || (b.y & 3) || (b.z & 3) || b.x >= extent || b.y >= extent || b.z >= extent)
      return refuse("block position is not a 4-aligned coordinate inside the tree extent");
    if (b.mask == 0) return refuse("block with empty occupancy mask");
    // depth-first order key: per level, x slowest (node/internal.rs:78-81)
    uint64_t key = 0;
    const uint32_t shifts_deep[3] = {8, 4, 2}, bits_deep[3] = {4, 4, 2};
    const uint32_t shifts_std[2] = {4, 2}, bits_std[2] = {4, 2};
    const uint32_t* sh = deep ? shifts_deep : shifts_std;
    const uint32_t* bt = deep ? bits_deep : bits_std;
    const int nl = deep ? 3 : 2;
    for (int l = 0; l < nl; ++l) {
      const uint32_t m = (1u << bt[l]) - 1;
      key = (key << (3 * bt[l])) | (uint64_t(((b.x >> sh[l]) & m)) << (2 * bt[l])) | (uint64_t((b.y >> sh[l]) & m) << bt[l]) |
            uint64_t((b.z >> sh[l]) & m);
    }
    if (i > 0 && key <= prev_key)
      return refuse("blocks are not in Tree::iter_leaf order (depth-first, ascending child bits)");
    prev_key = key;
    const float p[3] = {float(b.x), float(b.y), float(b.z)};
    for (int a = 0; a < 3; ++a) {
      bmin[a] = std::min(bmin[a], p[a]);
      bmax[a] = std::max(bmax[a], p[a] + 4.0f);
    }
    // descend, creating nodes on first touch (children of a node are contiguous because of the order)
    size_t n16 = 0;           // node holding the 16-cell bit
    N16Builder* holder = &root;
    if (deep) {
      const uint32_t cell = idx16(b.x >> 8, b.y >> 8, b.z >> 8);
      if (cell != cur_l2_cell) {
        cur_l2 = int64_t(l2.add());
        cur_l2_cell = cell;
        vdb::bit_set(reinterpret_cast<uint64_t*>(root.node(0)), cell, true);
        cur_mid_cell = 0xFFFFFFFFu;
      }
      holder = &l2;
      n16 = size_t(cur_l2);
    }
    const uint32_t cell16 = idx16((b.x >> 4) & 15, (b.y >> 4) & 15, (b.z >> 4) & 15);
    const uint32_t mid_cell_key = deep ? uint32_t(cur_l2) * 4096u + cell16 : cell16;
    if (mid_cell_key != cur_mid_cell) {
      vdb::bit_set(reinterpret_cast<uint64_t*>(holder->node(n16)), cell16, true);
      DevN4 nd{0, 0, i, 0};
      mid.push_back(nd);
      cur_mid = int64_t(mid.size()) - 1;
      cur_mid_cell = mid_cell_key;
    }
    const uint32_t bit = (((b.x >> 2) & 3) << 4) | (((b.y >> 2) & 3) << 2) | ((b.z >> 2) & 3);
    if (bit < 32) mid[size_t(cur_mid)].mask_lo |= 1u << bit;
    else mid[size_t(cur_mid)].mask_hi |= 1u << (bit - 32);
    if (dense_mask.size() < mid.size() * 64) dense_mask.resize(mid.size() * 64, 0);
    dense_mask[size_t(cur_mid) * 64 + bit] = b.mask;
  }
  // prefixes and child bases: children were appended in order, so base = running count
  if (deep) {
    root.finish(0, 0);
    uint32_t run = 0;
    for (size_t i = 0; i < l2.count(); ++i) {
      l2.finish(i, run);
      const uint64_t* mask = reinterpret_cast<const uint64_t*>(l2.node(i));
      for (int w = 0; w < 64; ++w) run += uint32_t(__builtin_popcountll(mask[w]));
    }
  } else {
    root.finish(0, 0);
  }
  if (n == 0) { for (int a = 0; a < 3; ++a) { bmin[a] = 0.0f; bmax[a] = 0.0f; } }
  return DUST_OK;
}

// 4096^3 trees: the per-cell table the DEEP kernel variants look 16-cells up in, {mid index, occupied box, child mask} per cell of every
// l2 node, from the l2 nodes and the mid nodes build_hierarchy made
inline void build_l2_cells(Hierarchy& h) {
  const size_t n_l2 = h.l2.count();
  h.l2_cells.assign(n_l2 * 4096, DevL2Cell{0xFFFFFFFFu, 0u, 0ull});
  for (size_t i = 0; i < n_l2; ++i) {
    const uint64_t* mask = reinterpret_cast<const uint64_t*>(h.l2.node(i));
    uint32_t base;
    std::memcpy(&base, h.l2.node(i) + 640, 4);
    uint32_t run = base;  // children of a node are contiguous, in ascending bit order
    for (uint32_t w = 0; w < 64; ++w)
      for (uint64_t bits = mask[w]; bits; bits &= bits - 1) {
        DevL2Cell& c = h.l2_cells[i * 4096 + w * 64 + uint32_t(__builtin_ctzll(bits))];
        c.mid = run;
        c.child_mask = (uint64_t(h.mid[run].mask_hi) << 32) | h.mid[run].mask_lo;
        uint32_t lo[3] = {3, 3, 3}, hi[3] = {0, 0, 0};
        for (uint64_t cm = c.child_mask; cm; cm &= cm - 1) {
          const uint32_t b = uint32_t(__builtin_ctzll(cm)), xyz[3] = {b >> 4, (b >> 2) & 3u, b & 3u};
          for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], xyz[k]); hi[k] = std::max(hi[k], xyz[k]); }
        }
        c.bounds = lo[0] | (lo[1] << 2) | (lo[2] << 4) | (hi[0] << 6) | (hi[1] << 8) | (hi[2] << 10);
        ++run;
      }
  }
}

}  // namespace dust
