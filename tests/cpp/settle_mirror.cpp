// A crater's aftermath through the C++ mirror (include/dust_hip.hpp): sand (palette indices 3 and 4) lies on rock; after a carve, ask
// how much of it would fall, let it fall, and let the heap run out over up to 64 generations. Compiled (not run) by
// tests/test_settle_abi.py.
#include "dust_hip.hpp"

struct Aftermath { uint32_t hanging; uint64_t slid, fell; uint32_t generations; uint32_t last_row; };

Aftermath settle_sand(dust::VoxGeometry& block) {
  DustHipSettleQuery sand{};
  sand.toward = DUST_HIP_FACE_NEG_Y;                                  // ordinary gravity
  for (int r = 0; r < 3; ++r) sand.hi[r] = 255;
  sand.loose[0] = (1u << 3) | (1u << 4);
  const DustHipSettleResult ask = block.settle(sand);                 // ask first
  Aftermath a{};
  a.hanging = ask.moved;
  if (ask.moved == 0) return a;
  std::vector<uint32_t> rows;
  const DustHipSettleApplied done = block.settle_apply(sand, 64, &rows);   // apply after
  a.slid = done.slid;
  a.fell = done.fell + done.first_moved;
  a.generations = done.generations;
  a.last_row = done.generations ? rows[2 * (done.generations - 1)] + rows[2 * (done.generations - 1) + 1] : 0;
  DustHipSettleQuery all = sand;                                      // everything is loose: a plain vertical settle of the lot
  for (uint32_t& w : all.loose) w = 0xFFFFFFFFu;
  all.loose[7] = 0x7FFFFFFFu;
  a.fell += block.settle_apply(all).first_moved;
  static_assert(sizeof(DustHipSettleQuery) == 72 && sizeof(DustHipSettleResult) == 64 && sizeof(DustHipSettleApplied) == 64 &&
                    DUST_HIP_SETTLE_MAX_GENERATIONS == 256u,
                "settle records");
  return a;
}
