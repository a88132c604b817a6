// frame_plan_test.cpp -- dust_amd/csrc/frame_plan.hpp driven on a CPU (tests/test_frame_plan.py builds this with g++ under AddressSanitizer
// and UBSan and checks what it writes): launch-shaping inputs in, plans out.
//   frame_plan_test IN OUT
// IN and OUT are u32 words (a u64 is its low word, then its high word; a float is its bit pattern). IN: one u32 count per section, then the sections:
//   0 slot axes     : 12 lists {n, values...}: cus, max_lds, block, bpc, models, {instances, groups}, {reserve, in_collective}, {side_busy, share},
//                     {frames in flight, slot mode}, oversub, tiles, batch frames -- a pair is one value of its axis; then flags: bit 0 no_lds_boxes,
//                     1 wide_fused, 2 wide_share. The program walks their product, the last axis fastest.
//                     -> per case {flags (1 too_big, 2 share_slots, 4 fused too_big), lds, n_lds_boxes, bpc, resident, reserve_blocks, side_slots,
//                        main_resident, frame_slots, grid, fblock, fgrid}
//   1 calibrated    : {P, Q, deep} -> share              2 guessed : {pool, width, rows} -> share
//   3 stream layout : {budget u64, bin, dim[3], n_items, n_instances, no_stream_lds} -> {boxes, cells, items, enters, total}
//   4 walk budget   : {max_lds u64, n_lds_models} -> u64
//   5 grids         : {slots, tiles, block, want, share} -> {packet_grid(slots, tiles), ray_walk_grid(slots, block, want), side_resident(slots, share)}
//   6 paths         : {passes, has_grid, gi_path, deep, debug, no_gather_order} -> {gather_as_stream, surfel_as_stream}
//   7 view keys     : {camera 15, scene u64, revision u64, sky 56, row_begin, row_end} -> u64
//   8 fnv           : {n bytes, then ceil(n / 4) words holding them} -> u64
//   9 view runs     : {n, continues as a bit mask} -> 8 run lengths (0xFFFFFFFF behind the n-th)
//  10 timing        : {context stride, batched, frames, counter} -> {stride, timed}
//  11 shard ranges  : {pool, rank, world} -> {groups, per, cap u64, group_begin, group_count, slots_per_rank}
//  12 key bits      : {capacity} -> bits
//  13 tile schedule : {first (the state starts afresh), tiles_x, tiles_y, view u64, flags (1 no_tile_order, 2 equal_bands, 4 dilate, 8 force_moving),
//                     cuts_reuse, moving_refresh, still_refresh_max} -> {decisions (1 allocate, 2 reset, 4 blend, 8 dilate, 16 reuse_cuts, 32 hand_order,
//                     64 hand_cuts, 128 measure), total, per_band, tiles_x, tiles_y, capacity, age, refresh, view u64, state (1 recorded, 2 ordered,
//                     4 measured, 8 moving), cuts_age}
// OUT ends with {sizeof(DevEnter), kTileOrderMaxBand, kMaxBatch, kRegions}.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "frame_plan.hpp"

namespace {
std::vector<uint32_t> in, out;
size_t at = 0;
uint32_t take() {
  if (at >= in.size()) { std::fprintf(stderr, "input too short\n"); std::exit(2); }
  return in[at++];
}
uint64_t take64() { const uint64_t lo = take(); return lo | uint64_t(take()) << 32; }
float takef() { const uint32_t w = take(); float f; std::memcpy(&f, &w, 4); return f; }
void put(uint32_t v) { out.push_back(v); }
void put64(uint64_t v) { put(uint32_t(v)); put(uint32_t(v >> 32)); }
std::vector<uint32_t> take_list(uint32_t width) {
  std::vector<uint32_t> v(size_t(take()) * width);
  for (uint32_t& x : v) x = take();
  return v;
}

void slot_product() {
  std::vector<uint32_t> ax[12];
  const uint32_t width[12] = {1, 1, 1, 1, 1, 2, 2, 2, 2, 1, 1, 1};
  for (int k = 0; k < 12; ++k) ax[k] = take_list(width[k]);
  const uint32_t flags = take();
  size_t idx[12] = {};
  for (bool done = false; !done;) {
    auto v = [&](int k, int j = 0) { return ax[k][idx[k] * width[k] + j]; };
    dust::SlotInputs si;
    si.num_cus = v(0); si.max_lds = v(1); si.block = v(2); si.blocks_per_cu = v(3); si.n_lds_models = v(4);
    si.n_instances = v(5); si.n_groups = v(5, 1);
    si.no_lds_boxes = flags & 1u;
    si.reserve_request = v(6); si.in_collective = v(6, 1);
    si.side_busy = v(7); si.share = v(7, 1);
    si.frames_in_flight = v(8); si.in_flight_slots = v(8, 1); si.in_flight_oversub = v(9);
    si.total_tiles = v(10);
    const dust::SlotPlan pl = dust::slot_plan(si);
    dust::FusedShape f;
    if (!pl.too_big) f = dust::fused_shape(si, pl, flags & 2u, flags & 4u, v(11));
    put((pl.too_big ? 1u : 0u) | (pl.share_slots ? 2u : 0u) | (f.too_big ? 4u : 0u));
    put(uint32_t(pl.lds)); put(pl.n_lds_boxes); put(pl.bpc); put(pl.resident); put(pl.reserve_blocks); put(pl.side_slots); put(pl.main_resident);
    put(pl.frame_slots); put(pl.grid); put(f.fblock); put(f.fgrid);
    int k = 11;
    while (k >= 0 && ++idx[k] * width[k] == ax[k].size()) idx[k--] = 0;
    done = k < 0;
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    uint32_t buf[16384];
    for (size_t k; (k = std::fread(buf, 4, 16384, f)) > 0;) in.insert(in.end(), buf, buf + k);
    std::fclose(f);
  } else {
    return 2;
  }
  uint32_t n[14];
  for (uint32_t& c : n) c = take();

  for (uint32_t i = 0; i < n[0]; ++i) slot_product();
  for (uint32_t i = 0; i < n[1]; ++i) { const float P = takef(), Q = takef(); put(dust::calibrated_share(P, Q, take() != 0)); }
  for (uint32_t i = 0; i < n[2]; ++i) { const uint32_t pool = take(), w = take(), rows = take(); put(dust::guessed_share(pool, w, rows)); }
  for (uint32_t i = 0; i < n[3]; ++i) {
    const uint64_t budget = take64();
    const bool bin = take() != 0;
    const uint32_t dim[3] = {take(), take(), take()};   // (braced: read in order)
    const uint32_t items = take(), inst = take();
    const dust::DevStreamLds l = dust::stream_lds(size_t(budget), bin, dim, items, inst, take() != 0);
    put(l.boxes); put(l.cells); put(l.items); put(l.enters); put(l.total);
  }
  for (uint32_t i = 0; i < n[4]; ++i) { const uint64_t max_lds = take64(); put64(dust::stream_walk_budget(size_t(max_lds), take())); }
  for (uint32_t i = 0; i < n[5]; ++i) {
    const uint32_t slots = take(), tiles = take(), block = take(), want = take(), share = take();
    put(dust::packet_grid(slots, tiles)); put(dust::ray_walk_grid(slots, block, want)); put(dust::side_resident(slots, share));
  }
  for (uint32_t i = 0; i < n[6]; ++i) {
    const uint32_t passes = take(), grid = take(), path = take(), deep = take(), debug = take(), ngo = take();
    put(dust::gather_as_stream(passes, grid != 0, path, deep != 0, debug, ngo != 0)); put(dust::surfel_as_stream(passes, grid != 0, path));
  }
  for (uint32_t i = 0; i < n[7]; ++i) {
    DustHipCamera cam; DustHipSky sky;
    static_assert(sizeof cam == 60 && sizeof sky == 224, "the view key's bytes");
    uint32_t w[15 + 56];
    for (int k = 0; k < 15; ++k) w[k] = take();
    const uint64_t scene = take64(), revision = take64();
    for (int k = 0; k < 56; ++k) w[15 + k] = take();
    std::memcpy(&cam, w, sizeof cam); std::memcpy(&sky, w + 15, sizeof sky);
    const uint32_t rb = take(), re = take();
    put64(dust::view_key(cam, reinterpret_cast<const void*>(uintptr_t(scene)), revision, sky, rb, re));
  }
  for (uint32_t i = 0; i < n[8]; ++i) {
    const uint32_t bytes = take();
    std::vector<uint32_t> w((bytes + 3) / 4);
    for (uint32_t& x : w) x = take();
    dust::Fnv1a h;
    h.mix(w.data(), bytes);
    put64(h.k);
  }
  for (uint32_t i = 0; i < n[9]; ++i) {
    const uint32_t frames = take(), mask = take();
    if (frames > dust::kMaxBatch) return 3;
    std::vector<uint32_t> run(frames, 0xFFFFFFFFu);   // (heap arrays of exactly n: a step past the end is the sanitizer's to see)
    bool* cont = new bool[frames ? frames : 1];
    for (uint32_t k = 0; k < frames; ++k) cont[k] = (mask >> k) & 1u;
    dust::view_runs(cont, frames, run.data());
    delete[] cont;
    for (uint32_t k = 0; k < dust::kMaxBatch; ++k) put(k < frames ? run[k] : 0xFFFFFFFFu);
  }
  for (uint32_t i = 0; i < n[10]; ++i) {
    const uint32_t cs = take(), batched = take(), frames = take(), counter = take();
    const uint32_t stride = dust::timing_stride(cs, batched != 0, frames);
    put(stride); put(dust::launch_timed(counter, stride));
  }
  for (uint32_t i = 0; i < n[11]; ++i) {
    const uint32_t pool = take(), rank = take(), world = take();
    const dust::ShardRange r = dust::shard_range(pool, rank, world);
    put(r.groups); put(r.per); put64(r.cap); put(r.group_begin); put(r.group_count); put(r.slots_per_rank);
  }
  for (uint32_t i = 0; i < n[12]; ++i) put(dust::apply_key_bits(take()));
  dust::TileState h;
  for (uint32_t i = 0; i < n[13]; ++i) {
    if (take()) h = dust::TileState{};
    const uint32_t tx = take(), ty = take();
    const uint64_t view = take64();
    const uint32_t fl = take(), cuts_reuse = take(), moving_refresh = take(), still_max = take();
    const dust::TileStep d = dust::tile_step(h, tx, ty, view, {(fl & 1u) != 0, (fl & 2u) != 0, (fl & 4u) != 0, (fl & 8u) != 0, cuts_reuse, moving_refresh, still_max});
    put(uint32_t(d.allocate) | d.reset << 1 | d.blend << 2 | d.dilate << 3 | d.reuse_cuts << 4 | d.hand_order << 5 | d.hand_cuts << 6 | d.measure << 7);
    put(d.total); put(d.per_band);
    put(h.tiles_x); put(h.tiles_y); put(h.capacity); put(h.age); put(h.refresh); put64(h.view);
    put(uint32_t(h.recorded) | h.ordered << 1 | h.measured << 2 | h.moving << 3); put(h.cuts_age);
  }
  put(uint32_t(sizeof(dust::DevEnter))); put(dust::kTileOrderMaxBand); put(dust::kMaxBatch); put(dust::kRegions);
  if (at != in.size()) { std::fprintf(stderr, "input too long\n"); return 2; }

  FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size() || std::fclose(f) != 0) return 2;
  return 0;
}
