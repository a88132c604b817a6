// walk_cell_test.cpp -- dust_amd/csrc/walk_cell.hpp driven on a CPU (tests/test_walk_cell.py builds this with g++ under AddressSanitizer and
// UBSan, -ffp-contract=off like the device build, and compares what it writes bit for bit): cases in, every output of the three functions out.
//   walk_cell_test IN OUT
// IN and OUT are u32 words (a float is its bit pattern). IN: three counts, then the cases:
//   walk_enter        : {o[3], d[3], bmin[3], bmax[3], te, tx, tmin, RT (0..3)}                                     -> {t, ijk[3], near_tol, screen, tx_stop}
//   whole_cell_screen : {o[3], d[3], t, ijk[3], stepped, near_tol, prev_whole, key, mask4 low, mask4 high}          -> {screen}
//   cell_exit         : {o[3], d[3], inv[3], ijk[3], cl_main, extent, near_tol}                                     -> {tn, next_ijk[3], next_stepped, stuck, outside, next_screen}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "walk_cell.hpp"

namespace {
std::vector<uint32_t> in, out;
size_t at = 0;
uint32_t take() {
  if (at >= in.size()) { std::fprintf(stderr, "input too short\n"); std::exit(2); }
  return in[at++];
}
float takef() { const uint32_t w = take(); float f; std::memcpy(&f, &w, 4); return f; }
void take3(float (&v)[3]) { for (float& x : v) x = takef(); }
void take3(int (&v)[3]) { for (int& x : v) x = (int)take(); }
void put(uint32_t v) { out.push_back(v); }
void putf(float f) { uint32_t w; std::memcpy(&w, &f, 4); put(w); }

void enter_case() {
  float o[3], d[3], bmin[3], bmax[3];
  take3(o); take3(d); take3(bmin); take3(bmax);
  const float te = takef(), tx = takef(), tmin = takef();
  const uint32_t rt = take();
  float t, near_tol, tx_stop;
  int ijk[3];
  bool screen;
  switch (rt) {
    case 0: dust::walk_enter<0>(o, d, bmin, bmax, te, tx, tmin, t, ijk, near_tol, screen, tx_stop); break;
    case 1: dust::walk_enter<1>(o, d, bmin, bmax, te, tx, tmin, t, ijk, near_tol, screen, tx_stop); break;
    case 2: dust::walk_enter<2>(o, d, bmin, bmax, te, tx, tmin, t, ijk, near_tol, screen, tx_stop); break;
    case 3: dust::walk_enter<3>(o, d, bmin, bmax, te, tx, tmin, t, ijk, near_tol, screen, tx_stop); break;
    default: std::fprintf(stderr, "ray type %u\n", rt); std::exit(2);
  }
  putf(t); put((uint32_t)ijk[0]); put((uint32_t)ijk[1]); put((uint32_t)ijk[2]); putf(near_tol); put(screen); putf(tx_stop);
}

void screen_case() {
  float o[3], d[3];
  int ijk[3];
  take3(o); take3(d);
  const float t = takef();
  take3(ijk);
  const uint32_t stepped = take();
  const float near_tol = takef();
  const bool prev_whole = take() != 0;
  const int key = (int)take();
  const uint64_t lo = take(), hi = take();
  put(dust::whole_cell_screen(o, d, t, ijk, stepped, near_tol, prev_whole, key, lo | hi << 32));
}

void exit_case() {
  float o[3], d[3], inv[3];
  int ijk[3];
  take3(o); take3(d); take3(inv); take3(ijk);
  const uint32_t cl_main = take();
  const int extent = (int)take();
  const float near_tol = takef();
  float tn;
  bool stuck;
  uint32_t next_stepped;
  int next_ijk[3];
  bool outside, next_screen;
  dust::cell_exit(o, d, inv, ijk, cl_main, extent, near_tol, tn, next_ijk, next_stepped, stuck, outside, next_screen);
  putf(tn); put((uint32_t)next_ijk[0]); put((uint32_t)next_ijk[1]); put((uint32_t)next_ijk[2]); put(next_stepped); put(stuck); put(outside); put(next_screen);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: walk_cell_test IN OUT\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  in.resize((size_t)bytes / 4);
  if (std::fread(in.data(), 4, in.size(), f) != in.size()) { std::fprintf(stderr, "short read\n"); return 2; }
  std::fclose(f);
  const uint32_t n_enter = take(), n_screen = take(), n_exit = take();
  out.reserve((size_t)n_enter * 7 + n_screen + (size_t)n_exit * 8);
  for (uint32_t i = 0; i < n_enter; ++i) enter_case();
  for (uint32_t i = 0; i < n_screen; ++i) screen_case();
  for (uint32_t i = 0; i < n_exit; ++i) exit_case();
  if (at != in.size()) { std::fprintf(stderr, "input too long\n"); return 2; }
  f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  if (std::fwrite(out.data(), 4, out.size(), f) != out.size()) { std::fprintf(stderr, "short write\n"); return 2; }
  std::fclose(f);
  return 0;
}
