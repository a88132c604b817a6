// model_records_test.cpp -- dust_amd/csrc/model_records.hpp driven on a CPU (tests/test_model_records.py builds this with g++ under
// AddressSanitizer and UBSan and checks what it writes): caller records in, device records, chunks, cell lists and cast hits out.
//   model_records_test IN OUT
// IN : u32 n_shapes, n_stamps, n_casts, n_bounds, n_configs, n_decode; DustHipEditShape[]; DustHipStamp[]; DustHipCast[];
//      {u32 lo, hi}[n_bounds]; {u32 max_entries, max_records}[n_configs]; {DustHipCast, u64 best, CastAcc}[n_decode]
// OUT: {u32 live, DevEditShape}[]; {u32 live, DevStamp}[]; {u32 live, DevCast}[]; u32 live indices of live_records over the casts
//      (count first); per config: u32 n_chunks, then per chunk u32 c1, n_cells, n_ids, n_items, cells[], starts[n_cells + 1],
//      ids[] (u16), items[] ({u32 cast, cell}); DustHipCastHit[n_decode]; u32 chunk_end of 513 whole-tree shapes and of 257
//      whole-tree casts at the real limits; i32 kCastOffsetLimit
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "model_records.hpp"

namespace {
std::vector<unsigned char> out;
template <class T>
void put(const T& v) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
  out.insert(out.end(), p, p + sizeof(T));
}
template <class T>
void put_all(const std::vector<T>& v) {
  for (const T& x : v) put(x);
}

struct Reader {
  std::vector<unsigned char> bytes;
  size_t at = 0;
  template <class T>
  std::vector<T> take(size_t n) {
    if (at + n * sizeof(T) > bytes.size()) { std::fprintf(stderr, "input too short\n"); std::exit(2); }
    std::vector<T> v(n);
    if (n) std::memcpy(v.data(), bytes.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
  }
};

template <class In, class Rec>
void convert_all(const std::vector<In>& in, bool (*convert)(const In&, Rec&)) {
  for (const In& s : in) {
    Rec d{};
    const uint32_t live = convert(s, d) ? 1u : 0u;
    put(live);
    put(live ? d : Rec{});
  }
}

struct Bounds { uint32_t lo, hi; };
struct Config { uint32_t max_entries, max_records; };
struct Decode { DustHipCast cast; unsigned long long best; dust::CastAcc acc; };
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  Reader in;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    unsigned char buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof(buf), f)) > 0;) in.bytes.insert(in.bytes.end(), buf, buf + k);
    std::fclose(f);
  } else {
    return 2;
  }
  const std::vector<uint32_t> head = in.take<uint32_t>(6);
  const auto shapes = in.take<DustHipEditShape>(head[0]);
  const auto stamps = in.take<DustHipStamp>(head[1]);
  const auto casts = in.take<DustHipCast>(head[2]);
  const auto bounds = in.take<Bounds>(head[3]);
  const auto configs = in.take<Config>(head[4]);
  const auto decode = in.take<Decode>(head[5]);

  convert_all(shapes, dust::device_shape);
  convert_all(stamps, dust::device_stamp);
  convert_all(casts, dust::device_cast);
  {
    std::vector<dust::DevCast> dev;
    std::vector<uint32_t> index;
    dust::live_records<dust::device_cast>(casts.data(), uint32_t(casts.size()), dev, index);
    put(uint32_t(index.size()));
    put_all(index);
  }

  // the same bounds as stamps (cell lists) and as casts (work items)
  std::vector<dust::DevStamp> as_stamps(bounds.size());
  std::vector<dust::DevCast> as_casts(bounds.size());
  for (size_t i = 0; i < bounds.size(); ++i) {
    as_stamps[i].lo = as_casts[i].lo = bounds[i].lo;
    as_stamps[i].hi = as_casts[i].hi = bounds[i].hi;
  }
  dust::CellLists lists;
  std::vector<dust::CastItem> items;
  for (const Config& c : configs) {
    std::vector<size_t> ends;
    for (size_t c0 = 0; c0 < bounds.size(); c0 = ends.back()) {
      ends.push_back(dust::chunk_end(as_stamps, c0, c.max_entries, c.max_records));
      if (dust::chunk_end(as_casts, c0, c.max_entries, c.max_records) != ends.back() || ends.back() <= c0) return 3;
    }
    put(uint32_t(ends.size()));
    size_t c0 = 0;
    for (size_t c1 : ends) {
      lists.bin(as_stamps, c0, c1);
      dust::cast_items(as_casts, c0, c1, items);
      put(uint32_t(c1)); put(uint32_t(lists.cells.size())); put(uint32_t(lists.ids.size())); put(uint32_t(items.size()));
      put_all(lists.cells); put_all(lists.starts); put_all(lists.ids); put_all(items);
      c0 = c1;
    }
  }

  for (const Decode& d : decode) put(dust::cast_hit(d.cast, d.best, d.acc));

  dust::DevEditShape whole_shape{};
  whole_shape.hi = 0xFFFFFFu;
  dust::DevCast whole_cast{};
  whole_cast.hi = 0xFFFFFFu;
  put(uint32_t(dust::chunk_end(std::vector<dust::DevEditShape>(513, whole_shape), 0, dust::kShapeChunkIds, dust::kShapeChunkRecords)));
  put(uint32_t(dust::chunk_end(std::vector<dust::DevCast>(257, whole_cast), 0, dust::kCastChunkItems, dust::kNoRecordCap)));
  put(int32_t(dust::kCastOffsetLimit));

  FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0) return 2;
  return 0;
}
