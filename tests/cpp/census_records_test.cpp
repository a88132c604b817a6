// census_records_test.cpp -- the device-free half of dust_hip_model_census driven on a CPU (tests/test_census_records.py builds this
// with g++ -ffp-contract=off under AddressSanitizer and UBSan and checks what it writes): shape_bounds against device_shape,
// census_record / census_records / census_tables (dust_amd/csrc/model_records.hpp), and the membership text both shape kernels run
// (dust_amd/csrc/shape_cover.hpp) over boxes of voxels.
//   census_records_test IN OUT
// IN : u32 n_shapes, n_acc, n_scatter, n_cover; DustHipEditShape[n_shapes]; {u32 live, pad; CensusAcc}[n_acc]; u32 index[n_scatter]
//      (ascending places among n_acc callers' shapes: census_records scatters acc[0 .. n_scatter) through it);
//      {DustHipEditShape; u32 lo[3], hi[3]}[n_cover] (hi exclusive)
// OUT: {u32 bounds_live, lo, hi; u32 shape_live; DevEditShape; u32 census_live; DevEditShape}[n_shapes]; DustHipCensus[n_acc]
//      (census_record, null for live == 0); DustHipCensus[n_acc] and u32[n_acc * 256] (census_records / census_tables of the first
//      n_scatter accumulators through index; row k holds k + 1 in bin k % 256 and 7 in bin 255);
//      per cover: u32 live, then (live only) one byte per voxel of the box, x slowest: shape_covers at its centre
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "model_records.hpp"
#include "shape_cover.hpp"

namespace {
std::vector<unsigned char> out;
template <class T>
void put(const T& v) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
  out.insert(out.end(), p, p + sizeof(T));
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

struct AccCase { uint32_t live, pad; dust::CensusAcc acc; };
struct CoverCase { DustHipEditShape shape; uint32_t lo[3], hi[3]; };
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  Reader in;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    unsigned char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) != 0;) in.bytes.insert(in.bytes.end(), buf, buf + n);
    std::fclose(f);
  } else {
    return 2;
  }
  const std::vector<uint32_t> head = in.take<uint32_t>(4);
  const std::vector<DustHipEditShape> shapes = in.take<DustHipEditShape>(head[0]);
  const std::vector<AccCase> accs = in.take<AccCase>(head[1]);
  const std::vector<uint32_t> index = in.take<uint32_t>(head[2]);
  const std::vector<CoverCase> covers = in.take<CoverCase>(head[3]);

  for (const DustHipEditShape& s : shapes) {
    uint32_t lo = 0, hi = 0;
    const uint32_t bounds_live = dust::shape_bounds(s, lo, hi) ? 1u : 0u;
    put(bounds_live); put(bounds_live ? lo : 0u); put(bounds_live ? hi : 0u);
    dust::DevEditShape d{};
    const uint32_t shape_live = dust::device_shape(s, d) ? 1u : 0u;
    put(shape_live); put(shape_live ? d : dust::DevEditShape{});
    dust::DevEditShape c{};
    const uint32_t census_live = dust::device_census_shape(s, c) ? 1u : 0u;
    put(census_live); put(census_live ? c : dust::DevEditShape{});
  }

  for (const AccCase& a : accs) put(dust::census_record(a.live ? &a.acc : nullptr));
  {
    if (index.size() > accs.size()) return 2;
    std::vector<dust::CensusAcc> live;
    std::vector<uint32_t> rows(index.size() * dust::kCensusBins, 0u);
    for (size_t k = 0; k < index.size(); ++k) {
      if (index[k] >= accs.size()) return 2;
      live.push_back(accs[k].acc);
      rows[k * dust::kCensusBins + k % dust::kCensusBins] = uint32_t(k) + 1u;
      rows[k * dust::kCensusBins + 255] += 7u;
    }
    const uint32_t n = uint32_t(accs.size());
    std::vector<DustHipCensus> records(n);
    std::vector<uint32_t> counts(size_t(n) * dust::kCensusBins, 0xDEADBEEFu);
    for (DustHipCensus& r : records) std::memset(&r, 0xEE, sizeof(r));  // (every byte of the outputs must be written)
    dust::census_records(live.data(), index, n, records.data());
    dust::census_tables(rows.data(), index, n, counts.data());
    for (const DustHipCensus& r : records) put(r);
    for (uint32_t v : counts) put(v);
  }

  for (const CoverCase& cc : covers) {
    dust::DevEditShape d{};
    const uint32_t live = dust::device_census_shape(cc.shape, d) ? 1u : 0u;
    put(live);
    if (!live) continue;
    const dust::ShapeCover cover = dust::shape_cover(d.a, d.b, d.kind, d.radius);
    for (uint32_t x = cc.lo[0]; x < cc.hi[0]; ++x)
      for (uint32_t y = cc.lo[1]; y < cc.hi[1]; ++y)
        for (uint32_t z = cc.lo[2]; z < cc.hi[2]; ++z)
          out.push_back(dust::shape_covers(cover, float(x) + 0.5f, float(y) + 0.5f, float(z) + 0.5f) ? 1 : 0);
  }

  FILE* f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
  return std::fclose(f) == 0 && ok ? 0 : 2;
}
