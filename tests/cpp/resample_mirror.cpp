// A fallen wall segment put down at 30 degrees through the C++ mirror (include/dust_hip.hpp): the inverse of a rotation about z written
// into a record in 1 / 65536, a dry run as the fit test, then the real call. Compiled (not run) by tests/test_resample_abi.py.
#include <cmath>
#include <vector>

#include "dust_hip.hpp"

// the record that turns the source sub-box lo..hi by `degrees` about z around its own centre and puts that centre at `at`
DustHipResample turned(const uint8_t (&lo)[3], const uint8_t (&hi)[3], const double (&at)[3], double degrees) {
  const double a = degrees * 3.14159265358979323846 / 180.0, c = std::cos(a), s = std::sin(a);
  const double inverse[3][3] = {{c, s, 0.0}, {-s, c, 0.0}, {0.0, 0.0, 1.0}};  // the rotation's transpose
  DustHipResample r{};
  double reach = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double centre = 0.5 * (double(lo[k]) + double(hi[k]) + 1.0);
    double t = centre;
    for (int j = 0; j < 3; ++j) {
      r.m[k][j] = int32_t(std::lround(inverse[k][j] * DUST_HIP_RESAMPLE_ONE));
      t -= inverse[k][j] * at[j];
    }
    r.t[k] = int32_t(std::lround(t * DUST_HIP_RESAMPLE_ONE));
    r.src_lo[k] = lo[k]; r.src_hi[k] = hi[k];
    reach += (double(hi[k]) - double(lo[k]) + 1.0) * (double(hi[k]) - double(lo[k]) + 1.0);
  }
  reach = 0.5 * std::sqrt(reach) + 1.0;  // the box's half diagonal: the image lies within it of `at`
  for (int k = 0; k < 3; ++k) {
    r.dst_lo[k] = int32_t(std::floor(at[k] - reach));
    r.dst_hi[k] = int32_t(std::ceil(at[k] + reach));
  }
  r.op = DUST_HIP_STAMP_PLACE;
  return r;
}

bool put_down(dust::VoxGeometry& world, const dust::VoxGeometry& piece, const uint8_t (&lo)[3], const uint8_t (&hi)[3], const double (&at)[3]) {
  const std::vector<DustHipResample> records{turned(lo, hi, at, 30.0)};
  const std::vector<DustHipResampleCount> fit = world.resample(piece, records, nullptr, true);
  if (fit[0].blocked != 0u || fit[0].solid == 0u) return false;
  const std::vector<DustHipResampleCount> done = world.resample(piece, records);
  static_assert(sizeof(DustHipResample) == 96 && sizeof(DustHipResampleCount) == 16 && DUST_HIP_RESAMPLE_ONE == 65536 && DUST_HIP_MAX_RESAMPLES == 65536u &&
                    DUST_HIP_RESAMPLE_DRY_RUN == 1u,
                "resample records");
  return done[0].changed == fit[0].changed;
}
