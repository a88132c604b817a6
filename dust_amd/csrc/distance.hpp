// distance.hpp -- interface between the host runtime (capi_model.cpp) and the distance fields of an editable model (distance.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dust {

constexpr uint32_t kDistanceToSolid = 0, kDistanceToEmpty = 1, kDistanceToMaterial = 2;  // DUST_HIP_DISTANCE_TO_*
constexpr uint32_t kDistanceEuclidean = 0, kDistanceChebyshev = 1;                       // DUST_HIP_DISTANCE_EUCLIDEAN, _CHEBYSHEV

// the result reduction's accumulator (8-byte aligned; zeroed by the caller)
struct DistanceAcc {
  unsigned long long best;  // max over the voxels with value != FAR of value << 32 | (0xFFFFFF - key): the largest value, at its lowest key
  uint32_t targets, far;    // voxels with value 0, with value FAR
};

// a query as the kernels read it (model_records.hpp device_distance fills target .. walls)
struct DistanceArgs {
  const uint8_t* grid;         // EditArgs::grid (brick-major); read under TO_MATERIAL only
  const uint64_t* brick_mask;  // EditArgs::brick_mask (kLattice, iter_leaf order, bit x<<4 | y<<2 | z)
  uint16_t* field;             // kLattice * 64 values, brick-major like the grid: leaf_code(bx, by, bz) * 64 + bit
  uint32_t target, metric;
  uint32_t byte;               // TO_MATERIAL: the grid byte (palette index + 1) that is a target
  uint32_t radius;             // 1..255: no pass looks further along its axis
  uint32_t limit;              // radius^2 (EUCLIDEAN) or radius (CHEBYSHEV): a value above it is FAR
  uint32_t walls;              // the voxels outside the tree are targets (folded into the last pass's store)
  DistanceAcc* acc;
};

// the three passes (x, y, z) and the result reduction; afterwards a.field is complete and a.acc holds the counts
hipError_t launch_distance_field(const DistanceArgs& a, hipStream_t s);

}  // namespace dust
