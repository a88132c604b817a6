// model_records.hpp -- the device-free half of the model calls (capi_model.cpp): the integer and float arithmetic that turns a caller's
// record (include/dust_hip.h) into the device's (edit.hpp, stamp.hpp, cast.hpp, distance.hpp, census.hpp, surface.hpp, mesh.hpp, boxes.hpp, body.hpp, joint.hpp, delta.hpp, column.hpp, neighbour.hpp, settle.hpp, triangle.hpp, fracture.hpp, resample.hpp), cuts a call into chunks, bins a chunk's records into
// root cells, decodes a cast's result and turns a census's accumulators into the caller's records. No HIP call, no handle, no error state:
// tests/cpp/model_records_test.cpp, tests/cpp/census_records_test.cpp, tests/cpp/surface_rule_test.cpp, tests/cpp/mesh_rule_test.cpp, tests/cpp/boxes_rule_test.cpp, tests/cpp/body_rule_test.cpp, tests/cpp/joint_rule_test.cpp, tests/cpp/delta_rule_test.cpp, tests/cpp/column_rule_test.cpp, tests/cpp/neighbour_rule_test.cpp, tests/cpp/settle_rule_test.cpp, tests/cpp/triangle_rule_test.cpp, tests/cpp/fracture_rule_test.cpp and tests/cpp/resample_rule_test.cpp drive it on a CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/dust_hip.h"
#include "body.hpp"
#include "boxes.hpp"
#include "cast.hpp"
#include "census.hpp"
#include "column.hpp"
#include "delta.hpp"
#include "distance.hpp"
#include "edit.hpp"
#include "fracture.hpp"
#include "joint.hpp"
#include "mesh.hpp"
#include "neighbour.hpp"
#include "resample.hpp"
#include "settle.hpp"
#include "stamp.hpp"
#include "surface.hpp"
#include "triangle.hpp"

namespace dust {

static_assert(sizeof(DustHipSurfaceQuery) == 48 && sizeof(DustHipSurfaceResult) == 64 && sizeof(DustHipSurfaceVoxel) == 8 && kSurfaceBins == DUST_HIP_SURFACE_BINS,
              "surface records");
static_assert(sizeof(DustHipMeshQuery) == sizeof(DustHipSurfaceQuery) && sizeof(DustHipMeshResult) == 64 && sizeof(DustHipMeshQuad) == 8 &&
                  DUST_HIP_MESH_WALLS == DUST_HIP_SURFACE_WALLS,
              "mesh records");
static_assert(sizeof(DustHipBoxesQuery) == sizeof(DustHipSurfaceQuery) && sizeof(DustHipBoxesResult) == 64 && sizeof(DustHipBox) == 8, "boxes records");
static_assert(sizeof(DustHipBodyQuery) == sizeof(DustHipSurfaceQuery) && sizeof(DustHipBody) == 96 && sizeof(DustHipBody) == sizeof(BodyRecord) &&
                  offsetof(DustHipBody, mass) == offsetof(BodyRecord, mass) && offsetof(DustHipBody, m2) == offsetof(BodyRecord, m2) &&
                  kBodiesAll == DUST_HIP_BODIES_ALL && kBodiesMaterials == DUST_HIP_BODIES_MATERIALS && kBodiesIslands == DUST_HIP_BODIES_ISLANDS &&
                  kBodiesCells == DUST_HIP_BODIES_CELLS && kBodyMaterials == DUST_HIP_BODY_WEIGHTS,
              "body records");
static_assert(sizeof(DustHipJointQuery) == sizeof(DustHipSurfaceQuery) && sizeof(DustHipJoint) == 80 && sizeof(DustHipJoint) == sizeof(JointRecord) &&
                  offsetof(DustHipJoint, by_face) == offsetof(JointRecord, by_face) && offsetof(DustHipJoint, lo2) == offsetof(JointRecord, lo2) &&
                  offsetof(DustHipJoint, sum2) == offsetof(JointRecord, sum2) && kJointsMaterials == DUST_HIP_JOINTS_MATERIALS &&
                  kJointsCells == DUST_HIP_JOINTS_CELLS && kJointRest == DUST_HIP_JOINT_REST && kJointRest == DUST_HIP_NO_CELL,
              "joint records");
static_assert(sizeof(DustHipDeltaQuery) == sizeof(DustHipSurfaceQuery) && sizeof(DustHipDeltaResult) == 64 && sizeof(DustHipDeltaVoxel) == 8 &&
                  kDeltaBins == DUST_HIP_DELTA_BINS && kDeltaMaxRecords == DUST_HIP_MAX_DELTA_RECORDS && kDeltaAdded == DUST_HIP_DELTA_ADDED &&
                  kDeltaRemoved == DUST_HIP_DELTA_REMOVED && kDeltaRepainted == DUST_HIP_DELTA_REPAINTED,
              "delta records");
static_assert(sizeof(DustHipColumnsQuery) == sizeof(DustHipSurfaceQuery) && sizeof(DustHipColumnsResult) == 64 && sizeof(DustHipColumnCell) == 4 &&
                  kColumnBins == DUST_HIP_COLUMNS_BINS && kColumnsRun == DUST_HIP_COLUMNS_RUN && kColumnsGap == DUST_HIP_COLUMNS_GAP &&
                  kColumnNoKey == DUST_HIP_COLUMNS_NO_KEY,
              "columns records");
static_assert(sizeof(DustHipNeighboursQuery) == sizeof(DustHipSurfaceQuery) && sizeof(DustHipNeighboursResult) == 64 && sizeof(DustHipNeighboursApplied) == 64 &&
                  kNeighbourFaces == DUST_HIP_NEIGHBOURS_FACES && kNeighbourEdges == DUST_HIP_NEIGHBOURS_EDGES && kNeighbourCorners == DUST_HIP_NEIGHBOURS_CORNERS &&
                  kNeighbourBins == DUST_HIP_NEIGHBOURS_BINS && kNeighbourMaxGenerations == DUST_HIP_NEIGHBOURS_MAX_GENERATIONS &&
                  DUST_HIP_NEIGHBOURS_WALLS == DUST_HIP_SURFACE_WALLS,
              "neighbours records");
static_assert(sizeof(DustHipSettleQuery) == 72 && sizeof(DustHipSettleResult) == 64 && sizeof(DustHipSettleApplied) == 64 &&
                  kSettleMaxGenerations == DUST_HIP_SETTLE_MAX_GENERATIONS,
              "settle records");

static_assert(sizeof(DustHipTriangle) == 48 && sizeof(DustHipFillMeshQuery) == 48 && sizeof(DustHipFillMeshResult) == 48 && sizeof(DevTriangle) == 52 &&
                  kTriangleUnit == DUST_HIP_TRIANGLE_UNIT && kTriangleMaxCoord == DUST_HIP_TRIANGLE_MAX_COORD,
              "triangle records");

static_assert(sizeof(DustHipFractureSeed) == 16 && sizeof(DustHipFractureSeed) == sizeof(DevFractureSeed) && sizeof(DustHipFractureQuery) == 48 &&
                  sizeof(DustHipFractureResult) == 64 && sizeof(DustHipFractureCell) == 40 && sizeof(DustHipFractureCell) == sizeof(DevFractureCell) &&
                  kFractureMaxSeeds == DUST_HIP_MAX_FRACTURE_SEEDS && kFractureNoCell == DUST_HIP_NO_CELL && kFractureNoLimit == DUST_HIP_FRACTURE_NO_LIMIT &&
                  kFractureSeedMin == DUST_HIP_FRACTURE_SEED_MIN && kFractureSeedMax == DUST_HIP_FRACTURE_SEED_MAX && kFractureMaxScale == DUST_HIP_FRACTURE_MAX_SCALE,
              "fracture records");

static_assert(sizeof(DustHipCensus) == 40 && kCensusBins == DUST_HIP_CENSUS_BINS, "census records");
static_assert(sizeof(DustHipStamp) == 32 && sizeof(DevStamp) == 32, "stamp records");
static_assert(sizeof(DustHipResample) == 96 && sizeof(DustHipResampleCount) == 16 && sizeof(DevResample) == 72 && kResampleOne == DUST_HIP_RESAMPLE_ONE &&
                  kResampleMaxM == DUST_HIP_RESAMPLE_MAX_M && kResampleMaxT == DUST_HIP_RESAMPLE_MAX_T && kResampleMaxRecords == DUST_HIP_MAX_RESAMPLES &&
                  sizeof(DustHipResampleCount) == (1 + kResampleExtra) * 4,
              "resample records");
static_assert(sizeof(DustHipCast) == 48 && sizeof(DustHipCastHit) == 32 && sizeof(DevCast) == 48 && sizeof(CastItem) == 8 && sizeof(CastAcc) == 16,
              "cast records");

constexpr size_t kShapeChunkIds = size_t(1) << 21;   // cell-list entries (u16) one launch carries: 4 MiB, 512 whole-tree shapes
constexpr size_t kShapeChunkRecords = 65536;         // ... and records: a cell lists them by u16 id
constexpr size_t kCastChunkItems = size_t(1) << 20;  // work items (8 bytes) one launch carries; a whole-tree sub-box is 4096 of them
constexpr size_t kNoRecordCap = ~size_t(0);          // (a cast's work items name their cast in 32 bits)

// ---- the caller's record -> the device's. Each returns false for a record that covers nothing: it is never sent to the device
inline bool valid_orient(uint32_t o) {
  if (o >> 9) return false;
  const uint32_t p0 = o & 3u, p1 = (o >> 2) & 3u, p2 = (o >> 4) & 3u;
  return ((1u << p0) | (1u << p1) | (1u << p2)) == 7u;
}

// Conservative voxel bounds of a shape (packed x | y << 8 | z << 16, inclusive) -- its extent padded by more than a voxel (the float32
// formulas stay within a small fraction of a voxel of the real distance for coordinates up to 65 536), clipped to the tree. false: the
// shape covers nothing (a non-finite value, a box with a > b, a radius or coordinate outside its limits, wholly outside the tree).
// `op`, `palette` and `reserved` are not looked at: the half of device_shape a census shares with an edit.
inline bool shape_bounds(const DustHipEditShape& s, uint32_t& packed_lo, uint32_t& packed_hi) {
  const bool box = s.kind == DUST_HIP_SHAPE_BOX, sphere = s.kind == DUST_HIP_SHAPE_SPHERE;
  double lo[3], hi[3];
  for (int r = 0; r < 3; ++r) {
    if (!std::isfinite(s.a[r]) || (!sphere && !std::isfinite(s.b[r]))) return false;
    if (box) {
      if (s.a[r] > s.b[r]) return false;
      lo[r] = s.a[r]; hi[r] = s.b[r];
    } else {
      if (!std::isfinite(s.radius) || s.radius < 0.0f || s.radius > 65536.0f) return false;
      if (std::fabs(s.a[r]) > 65536.0f || (!sphere && std::fabs(s.b[r]) > 65536.0f)) return false;
      const double p = s.a[r], q = sphere ? p : double(s.b[r]);
      lo[r] = std::min(p, q) - double(s.radius); hi[r] = std::max(p, q) + double(s.radius);
    }
  }
  uint32_t vlo[3], vhi[3];
  for (int r = 0; r < 3; ++r) {  // voxel x is covered when lo <= x + 0.5 <= hi
    const double l = std::floor(lo[r] - 0.5) - 1.0, h = std::ceil(hi[r] - 0.5) + 1.0;
    if (l > 255.0 || h < 0.0) return false;
    vlo[r] = l < 0.0 ? 0u : uint32_t(l);
    vhi[r] = h > 255.0 ? 255u : uint32_t(h);
  }
  packed_lo = vlo[0] | (vlo[1] << 8) | (vlo[2] << 16);
  packed_hi = vhi[0] | (vhi[1] << 8) | (vhi[2] << 16);
  return true;
}
// ... and the shape itself as the membership text (shape_cover.hpp) reads it: a box without a radius, a sphere's b its centre
inline void device_shape_geometry(const DustHipEditShape& s, DevEditShape& d) {
  std::memcpy(d.a, s.a, sizeof(d.a)); std::memcpy(d.b, s.b, sizeof(d.b));
  d.kind = s.kind;
  d.radius = s.kind == DUST_HIP_SHAPE_BOX ? 0.0f : s.radius;
  if (s.kind == DUST_HIP_SHAPE_SPHERE) std::memcpy(d.b, s.a, sizeof(d.b));
}

// A shape edit's record: the bounds, the geometry and the two grid bytes of the operation.
inline bool device_shape(const DustHipEditShape& s, DevEditShape& d) {
  uint32_t lo, hi;
  if (!shape_bounds(s, lo, hi)) return false;
  device_shape_geometry(s, d);
  const uint32_t byte = uint32_t(s.palette) + 1u;
  switch (s.op) {
    case DUST_HIP_EDIT_CARVE: d.solid_to = 0; d.empty_to = 0; break;
    case DUST_HIP_EDIT_FILL: d.solid_to = byte; d.empty_to = byte; break;
    case DUST_HIP_EDIT_PAINT: d.solid_to = byte; d.empty_to = 0; break;
    default: d.solid_to = kEditKeep; d.empty_to = byte; break;  // PLACE
  }
  d.lo = lo; d.hi = hi;
  return true;
}

// A census's record (dust_hip_model_census): the same bounds and geometry; the operation is ignored, its two bytes stay 0.
inline bool device_census_shape(const DustHipEditShape& s, DevEditShape& d) {
  if (!shape_bounds(s, d.lo, d.hi)) return false;
  device_shape_geometry(s, d);
  d.solid_to = d.empty_to = 0;
  return true;
}

// What a census's caller gets from the device's accumulator; null: a shape that covers nothing -- the zero record, bounds 255 / 0
// (what a shape whose covered voxels are all empty has too).
inline DustHipCensus census_record(const CensusAcc* acc) {
  DustHipCensus c{};
  const bool solid = acc && acc->solid != 0u;
  for (int r = 0; r < 3; ++r) {
    c.lo[r] = solid ? uint8_t(acc->lo[r]) : uint8_t(255);
    c.hi[r] = solid ? uint8_t(acc->hi[r]) : uint8_t(0);
    c.sum[r] = solid ? acc->sum[r] : 0u;
  }
  if (acc) { c.covered = acc->covered; c.solid = acc->solid; }
  return c;
}
// the n records of a call: those of its live shapes (acc[k] belongs to the caller's shape index[k]), the zero record for the rest
inline void census_records(const CensusAcc* acc, const std::vector<uint32_t>& index, uint32_t n, DustHipCensus* records) {
  for (uint32_t i = 0; i < n; ++i) records[i] = census_record(nullptr);
  for (size_t k = 0; k < index.size(); ++k) records[index[k]] = census_record(acc + k);
}
// ... and its n rows of per-material counts (DUST_HIP_CENSUS_BINS each): zero rows for the shapes that cover nothing
inline void census_tables(const uint32_t* rows, const std::vector<uint32_t>& index, uint32_t n, uint32_t* counts) {
  std::fill(counts, counts + size_t(n) * kCensusBins, 0u);
  for (size_t k = 0; k < index.size(); ++k) std::memcpy(counts + size_t(index[k]) * kCensusBins, rows + k * kCensusBins, kCensusBins * 4);
}

// A stamp's operation as the kernels read it: two bits per case (source solid) << 1 | (destination solid) -- keep the destination's
// byte, take the source's, or None. (dust_hip_model_resample's records carry the same ops and the same table.)
inline uint32_t stamp_table(uint32_t op) {
  const uint32_t K = kStampKeep, T = kStampTake, N = kStampClear;
  auto table = [](uint32_t ee, uint32_t es, uint32_t se, uint32_t ss) { return ee | (es << 2) | (se << 4) | (ss << 6); };
  switch (op) {
    case DUST_HIP_STAMP_PLACE: return table(K, K, T, K);
    case DUST_HIP_STAMP_OVERWRITE: return table(K, K, T, T);
    case DUST_HIP_STAMP_REPLACE: return table(T, T, T, T);
    case DUST_HIP_STAMP_CARVE: return table(K, K, K, N);
    default: return table(K, K, K, T);  // PAINT
  }
}

// The image box clipped to the tree, one affine map per destination axis, the operation as a table. Everything in int64: any int32
// offset is legal.
inline bool device_stamp(const DustHipStamp& s, DevStamp& d) {
  for (int k = 0; k < 3; ++k)
    if (s.src_lo[k] > s.src_hi[k]) return false;
  uint32_t lo[3], hi[3];
  for (int r = 0; r < 3; ++r) {
    const uint32_t p = (s.orient >> (2 * r)) & 3u;
    const bool flip = (s.orient >> (6 + r)) & 1u;
    const int64_t off = s.offset[r], first = std::max<int64_t>(off, 0), last = std::min<int64_t>(off + int64_t(s.src_hi[p] - s.src_lo[p]), 255);
    if (first > last) return false;
    lo[r] = uint32_t(first); hi[r] = uint32_t(last);
    d.base[r] = int32_t(flip ? int64_t(s.src_hi[p]) + off : int64_t(s.src_lo[p]) - off);  // (|off| <= 255 here)
  }
  d.lo = lo[0] | (lo[1] << 8) | (lo[2] << 16);
  d.hi = hi[0] | (hi[1] << 8) | (hi[2] << 16);
  d.orient = s.orient;
  d.table = stamp_table(s.op);
  d.pad = 0;
  return true;
}

// Everything in int64: any int32 offset is legal. Per destination axis the placements at which the image box meets the tree are an
// interval; their intersection, cut to 0..max_steps, is all the device walks (under WALLS: from 0 to one past the last placement the
// image is inside, or placement 0 alone when it begins outside). false: the sub-box is empty.
inline bool device_cast(const DustHipCast& s, DevCast& d) {
  for (int k = 0; k < 3; ++k)
    if (s.src_lo[k] > s.src_hi[k]) return false;
  const bool walls = s.flags & DUST_HIP_CAST_WALLS;
  const bool still = s.step[0] == 0 && s.step[1] == 0 && s.step[2] == 0;
  const int64_t max_steps = still ? 0 : int64_t(s.max_steps);  // (every placement is placement 0)
  const int64_t never = int64_t(1) << 40;                      // beyond any placement
  int64_t first = -never, last = never;
  for (int r = 0; r < 3; ++r) {
    const uint32_t p = (s.orient >> (2 * r)) & 3u;
    const int64_t off = s.offset[r], ext = int64_t(s.src_hi[p]) - int64_t(s.src_lo[p]);
    int64_t f, l;
    if (s.step[r] == 0) {
      const bool meets = off + ext >= 0 && off <= 255;
      f = meets ? -never : 1; l = meets ? never : 0;
    } else if (s.step[r] > 0) {
      f = -(off + ext); l = 255 - off;
    } else {
      f = off - 255; l = off + ext;
    }
    first = std::max(first, f); last = std::min(last, l);
    d.off[r] = int32_t(std::clamp<int64_t>(off, -kCastOffsetLimit, kCastOffsetLimit));
    d.step[r] = s.step[r];
  }
  int64_t k_lo, k_hi;
  if (walls) {
    k_lo = 0;
    k_hi = first <= 0 && last >= 0 ? std::min(max_steps, last + 1) : 0;
  } else {
    k_lo = std::max<int64_t>(first, 0);
    k_hi = std::min(last, max_steps);
  }
  if (k_lo > k_hi) { k_lo = 1; k_hi = 0; }  // nothing to walk (the piece's voxels are still counted)
  d.k_lo = uint32_t(k_lo); d.k_hi = uint32_t(k_hi);
  d.max_steps = uint32_t(max_steps);
  d.orient = s.orient | (walls ? kCastWalls : 0u);
  d.lo = s.src_lo[0] | (uint32_t(s.src_lo[1]) << 8) | (uint32_t(s.src_lo[2]) << 16);
  d.hi = s.src_hi[0] | (uint32_t(s.src_hi[1]) << 8) | (uint32_t(s.src_hi[2]) << 16);
  return true;
}

// What a cast's caller gets: `best` is the device's minimum of (first blocked placement << 24 | source key), `acc` its counts. A cast
// that never ran (no sub-box: kCastNoHit and a zero acc) or found nothing comes back with steps == max_steps and no key.
inline DustHipCastHit cast_hit(const DustHipCast& c, unsigned long long best, const CastAcc& acc) {
  DustHipCastHit h{};
  h.steps = c.max_steps;
  h.src_key = DUST_HIP_CAST_NO_KEY;
  h.voxels = acc.voxels;
  if (best == kCastNoHit) return h;
  const uint32_t k = uint32_t(best >> 24), key = uint32_t(best & 0xFFFFFFu);
  const uint32_t sv[3] = {key >> 16, (key >> 8) & 255u, key & 255u};
  h.flags = DUST_HIP_CAST_HIT | (k == 0 ? DUST_HIP_CAST_OVERLAP : 0u) | (acc.wall ? DUST_HIP_CAST_HIT_WALL : 0u);
  h.steps = k ? k - 1 : 0;
  h.contacts = acc.contacts;
  h.src_key = key;
  for (int r = 0; r < 3; ++r) {
    const uint32_t p = (c.orient >> (2 * r)) & 3u;
    const int64_t u = ((c.orient >> (6 + r)) & 1u) ? int64_t(c.src_hi[p]) - int64_t(sv[p]) : int64_t(sv[p]) - int64_t(c.src_lo[p]);
    h.contact[r] = int32_t(uint32_t(uint64_t(int64_t(c.offset[r]) + int64_t(k) * c.step[r] + u)));  // (the low 32 bits)
  }
  return h;
}

// A distance query as the kernels read it: the target byte, the radius no pass looks beyond and the limit in the field's own units
// (squared under EUCLIDEAN). The pointers and the accumulator are the caller's. false: a query the call refuses.
inline bool device_distance(const DustHipDistanceQuery& q, DistanceArgs& d) {
  if (q.target > DUST_HIP_DISTANCE_TO_MATERIAL || q.metric > DUST_HIP_DISTANCE_CHEBYSHEV || (q.flags & ~DUST_HIP_DISTANCE_WALLS) != 0u) return false;
  if (q.target == DUST_HIP_DISTANCE_TO_MATERIAL && (q.palette < 0 || q.palette > 254)) return false;
  if (q.max_radius == 0u || q.max_radius > DUST_HIP_DISTANCE_MAX_RADIUS) return false;
  d.target = q.target;
  d.metric = q.metric;
  d.byte = q.target == DUST_HIP_DISTANCE_TO_MATERIAL ? uint32_t(q.palette) + 1u : 0u;
  d.radius = q.max_radius;
  d.limit = q.metric == DUST_HIP_DISTANCE_EUCLIDEAN ? q.max_radius * q.max_radius : q.max_radius;
  d.walls = (q.flags & DUST_HIP_DISTANCE_WALLS) ? 1u : 0u;
  return true;
}
// What a distance call's caller gets from the reduction's accumulator (2^24 voxels in all).
inline DustHipDistanceResult distance_result(const DistanceAcc& acc) {
  DustHipDistanceResult r{};
  r.targets = acc.targets;
  r.far = acc.far;
  r.near = (1u << 24) - acc.targets - acc.far;
  r.largest_key = DUST_HIP_DISTANCE_NO_KEY;
  if (r.targets + r.near != 0u) {
    r.largest = uint32_t(acc.best >> 32);
    r.largest_key = 0xFFFFFFu - uint32_t(acc.best & 0xFFFFFFu);
  }
  return r;
}

// A surface query as the kernels read it (dust_hip_model_surface, _surface_apply): the directions, the walls, the filter's grid byte,
// the region clipped to the tree and the root cells it reaches. The pointers are the caller's. nullptr: the query is fine; otherwise
// why the call refuses it. `empty` (lo > hi on an axis): legal, nothing is looked at and no launch is made -- lo, hi and box are not set.
inline const char* device_surface(const DustHipSurfaceQuery& q, SurfaceArgs& d, bool& empty) {
  if (q.faces == 0u || q.faces > DUST_HIP_FACES_ALL) return "faces must be 1..DUST_HIP_FACES_ALL";
  if ((q.flags & ~DUST_HIP_SURFACE_WALLS) != 0u) return "unknown surface flag";
  if (q.palette < -1 || q.palette > 254) return "palette must be -1 (every solid voxel) or 0..254";
  for (int r = 0; r < 3; ++r)
    if (q.lo[r] >= 256u || q.hi[r] >= 256u) return "region coordinate outside the tree extent";
  d.faces = q.faces;
  d.walls = (q.flags & DUST_HIP_SURFACE_WALLS) ? 1u : 0u;
  d.byte = q.palette < 0 ? 0u : uint32_t(q.palette) + 1u;
  empty = false;
  for (int r = 0; r < 3; ++r) empty |= q.lo[r] > q.hi[r];
  if (empty) return nullptr;
  for (int r = 0; r < 3; ++r) {
    d.lo[r] = q.lo[r]; d.hi[r] = q.hi[r];
    d.box.lo[r] = q.lo[r] >> 4; d.box.hi[r] = q.hi[r] >> 4;
  }
  return nullptr;
}
// What a surface call's caller gets from the device's kSurfaceAccWords accumulator; null: nothing was looked at -- the zero result,
// bounds 255 / 0 (what a region without a listed voxel has too).
inline DustHipSurfaceResult surface_result(const uint32_t* acc) {
  DustHipSurfaceResult r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  if (!acc) return r;
  r.voxels = acc[0];
  for (int d = 0; d < 6; ++d) { r.by_face[d] = acc[1 + d]; r.faces += acc[1 + d]; }
  r.solid = acc[7];
  for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - acc[8 + k]); r.hi[k] = uint8_t(acc[11 + k]); }
  return r;
}

// A mesh query as the kernels read it (dust_hip_model_mesh): a surface query field for field -- device_surface's refusals, WALLS, filter
// and clipped region -- with one flag more. nullptr: the query is fine; otherwise why the call refuses it. `empty` as in device_surface.
inline const char* device_mesh(const DustHipMeshQuery& q, MeshArgs& d, bool& empty) {
  DustHipSurfaceQuery sq{};
  sq.struct_size = sizeof(sq);
  sq.faces = q.faces;
  sq.flags = q.flags & DUST_HIP_MESH_WALLS;
  sq.palette = q.palette;
  for (int r = 0; r < 3; ++r) { sq.lo[r] = q.lo[r]; sq.hi[r] = q.hi[r]; }
  SurfaceArgs s{};
  if (const char* why = device_surface(sq, s, empty)) return why;
  if ((q.flags & ~(DUST_HIP_MESH_WALLS | DUST_HIP_MESH_ANY_PALETTE)) != 0u) return "unknown mesh flag";
  d.faces = s.faces;
  d.walls = s.walls;
  d.byte = s.byte;
  d.any_palette = (q.flags & DUST_HIP_MESH_ANY_PALETTE) ? 1u : 0u;
  for (int r = 0; r < 3; ++r) { d.lo[r] = s.lo[r]; d.hi[r] = s.hi[r]; }  // (not set when empty)
  return nullptr;
}
// What a mesh call's caller gets from the device's kMeshAccWords accumulator; null: nothing was looked at -- the zero result.
inline DustHipMeshResult mesh_result(const uint32_t* acc) {
  DustHipMeshResult r{};
  if (!acc) return r;
  for (int d = 0; d < 6; ++d) {
    r.quads_by_face[d] = acc[d]; r.quads += acc[d];
    r.faces_by_face[d] = acc[6 + d]; r.faces += acc[6 + d];
  }
  r.largest = acc[12];
  return r;
}

// A boxes query as the kernels read it (dust_hip_model_boxes): the stacking axis, the filter's grid byte and the region clipped to the
// tree. nullptr: the query is fine; otherwise why the call refuses it, in the header's order. `empty` as in device_surface: nothing is
// looked at and no launch is made -- lo and hi are not set.
inline const char* device_boxes(const DustHipBoxesQuery& q, BoxesArgs& d, bool& empty) {
  if (q.axis > 2u) return "axis must be 0..2";
  if ((q.flags & ~DUST_HIP_BOXES_ANY_PALETTE) != 0u) return "unknown boxes flag";
  if (q.palette < -1 || q.palette > 254) return "palette must be -1 (every solid voxel) or 0..254";
  for (int r = 0; r < 3; ++r)
    if (q.lo[r] >= 256u || q.hi[r] >= 256u) return "region coordinate outside the tree extent";
  d.axis = q.axis;
  d.byte = q.palette < 0 ? 0u : uint32_t(q.palette) + 1u;
  d.any_palette = (q.flags & DUST_HIP_BOXES_ANY_PALETTE) ? 1u : 0u;
  empty = false;
  for (int r = 0; r < 3; ++r) empty |= q.lo[r] > q.hi[r];
  if (empty) return nullptr;
  for (int r = 0; r < 3; ++r) { d.lo[r] = q.lo[r]; d.hi[r] = q.hi[r]; }
  return nullptr;
}
// What a boxes call's caller gets from the device's kBoxesAccWords accumulator; null: nothing was looked at -- the zero result, bounds
// 255 / 0 (what a region without a solid voxel has too).
inline DustHipBoxesResult boxes_result(const uint32_t* acc) {
  DustHipBoxesResult r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  if (!acc) return r;
  r.boxes = acc[0] - acc[1];
  r.rects = acc[0];
  r.voxels = acc[2];
  for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - acc[3 + k]); r.hi[k] = uint8_t(acc[6 + k]); }
  return r;
}

// A body query as the kernels read it (dust_hip_model_bodies): the group kind, the filter's grid byte, the region and the root cells it
// reaches. nullptr: the query is fine; otherwise why the call refuses it, in the header's order. `empty` as in device_surface: no voxel
// is looked at -- lo, hi and box are not set.
inline const char* device_bodies(const DustHipBodyQuery& q, BodyArgs& d, bool& empty) {
  if (q.group > DUST_HIP_BODIES_CELLS) return "unknown body group";
  if (q.flags != 0u) return "unknown bodies flag";
  if (q.reserved[0] != 0u || q.reserved[1] != 0u) return "reserved word not 0";
  if (q.palette < -1 || q.palette > 254) return "palette must be -1 (every solid voxel) or 0..254";
  for (int r = 0; r < 3; ++r)
    if (q.lo[r] >= 256u || q.hi[r] >= 256u) return "region coordinate outside the tree extent";
  d.group = q.group;
  d.byte = q.palette < 0 ? 0u : uint32_t(q.palette) + 1u;
  empty = false;
  for (int r = 0; r < 3; ++r) empty |= q.lo[r] > q.hi[r];
  if (empty) return nullptr;
  for (int r = 0; r < 3; ++r) {
    d.lo[r] = q.lo[r]; d.hi[r] = q.hi[r];
    d.box.lo[r] = q.lo[r] >> 4; d.box.hi[r] = q.hi[r] >> 4;
  }
  return nullptr;
}

// A joint query as the kernels read it (dust_hip_model_joints): the group kind, the region clipped to the tree as device_columns clips it
// (a coordinate past 255 is cut back to it; lo past hi is the empty region) and the root cells it reaches. nullptr: the query is fine;
// otherwise why the call refuses it, in the header's order. `empty`: no voxel is looked at -- lo, hi and box are not set.
inline const char* device_joints(const DustHipJointQuery& q, JointArgs& d, bool& empty) {
  if (q.group > DUST_HIP_JOINTS_CELLS) return "unknown joint group";
  if (q.flags != 0u) return "unknown joints flag";
  if (q.reserved[0] != 0u || q.reserved[1] != 0u) return "reserved word not 0";
  if (q.palette != -1) return "palette must be -1 (reserved for a later filter)";
  d.group = q.group;
  uint32_t lo[3], hi[3];
  empty = false;
  for (int r = 0; r < 3; ++r) {
    lo[r] = q.lo[r]; hi[r] = std::min(q.hi[r], 255u);
    empty |= lo[r] > hi[r];
  }
  if (empty) return nullptr;
  for (int r = 0; r < 3; ++r) {
    d.lo[r] = lo[r]; d.hi[r] = hi[r];
    d.box.lo[r] = lo[r] >> 4; d.box.hi[r] = hi[r] >> 4;
  }
  return nullptr;
}

// A delta query as the kernels read it (dust_hip_model_delta): the kinds, the filter's grid byte, the region clipped to the tree and the
// root cells it reaches. The pointers are the caller's. nullptr: the query is fine; otherwise why the call refuses it, in the header's
// order. `empty` as in device_surface: nothing is looked at and no launch is made -- lo, hi and box are not set.
inline const char* device_delta(const DustHipDeltaQuery& q, DeltaArgs& d, bool& empty) {
  if (q.kinds == 0u || q.kinds > DUST_HIP_DELTA_ALL) return "kinds must be 1..DUST_HIP_DELTA_ALL";
  if (q.flags != 0u) return "unknown delta flag";
  if (q.palette < -1 || q.palette > 254) return "palette must be -1 (every change) or 0..254";
  for (int r = 0; r < 3; ++r)
    if (q.lo[r] >= 256u || q.hi[r] >= 256u) return "region coordinate outside the tree extent";
  d.kinds = q.kinds;
  d.byte = q.palette < 0 ? 0u : uint32_t(q.palette) + 1u;
  empty = false;
  for (int r = 0; r < 3; ++r) empty |= q.lo[r] > q.hi[r];
  if (empty) return nullptr;
  for (int r = 0; r < 3; ++r) {
    d.lo[r] = q.lo[r]; d.hi[r] = q.hi[r];
    d.box.lo[r] = q.lo[r] >> 4; d.box.hi[r] = q.hi[r] >> 4;
  }
  return nullptr;
}
// What a delta call's caller gets from the device's kDeltaAccWords accumulator; null: nothing was looked at -- the zero result, bounds
// 255 / 0 (what a pair without a listed voxel has too).
inline DustHipDeltaResult delta_result(const uint32_t* acc) {
  DustHipDeltaResult r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  if (!acc) return r;
  r.added = acc[0]; r.removed = acc[1]; r.repainted = acc[2];
  r.voxels = acc[0] + acc[1] + acc[2];
  r.solid_before = acc[3]; r.solid_after = acc[4];
  for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - acc[5 + k]); r.hi[k] = uint8_t(acc[8 + k]); }
  return r;
}
// The records of a dust_hip_model_delta_apply call as k_delta_apply takes them: one 64-bit word each, a key named more than once
// keeping its LAST record (set_voxels' rule, and its walk: from the back, first come first kept). Seen keys are a bit each of the
// tree's 2^24 (2 MiB): a list may name every voxel, and a hash set took 0.6 s over the 12.6 M records of a half-density pair.
// nullptr: fine; otherwise why the call refuses them, `out` left alone.
inline const char* delta_apply_records(const DustHipDeltaVoxel* records, uint32_t n, std::vector<uint64_t>& out) {
  for (uint32_t i = 0; i < n; ++i)
    if (records[i].key >= (1u << 24)) return "record key outside the tree extent (x << 16 | y << 8 | z)";
  out.clear();
  if (n == 0) return nullptr;
  out.reserve(n);
  std::vector<uint64_t> seen(size_t(1) << 18, 0ull);
  for (uint32_t k = n; k-- > 0;) {
    const DustHipDeltaVoxel& v = records[k];
    uint64_t& word = seen[v.key >> 6];
    const uint64_t bit = 1ull << (v.key & 63u);
    if (word & bit) continue;
    word |= bit;
    out.push_back(uint64_t(v.key) | (uint64_t(v.kind) << 32) | (uint64_t(v.before) << 40) | (uint64_t(v.after) << 48));
  }
  return nullptr;
}

// A columns query as the kernels read it (dust_hip_model_columns, _columns_apply): the axis and the end the walk starts at, the filter's
// grid byte, the layer, the region clipped to the tree (a coordinate past 255 is cut back to it; lo past hi is the empty region) and the
// root-cell columns it reaches in the (u, v) plane. The pointers are the caller's. nullptr: the query is fine; otherwise why the call
// refuses it, in the header's order. `nu`, `nv`: the size of the map, 0 x 0 when `empty` -- then nothing is looked at, no launch is
// made and the region fields are not set.
inline const char* device_columns(const DustHipColumnsQuery& q, ColumnArgs& d, bool& empty, uint32_t& nu, uint32_t& nv) {
  if (q.face == 0u || q.face > DUST_HIP_FACES_ALL || (q.face & (q.face - 1u)) != 0u) return "face must be exactly one DUST_HIP_FACE_* bit";
  if (q.flags != 0u) return "unknown columns flag";
  if (q.reserved != 0u) return "reserved word not 0";
  if (q.palette < -1 || q.palette > 254) return "palette must be -1 (every solid voxel) or 0..254";
  if (q.layer > 255u) return "layer must be 0..255";
  uint32_t index = 0;  // the direction's index: -x, +x, -y, +y, -z, +z
  while ((q.face >> index) != 1u) ++index;
  d.axis = index >> 1;
  d.from_high = index & 1u;
  d.byte = q.palette < 0 ? 0u : uint32_t(q.palette) + 1u;
  d.layer = q.layer;
  uint32_t lo[3], hi[3];
  empty = false;
  for (int r = 0; r < 3; ++r) {
    lo[r] = q.lo[r]; hi[r] = std::min(q.hi[r], 255u);
    empty |= lo[r] > hi[r];
  }
  nu = nv = 0;
  if (empty) return nullptr;
  const uint32_t ua = column_u_axis(d.axis), va = column_v_axis(d.axis);
  d.lo_n = lo[d.axis]; d.hi_n = hi[d.axis];
  d.lo_u = lo[ua]; d.hi_u = hi[ua];
  d.lo_v = lo[va]; d.hi_v = hi[va];
  d.cell_u = d.lo_u >> 4; d.cells_u = (d.hi_u >> 4) - d.cell_u + 1u;
  d.cell_v = d.lo_v >> 4; d.cells_v = (d.hi_v >> 4) - d.cell_v + 1u;
  nu = d.hi_u - d.lo_u + 1u; nv = d.hi_v - d.lo_v + 1u;
  return nullptr;
}
// what dust_hip_model_columns_apply refuses beyond the query
inline const char* columns_apply_arguments(uint32_t where, uint32_t depth, int32_t value) {
  if (where > DUST_HIP_COLUMNS_GAP) return "where must be DUST_HIP_COLUMNS_RUN or DUST_HIP_COLUMNS_GAP";
  if (depth == 0u || depth > 256u) return "depth must be 1..256";
  if (value < -1 || value > 254) return "value must be -1 (None) or a palette index 0..254";
  return nullptr;
}
// What a columns call's caller gets from the device's kColumnAccWords accumulator and the size of the map; null: nothing was looked
// at -- the zero result, keys DUST_HIP_COLUMNS_NO_KEY, bounds 255 / 0 (what a region without a hit column has too, beside its columns
// and runs).
inline DustHipColumnsResult columns_result(const uint32_t* acc, uint32_t nu, uint32_t nv) {
  DustHipColumnsResult r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  r.nearest_key = r.farthest_key = kColumnNoKey;
  if (!acc) return r;
  r.columns = nu * nv;
  r.hit = acc[0]; r.voxels = acc[1]; r.runs = acc[2]; r.depth_sum = acc[3];
  if (r.hit != 0u) {
    r.nearest_key = column_near_key(acc[4]);
    r.farthest_key = column_far_key(acc[5]);
  }
  for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - acc[6 + k]); r.hi[k] = uint8_t(acc[9 + k]); }
  return r;
}

// A neighbours query as the kernels read it (dust_hip_model_neighbours, _neighbours_apply): the neighbourhood, the walls, the two masks,
// the region and the root cells it reaches; `byte` and `majority` are what a born voxel takes (an apply's). The pointers are the
// caller's. nullptr: the query is fine; otherwise why the call refuses it, in the header's order. `empty` as in device_surface: nothing
// is looked at and no launch is made -- lo, hi and box are not set.
inline const char* device_neighbours(const DustHipNeighboursQuery& q, NeighbourArgs& d, uint32_t& byte, uint32_t& majority, bool& empty) {
  if (q.neighbourhood != kNeighbourFaces && q.neighbourhood != kNeighbourEdges && q.neighbourhood != kNeighbourCorners)
    return "neighbourhood must be DUST_HIP_NEIGHBOURS_FACES, _EDGES or _CORNERS";
  if ((q.flags & ~(DUST_HIP_NEIGHBOURS_WALLS | DUST_HIP_NEIGHBOURS_MAJORITY)) != 0u) return "unknown neighbours flag";
  if (q.palette < 0 || q.palette > 254) return "palette must be 0..254";
  const uint32_t known = (2u << q.neighbourhood) - 1u;  // bits 0..neighbourhood
  if ((q.birth & ~known) != 0u || (q.survive & ~known) != 0u) return "birth or survive bit above the neighbourhood's size";
  for (int r = 0; r < 3; ++r)
    if (q.lo[r] >= 256u || q.hi[r] >= 256u) return "region coordinate outside the tree extent";
  d.neighbourhood = q.neighbourhood;
  d.walls = (q.flags & DUST_HIP_NEIGHBOURS_WALLS) ? 1u : 0u;
  d.birth = q.birth;
  d.survive = q.survive;
  byte = uint32_t(q.palette) + 1u;
  majority = (q.flags & DUST_HIP_NEIGHBOURS_MAJORITY) ? 1u : 0u;
  empty = false;
  for (int r = 0; r < 3; ++r) empty |= q.lo[r] > q.hi[r];
  if (empty) return nullptr;
  for (int r = 0; r < 3; ++r) {
    d.lo[r] = q.lo[r]; d.hi[r] = q.hi[r];
    d.box.lo[r] = q.lo[r] >> 4; d.box.hi[r] = q.hi[r] >> 4;
  }
  return nullptr;
}
// what dust_hip_model_neighbours_apply refuses beyond the query
inline const char* neighbours_apply_arguments(uint32_t generations) {
  if (generations == 0u || generations > kNeighbourMaxGenerations) return "generations must be 1..DUST_HIP_NEIGHBOURS_MAX_GENERATIONS";
  return nullptr;
}
// What a neighbours call's caller gets from the device's kNeighbourAccWords accumulator; null: nothing was looked at -- the zero
// result, bounds 255 / 0 (what a region in which nothing would change has too).
inline DustHipNeighboursResult neighbours_result(const uint32_t* acc) {
  DustHipNeighboursResult r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  if (!acc) return r;
  r.voxels = acc[0]; r.solid = acc[1]; r.born = acc[2]; r.died = acc[3];
  for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - acc[4 + k]); r.hi[k] = uint8_t(acc[7 + k]); }
  return r;
}
// What an apply's caller gets from the device's array of `generations` slots (kNeighbourSlotWords each: a generation that never ran
// left its slot 0) and the solid voxels the first generation found; null: nothing was looked at -- the zero record. per_generation
// (may be null): 2 * generations words, born and died per generation.
inline DustHipNeighboursApplied neighbours_applied(const uint32_t* slots, uint32_t generations, uint32_t solid_before, uint32_t* per_generation) {
  DustHipNeighboursApplied r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  if (per_generation) std::fill(per_generation, per_generation + size_t(generations) * 2, 0u);
  if (!slots) return r;
  uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // (lo as 255 - the bound)
  for (uint32_t g = 0; g < generations; ++g) {
    const uint32_t* s = slots + size_t(g) * kNeighbourSlotWords;
    if (s[0] + s[1] == 0u) continue;  // (a fixed point: no later generation changes anything either)
    r.generations = g + 1u;
    r.born += s[0]; r.died += s[1];
    for (int k = 0; k < 3; ++k) { lo[k] = std::max(lo[k], s[2 + k]); hi[k] = std::max(hi[k], s[5 + k]); }
    if (per_generation) { per_generation[2 * g] = s[0]; per_generation[2 * g + 1] = s[1]; }
  }
  r.solid_before = solid_before;
  r.solid_after = uint32_t(uint64_t(solid_before) + r.born - r.died);
  for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - lo[k]); r.hi[k] = uint8_t(hi[k]); }
  return r;
}

// A settle query as the kernels read it (dust_hip_model_settle, _settle_apply): the axis and the end things fall toward, the region and
// the root-cell columns it reaches in the (u, v) plane; `box` the root cells it reaches; `all_loose`: every palette index is loose (the
// loose masks are the brick masks then). The pointers are the caller's. nullptr: the query is fine; otherwise why the call refuses it, in
// the header's order. `nu`, `nv`: the columns of the region along u and v, 0 x 0 when `empty` -- then nothing is looked at, no launch is
// made and the region fields are not set.
inline const char* device_settle(const DustHipSettleQuery& q, SettleArgs& d, CellBox& box, bool& all_loose, bool& empty, uint32_t& nu, uint32_t& nv) {
  if (q.toward == 0u || q.toward > DUST_HIP_FACES_ALL || (q.toward & (q.toward - 1u)) != 0u) return "toward must be exactly one DUST_HIP_FACE_* bit";
  if (q.flags != 0u) return "unknown settle flag";
  if (q.reserved != 0u) return "reserved word not 0";
  for (int r = 0; r < 3; ++r)
    if (q.lo[r] >= 256u || q.hi[r] >= 256u) return "region coordinate outside the tree extent";
  if ((q.loose[7] >> 31) != 0u) return "loose bit 255 is set (palette indices are 0..254)";
  uint32_t index = 0;  // the direction's index: -x, +x, -y, +y, -z, +z
  while ((q.toward >> index) != 1u) ++index;
  d.axis = index >> 1;
  d.from_high = index & 1u;
  all_loose = q.loose[7] == 0x7FFFFFFFu;
  for (int w = 0; w < 7; ++w) all_loose &= q.loose[w] == 0xFFFFFFFFu;
  empty = false;
  for (int r = 0; r < 3; ++r) empty |= q.lo[r] > q.hi[r];
  nu = nv = 0;
  if (empty) return nullptr;
  const uint32_t ua = column_u_axis(d.axis), va = column_v_axis(d.axis);
  d.lo_n = q.lo[d.axis]; d.hi_n = q.hi[d.axis];
  d.lo_u = q.lo[ua]; d.hi_u = q.hi[ua];
  d.lo_v = q.lo[va]; d.hi_v = q.hi[va];
  d.cell_u = d.lo_u >> 4; d.cells_u = (d.hi_u >> 4) - d.cell_u + 1u;
  d.cell_v = d.lo_v >> 4; d.cells_v = (d.hi_v >> 4) - d.cell_v + 1u;
  nu = d.hi_u - d.lo_u + 1u; nv = d.hi_v - d.lo_v + 1u;
  for (int r = 0; r < 3; ++r) { box.lo[r] = q.lo[r] >> 4; box.hi[r] = q.hi[r] >> 4; }
  return nullptr;
}
// what dust_hip_model_settle_apply refuses beyond the query
inline const char* settle_apply_arguments(uint32_t generations) {
  if (generations > kSettleMaxGenerations) return "generations must be 0..DUST_HIP_SETTLE_MAX_GENERATIONS";
  return nullptr;
}
// the slide of generation k: along +u, -u, +v, -v of the fall's axis for k mod 4 = 0, 1, 2, 3
inline void settle_slide_direction(uint32_t axis, uint32_t k, uint32_t& d_axis, uint32_t& d_up) {
  d_axis = (k & 2u) ? column_v_axis(axis) : column_u_axis(axis);
  d_up = (k & 1u) ? 0u : 1u;
}
// the bounds of one step's record into a running pair (lo as 255 - the bound)
inline void settle_fold_bounds(const uint32_t* acc, uint32_t (&lo)[3], uint32_t (&hi)[3]) {
  for (int k = 0; k < 3; ++k) { lo[k] = std::max(lo[k], acc[kSettleLo + k]); hi[k] = std::max(hi[k], acc[kSettleHi + k]); }
}
// What a settle call's caller gets from the device's kSettleAccWords accumulator and the size of the region; null: nothing was looked
// at -- the zero result, bounds 255 / 0 (what a region in which nothing would move has too, beside its columns and counts).
inline DustHipSettleResult settle_result(const uint32_t* acc, uint32_t nu, uint32_t nv) {
  DustHipSettleResult r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  if (!acc) return r;
  r.columns = nu * nv;
  r.loose = acc[0]; r.fixed = acc[1]; r.moved = acc[2]; r.changed = acc[3]; r.fall_sum = acc[4]; r.changed_columns = acc[5];
  r.fall_max = acc[kSettleFallMax];
  for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - acc[kSettleLo + k]); r.hi[k] = uint8_t(acc[kSettleHi + k]); }
  return r;
}
// What an apply's caller gets from the device's array of 1 + 2 * generations records (kSettleAccWords each: the initial fall, then the
// slide and the fall of every generation; a step that never ran left its record 0); null: nothing was looked at -- the zero record.
// per_generation (may be null): 2 * generations words, slid and fell per generation.
inline DustHipSettleApplied settle_applied(const uint32_t* slots, uint32_t generations, uint32_t* per_generation) {
  DustHipSettleApplied r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  if (per_generation) std::fill(per_generation, per_generation + size_t(generations) * 2, 0u);
  if (!slots) return r;
  uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  r.first_moved = slots[2];
  r.loose = slots[0];
  r.fall_sum = slots[4];
  settle_fold_bounds(slots, lo, hi);
  for (uint32_t g = 0; g < generations; ++g) {
    const uint32_t* slide = slots + size_t(1u + 2u * g) * kSettleAccWords;
    const uint32_t* fall = slide + kSettleAccWords;
    const uint32_t slid = slide[kSettleSlid], fell = fall[2];
    if (slid + fell == 0u) continue;
    r.generations = g + 1u;
    r.slid += slid; r.fell += fell; r.fall_sum += fall[4];
    settle_fold_bounds(slide, lo, hi);
    settle_fold_bounds(fall, lo, hi);
    if (per_generation) { per_generation[2 * g] = slid; per_generation[2 * g + 1] = fell; }
  }
  for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - lo[k]); r.hi[k] = uint8_t(hi[k]); }
  return r;
}
// Whether the first `ran` generations of an apply's records end in four that moved nothing: the model is at rest then -- the four
// covered every direction -- and no later generation would move anything
inline bool settle_at_rest(const uint32_t* slots, uint32_t ran) {
  uint32_t still = 0;
  for (uint32_t g = 0; g < ran; ++g) {
    const uint32_t* slide = slots + size_t(1u + 2u * g) * kSettleAccWords;
    still = slide[kSettleSlid] + slide[kSettleAccWords + 2] == 0u ? still + 1u : 0u;
    if (still == 4u) return true;
  }
  return false;
}

// ---- model voxelisation (dust_hip_model_edit_triangles, _fill_mesh)
// an edit operation as the two grid bytes it writes (device_shape's table)
inline void edit_op_bytes(uint32_t op, int32_t palette, uint32_t& solid_to, uint32_t& empty_to) {
  const uint32_t byte = uint32_t(palette) + 1u;
  switch (op) {
    case DUST_HIP_EDIT_CARVE: solid_to = 0; empty_to = 0; break;
    case DUST_HIP_EDIT_FILL: solid_to = byte; empty_to = byte; break;
    case DUST_HIP_EDIT_PAINT: solid_to = byte; empty_to = 0; break;
    default: solid_to = kEditKeep; empty_to = byte; break;  // PLACE
  }
}
// floor(v / 256) for any sign
inline int32_t triangle_floor_voxel(int32_t v) { return v >= 0 ? v / kTriangleUnit : -((-v + kTriangleUnit - 1) / kTriangleUnit); }

// A triangle of dust_hip_model_edit_triangles: the range check, n == 0, and the inclusive bounds of the voxels its vertices' extent
// touches -- a coordinate at exactly 256 k touches voxels k - 1 and k -- clipped to the tree. false: it covers nothing (out of range,
// zero normal, wholly outside the tree). They cull; the 13-axis test decides.
inline bool device_triangle(const DustHipTriangle& s, DevTriangle& d) {
  if (!triangle_in_range(s.v)) return false;
  const TriangleSetup t = triangle_setup(s.v);
  if (triangle_degenerate(t)) return false;
  uint32_t vlo[3], vhi[3];
  for (int r = 0; r < 3; ++r) {
    const int32_t l = triangle_floor_voxel(t.lo[r] - 1), h = triangle_floor_voxel(t.hi[r]);
    if (l > 255 || h < 0) return false;
    vlo[r] = l < 0 ? 0u : uint32_t(l);
    vhi[r] = h > 255 ? 255u : uint32_t(h);
  }
  std::memcpy(d.v, s.v, sizeof(d.v));
  edit_op_bytes(s.op, s.palette, d.solid_to, d.empty_to);
  d.lo = vlo[0] | (vlo[1] << 8) | (vlo[2] << 16);
  d.hi = vhi[0] | (vhi[1] << 8) | (vhi[2] << 16);
  return true;
}

// A triangle of dust_hip_model_fill_mesh. `live`: in range and not degenerate; `crossing`: live with n.z != 0. true: it is crossing and
// some column centre (256 x + 128, 256 y + 128) of the region lo..hi lies in its vertices' extent -- d.lo / d.hi are those columns with
// z = 0 (the tiles k_fill_columns is launched for), the operation bytes 0. Its height is not looked at: a triangle above or below the
// tree still toggles the centres below it.
inline bool device_fill_triangle(const DustHipTriangle& s, const uint32_t* lo, const uint32_t* hi, DevTriangle& d, bool& live, bool& crossing) {
  live = crossing = false;
  if (!triangle_in_range(s.v)) return false;
  const TriangleColumn t = triangle_column(s.v);
  if (triangle_degenerate(t)) return false;
  live = true;
  if (t.s == 0) return false;
  crossing = true;
  uint32_t clo[2], chi[2];
  for (int r = 0; r < 2; ++r) {
    const int32_t least = std::min({s.v[0][r], s.v[1][r], s.v[2][r]}), most = std::max({s.v[0][r], s.v[1][r], s.v[2][r]});
    const int32_t l = triangle_floor_voxel(least - kTriangleUnit / 2 - 1) + 1, h = triangle_floor_voxel(most - kTriangleUnit / 2);  // ceil, floor
    const int32_t first = std::max(l, int32_t(lo[r])), last = std::min(h, int32_t(hi[r]));
    if (first > last) return false;
    clo[r] = uint32_t(first); chi[r] = uint32_t(last);
  }
  std::memcpy(d.v, s.v, sizeof(d.v));
  d.solid_to = d.empty_to = 0;
  d.lo = clo[0] | (clo[1] << 8);
  d.hi = chi[0] | (chi[1] << 8);
  return true;
}

// A fill_mesh query as k_fill_apply reads it: the operation's two bytes, the region clipped to the tree as device_columns clips it (a
// coordinate past 255 is cut back to it; lo past hi is the empty region) and the root cells it reaches. The pointers are the caller's.
// nullptr: the query is fine; otherwise why the call refuses it, in the header's order. `empty`: nothing is looked at, no launch is made
// and the region fields are not set.
inline const char* device_fill_mesh(const DustHipFillMeshQuery& q, FillApplyArgs& d, bool& empty) {
  if (q.op > DUST_HIP_EDIT_PLACE) return "unknown edit op";
  if (q.op != DUST_HIP_EDIT_CARVE && (q.palette < 0 || q.palette > 254)) return "palette index must be 0..254";
  if (q.flags != 0u) return "unknown fill_mesh flag";
  if (q.reserved[0] != 0u || q.reserved[1] != 0u) return "reserved word not 0";
  edit_op_bytes(q.op, q.palette, d.solid_to, d.empty_to);
  uint32_t lo[3], hi[3];
  empty = false;
  for (int r = 0; r < 3; ++r) {
    lo[r] = q.lo[r]; hi[r] = std::min(q.hi[r], 255u);
    empty |= lo[r] > hi[r];
  }
  if (empty) return nullptr;
  for (int r = 0; r < 3; ++r) {
    d.lo[r] = lo[r]; d.hi[r] = hi[r];
    d.box.lo[r] = lo[r] >> 4; d.box.hi[r] = hi[r] >> 4;
  }
  return nullptr;
}
// What a fill_mesh call's caller gets from the device's kFillAccWords accumulator and the host's triangle counts; null: nothing was
// looked at -- the zero result, bounds 255 / 0 (what a region without a covered voxel has too, beside its counts).
inline DustHipFillMeshResult fill_mesh_result(const uint32_t* acc, uint32_t live, uint32_t crossing) {
  DustHipFillMeshResult r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  if (!acc) return r;
  r.covered = acc[0]; r.changed = acc[1];
  r.live = live; r.crossing = crossing;
  for (int k = 0; k < 3; ++k) { r.lo[k] = 255u - acc[2 + k]; r.hi[k] = acc[5 + k]; }
  return r;
}

// A fracture query as k_fracture_label reads it (dust_hip_model_fracture): the filter's grid byte, the limit, the scales, the region
// clipped to the tree as device_columns clips it and the root cells it reaches. The pointers, the seeds and `cull` are the caller's.
// nullptr: the query is fine; otherwise why the call refuses it, in the header's order. `empty` as in device_surface: nothing is looked
// at, no launch is made and the region fields are not set.
inline const char* device_fracture(const DustHipFractureQuery& q, FractureArgs& d, bool& empty) {
  for (int r = 0; r < 3; ++r)
    if (q.scale[r] == 0u || q.scale[r] > kFractureMaxScale) return "scale must be 1..16 on every axis";
  if (q.palette < -1 || q.palette > 254) return "palette must be -1 (every solid voxel) or 0..254";
  if (q.flags != 0u) return "unknown fracture flag";
  if (q.reserved0 != 0u || q.reserved != 0u) return "reserved word not 0";
  d.byte = q.palette < 0 ? 0u : uint32_t(q.palette) + 1u;
  d.limit = q.max_distance2;
  empty = false;
  for (int r = 0; r < 3; ++r) {
    d.scale[r] = q.scale[r];
    const uint32_t lo = q.lo[r], hi = std::min(q.hi[r], 255u);
    empty |= lo > hi;
    if (empty) continue;
    d.lo[r] = lo; d.hi[r] = hi;
    d.box.lo[r] = lo >> 4; d.box.hi[r] = hi >> 4;
  }
  return nullptr;
}
// what dust_hip_model_fracture refuses in its seeds
inline const char* fracture_seeds(const DustHipFractureSeed* seeds, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    const int32_t c[3] = {seeds[i].x, seeds[i].y, seeds[i].z};
    for (int32_t v : c)
      if (v < kFractureSeedMin || v > kFractureSeedMax) return "seed coordinate outside -1024..1279";
    if (seeds[i].reserved != 0u) return "a seed's reserved word is not 0";
  }
  return nullptr;
}
// what dust_hip_model_fracture_apply refuses
inline const char* fracture_apply_arguments(uint32_t where, int32_t value) {
  if (where > DUST_HIP_FRACTURE_LABELLED) return "where must be DUST_HIP_FRACTURE_SEAMS or DUST_HIP_FRACTURE_LABELLED";
  if (value < -1 || value > 254) return "value must be -1 (None) or a palette index 0..254";
  return nullptr;
}
// A detach's selection: a bit per named cell. nullptr, or why the call refuses (an index that is no cell of the labelling).
inline const char* fracture_selection(const uint32_t* cells, uint32_t n, uint32_t n_seeds, uint64_t (&selected)[kFractureSelectWords]) {
  std::memset(selected, 0, sizeof(selected));
  for (uint32_t i = 0; i < n; ++i) {
    if (cells[i] >= n_seeds) return "a cell index is not below the labelling's n_seeds";
    selected[cells[i] >> 6] |= 1ull << (cells[i] & 63u);
  }
  return nullptr;
}
// What a fracture's caller gets from the device's kFractureAccWords accumulator; null: nothing was looked at -- the zero result with
// no largest cell and bounds 255 / 0 (what a call that labels nothing has too, beside its `solid`).
inline DustHipFractureResult fracture_result(const uint32_t* acc) {
  DustHipFractureResult r{};
  for (int k = 0; k < 3; ++k) r.lo[k] = 255;
  r.largest_cell = 0xFFFFFFFFu;
  if (!acc) return r;
  r.solid = acc[kFractureSolid]; r.labelled = acc[kFractureLabelled]; r.cut_faces = acc[kFractureCut];
  r.cells = acc[kFractureCells];
  if (r.labelled != 0u) {
    r.max_d2 = acc[kFractureMaxD2];
    for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - acc[kFractureLo + k]); r.hi[k] = uint8_t(acc[kFractureHi + k]); }
  }
  if (r.cells != 0u) {
    r.largest_cell = 0xFFFFFFFFu - acc[kFractureLargest];
    r.largest_voxels = acc[kFractureLargest + 1];
  }
  return r;
}
// the record of a cell without a voxel (what every cell of a call that labels nothing gets)
inline DustHipFractureCell fracture_empty_cell() {
  DustHipFractureCell c{};
  for (int k = 0; k < 3; ++k) c.lo[k] = 255;
  return c;
}

// ---- model resampling (dust_hip_model_resample)
// what the call refuses in a record; nullptr: fine. Two steps, because the header puts the flags between them: the op ...
inline const char* resample_op_refusal(const DustHipResample& s) { return s.op > DUST_HIP_STAMP_PAINT ? "unknown stamp op" : nullptr; }
// ... and the map's limits
inline const char* resample_map_refusal(const DustHipResample& s) {
  for (int k = 0; k < 3; ++k) {
    for (int r = 0; r < 3; ++r)
      if (s.m[k][r] > kResampleMaxM || s.m[k][r] < -kResampleMaxM) return "a matrix entry beyond 8 * DUST_HIP_RESAMPLE_ONE in magnitude";
    if (s.t[k] > kResampleMaxT || s.t[k] < -kResampleMaxT) return "a translation beyond 2^28 in magnitude";
  }
  return nullptr;
}
// The destination box clipped to the tree, the map in the rule's form, the sub-box, the stamp's table. false: the record covers nothing --
// an empty box of either kind, a box wholly outside the tree, or one the interval test rules out as a whole.
inline bool device_resample(const DustHipResample& s, DevResample& d) {
  int32_t lo[3], hi[3], sl[3], sh[3];
  for (int k = 0; k < 3; ++k) {
    if (s.src_lo[k] > s.src_hi[k]) return false;
    lo[k] = std::max<int32_t>(s.dst_lo[k], 0); hi[k] = std::min<int32_t>(s.dst_hi[k], 255);
    if (lo[k] > hi[k]) return false;
    sl[k] = s.src_lo[k]; sh[k] = s.src_hi[k];
    for (int r = 0; r < 3; ++r) d.map.m[k][r] = s.m[k][r];
    d.map.t2[k] = 2 * s.t[k];
  }
  if (!resample_box_meets(d.map, lo, hi, sl, sh)) return false;
  d.lo = uint32_t(lo[0]) | (uint32_t(lo[1]) << 8) | (uint32_t(lo[2]) << 16);
  d.hi = uint32_t(hi[0]) | (uint32_t(hi[1]) << 8) | (uint32_t(hi[2]) << 16);
  d.src_lo = uint32_t(sl[0]) | (uint32_t(sl[1]) << 8) | (uint32_t(sl[2]) << 16);
  d.src_hi = uint32_t(sh[0]) | (uint32_t(sh[1]) << 8) | (uint32_t(sh[2]) << 16);
  d.table = stamp_table(s.op);
  d.pad = 0;
  return true;
}
// whether root cell `cell` (x << 8 | y << 4 | z), clipped to the record's box, can hold a voxel of its image: the interval test
inline bool resample_cell_meets(const DevResample& d, uint32_t cell) {
  const int32_t c[3] = {int32_t(cell >> 8) * 16, int32_t((cell >> 4) & 15u) * 16, int32_t(cell & 15u) * 16};
  int32_t lo[3], hi[3], sl[3], sh[3];
  for (int r = 0; r < 3; ++r) {
    lo[r] = std::max(c[r], int32_t((d.lo >> (8 * r)) & 255u)); hi[r] = std::min(c[r] + 15, int32_t((d.hi >> (8 * r)) & 255u));
    if (lo[r] > hi[r]) return false;
    sl[r] = int32_t((d.src_lo >> (8 * r)) & 255u); sh[r] = int32_t((d.src_hi >> (8 * r)) & 255u);
  }
  return resample_box_meets(d.map, lo, hi, sl, sh);
}
// what a resample's caller gets from a record's `changed` and its kResampleExtra further counts; null: it covers nothing
inline DustHipResampleCount resample_count(uint32_t changed, const uint32_t* extra) {
  DustHipResampleCount c{};
  if (!extra) return c;
  c.changed = changed; c.covered = extra[0]; c.solid = extra[1]; c.blocked = extra[2];
  return c;
}

// the records of a call that cover something, in call order: `index` maps them back to the caller's
template <auto Convert, class In, class Rec>  // (the conversion as a template argument: called directly, as it was before this header)
void live_records(const In* in, uint32_t n, std::vector<Rec>& dev, std::vector<uint32_t>& index) {
  dev.reserve(n); index.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    Rec d{};
    if (Convert(in[i], d)) { dev.push_back(d); index.push_back(i); }
  }
}

// ---- root cells (16^3 voxels, x << 8 | y << 4 | z) that a record's packed inclusive voxel bounds (lo, hi: x | y << 8 | z << 16) reach
inline size_t root_cell_count(uint32_t lo, uint32_t hi) {
  size_t n = 1;
  for (int r = 0; r < 3; ++r) n *= size_t((((hi >> (8 * r)) & 255u) >> 4) - (((lo >> (8 * r)) & 255u) >> 4) + 1u);
  return n;
}
template <class F>
inline __attribute__((always_inline)) void for_each_root_cell(uint32_t lo, uint32_t hi, F&& f) {  // x slowest
  for (uint32_t x = (lo & 255u) >> 4; x <= (hi & 255u) >> 4; ++x)
    for (uint32_t y = ((lo >> 8) & 255u) >> 4; y <= ((hi >> 8) & 255u) >> 4; ++y)
      for (uint32_t z = ((lo >> 16) & 255u) >> 4; z <= ((hi >> 16) & 255u) >> 4; ++z) f((x << 8) | (y << 4) | z);
}

// the root cells a record is listed in: those its bounds reach -- for a resample, those of them the interval test cannot rule out
template <class Rec, class F>
inline __attribute__((always_inline)) void for_each_record_cell(const Rec& r, F&& f) { for_each_root_cell(r.lo, r.hi, f); }
template <class F>
inline __attribute__((always_inline)) void for_each_record_cell(const DevResample& r, F&& f) {
  for_each_root_cell(r.lo, r.hi, [&](uint32_t cell) { if (resample_cell_meets(r, cell)) f(cell); });
}

// where the order-preserving chunk that begins at record c0 ends: before its root cells would pass max_entries (a single record is
// never cut) or its records max_records
template <class Rec>
size_t chunk_end(const std::vector<Rec>& dev, size_t c0, size_t max_entries, size_t max_records) {
  size_t c1 = c0, total = 0;
  while (c1 < dev.size() && c1 - c0 < max_records && (c1 == c0 || total + root_cell_count(dev[c1].lo, dev[c1].hi) <= max_entries)) {
    total += root_cell_count(dev[c1].lo, dev[c1].hi);
    ++c1;
  }
  return c1;
}

// a chunk of shapes or stamps on the host: the non-empty cells, and per cell an ascending list of u16 record ids (relative to c0) in CSR form
struct CellLists {
  std::vector<uint32_t> cells, starts, fill = std::vector<uint32_t>(4096);
  std::vector<uint16_t> ids;
  template <class Rec>
  void bin(const std::vector<Rec>& dev, size_t c0, size_t c1) {
    std::fill(fill.begin(), fill.end(), 0u);
    for (size_t i = c0; i < c1; ++i) for_each_record_cell(dev[i], [&](uint32_t cell) { ++fill[cell]; });
    cells.clear(); starts.clear();
    uint32_t run = 0;
    for (uint32_t cell = 0; cell < 4096; ++cell) {
      const uint32_t k = fill[cell];
      fill[cell] = run;  // where the cell's next id goes
      if (k) { cells.push_back(cell); starts.push_back(run); run += k; }
    }
    starts.push_back(run);
    ids.resize(run);
    for (size_t i = c0; i < c1; ++i) for_each_record_cell(dev[i], [&](uint32_t cell) { ids[fill[cell]++] = uint16_t(i - c0); });
  }
};

// a chunk of casts: one work item per cast (relative to c0) and source root cell its sub-box reaches, in cast order
inline void cast_items(const std::vector<DevCast>& dev, size_t c0, size_t c1, std::vector<CastItem>& items) {
  items.clear();
  for (size_t i = c0; i < c1; ++i) for_each_root_cell(dev[i].lo, dev[i].hi, [&](uint32_t cell) { items.push_back({uint32_t(i - c0), cell}); });
}

}  // namespace dust
