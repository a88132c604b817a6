// query.hpp -- the launch of the scene ray queries (query.hip), as the host runtime (capi_scene.cpp) calls it
#pragma once
#include <hip/hip_runtime.h>

#include "dust_dev.h"

namespace dust {

struct QueryArgs {  // the kernel's second argument, behind the launch descriptor (whose scene half the host fills as for a frame)
  const float* rays;               // n DustHipRay records (8 words each; 16-byte aligned)
  uint32_t* hits;                  // n DustHipRayHit records
  uint32_t n, any_hit;
  unsigned long long* counter;     // rays handed out so far (zero at launch)
  unsigned long long* next_counter;  // the next launch's counter: zeroed by this one (launches of one stream run one after the other)
};

hipError_t launch_ray_query(const FrameArgs& a, const QueryArgs& q, uint32_t grid, uint32_t block, hipStream_t s);
hipError_t configure_query_kernels(size_t max_lds);  // every variant may take the device's dynamic LDS (at context creation)

// scene box queries (overlap.hip, dust_hip_scene_overlap_boxes / _async)
struct OverlapArgs {
  const float* boxes;              // n DustHipBoxQuery records (8 words each; 16-byte aligned)
  uint32_t* counts;                // n counts
  uint32_t* records;               // n_records DustHipVoxelRef records (4 words each; 16-byte aligned)
  uint32_t n, n_records, any_hit, pad;
  unsigned long long* counter;     // queries handed out so far (zero at launch): the ray queries' pair of counters, same protocol
  unsigned long long* next_counter;
};
constexpr uint32_t kOverlapWaves = 4;   // waves per workgroup of k_overlap_boxes (one query per wave at a time)
constexpr uint32_t kOverlapChunk = 4;   // queries a wave takes from the counter at a time
hipError_t launch_overlap_boxes(const FrameArgs& a, const OverlapArgs& q, uint32_t grid, uint32_t block, hipStream_t s);

// scene box sweeps (sweep.hip, dust_hip_scene_sweep_boxes / _async)
struct SweepArgs {
  const float* sweeps;             // n DustHipBoxSweep records (12 words each; 16-byte aligned)
  uint32_t* hits;                  // n DustHipSweepHit records (8 words each; 16-byte aligned)
  uint32_t n, any_hit, ignore_start, pad;
  unsigned long long* counter;     // queries handed out so far (zero at launch): the ray queries' pair of counters, same protocol
  unsigned long long* next_counter;
};
constexpr uint32_t kSweepWaves = 4;   // waves per workgroup of k_sweep_boxes (one query per wave at a time)
constexpr uint32_t kSweepChunk = 4;   // queries a wave takes from the counter at a time
hipError_t launch_sweep_boxes(const FrameArgs& a, const SweepArgs& q, uint32_t grid, uint32_t block, hipStream_t s);

}  // namespace dust
