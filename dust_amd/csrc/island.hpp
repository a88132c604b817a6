// island.hpp -- interface between the host runtime (capi_model.cpp) and the connected-component labelling of an editable model (island.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dust {

constexpr uint32_t kIslandKeys = 1u << 24;          // voxels of a 256^3 model: a key is x << 16 | y << 8 | z
constexpr uint32_t kIslandRows = kIslandKeys / 64;  // runs of 64 consecutive keys: one x, one y, a quarter of the z axis
constexpr uint32_t kNoIsland = 0xFFFFFFFFu;         // label of an empty voxel (DUST_HIP_NO_ISLAND)

// One island while its record is being accumulated: zero-initialised, so the lower bounds are kept as 255 - lo (atomicMax).
struct IslandAcc {  // 64 bytes
  uint32_t key, voxels;
  uint32_t inv_lo[3], hi[3];
  uint32_t flags, pad;
  unsigned long long sum[3];
};
struct DevIsland {  // DustHipIsland, 40 bytes
  uint32_t key, voxels;
  uint32_t lo_flags, hi_reserved;  // lo[0] | lo[1] << 8 | lo[2] << 16 | flags << 24; hi the same with reserved = 0
  uint32_t sum[6];                 // three little-endian uint64
};
static_assert(sizeof(IslandAcc) == 64 && sizeof(DevIsland) == 40, "island records");

struct IslandArgs {
  const uint8_t* grid;     // EditArgs::grid (brick-major)
  uint32_t* label;         // kIslandKeys, indexed by KEY: the voxel's parent in the union-find forest, a smaller key of the same island
                           // (itself at the root); after the flatten pass the island's key; kNoIsland where the voxel is empty
  uint64_t* root_mask;     // kIslandRows: bit b of word r set when key r * 64 + b names an island
  uint32_t* root_count;    // kIslandRows (+ scan): islands per row -> an island's rank in key order
  uint32_t* scan_tmp;      // 256 block sums, then [256] = the number of islands
  IslandAcc* acc;          // `capacity` accumulators, zeroed by the caller
  DevIsland* records;      // `capacity` records
  uint32_t capacity;       // records wanted: min(islands, the caller's capacity)
  uint32_t corners;        // 26-connectivity (0: 6-connectivity)
  uint32_t anchor_lo[3], anchor_hi[3];  // inclusive, clipped to the tree; lo > hi on an axis: nothing is anchored
};

struct IslandDetachArgs {
  uint8_t* src;              // the source model's grid
  uint8_t* dst;              // the new model's grid (every byte is written), or null
  uint32_t* label;
  const uint64_t* selected;  // kIslandRows: bit set for every key being detached
  uint32_t carve;            // remove the voxels from the source (and from its labelling)
};

// label the grid, count the islands: afterwards scan_tmp[256] holds their number (read it back), label / root_mask / root_count are final.
// `relabel` false: a.label already holds a flat labelling of this grid under a.corners (islands may have been detached since); only the
// roots are found and counted again, since root_mask / root_count / scan_tmp are shared by the context's models
hipError_t launch_island_label(const IslandArgs& a, bool relabel, hipStream_t s);
// the first a.capacity records in key order (a.acc zeroed by the caller)
hipError_t launch_island_records(const IslandArgs& a, hipStream_t s);
// (dust_hip_model_island_of: the lookup of field.hpp, by key)
// selected (zeroed by the caller) gets a bit per key that names an island; *bad counts the keys that do not (zeroed by the caller)
hipError_t launch_island_select(const uint32_t* label, const uint32_t* keys, uint32_t n, uint64_t* selected, uint32_t* bad, hipStream_t s);
hipError_t launch_island_detach(const IslandDetachArgs& a, hipStream_t s);

}  // namespace dust
