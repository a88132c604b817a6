// scan.hpp -- the one workgroup prefix sum, and the exclusive scan of kLattice-entry tables built on it (kernels in edit.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dust {

// Exclusive scans of one or two tables of kLattice (262 144) counters, in place and in two parts: afterwards entry i holds the sum of the
// entries before it inside its 1024-entry block, tmp[256 * t + (i >> 10)] the sum of table t's blocks before that one (a reader adds
// the two), and *total[t] table t's sum.
struct TableScan {
  uint32_t* table[2];
  uint32_t* total[2];
  uint32_t* tmp;  // 256 words per table
};
hipError_t launch_table_scan(const TableScan& t, uint32_t n_tables, hipStream_t s);

#ifdef __HIPCC__
// inclusive prefix sum of v over the N threads of the workgroup (Hillis-Steele in N words of LDS); lds[N - 1] is the total
template <uint32_t N>
__device__ __forceinline__ uint32_t block_scan_inclusive(uint32_t* lds, uint32_t v) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t d = 1; d < N; d <<= 1) {
    const uint32_t x = threadIdx.x >= d ? lds[threadIdx.x - d] : 0u;
    __syncthreads();
    lds[threadIdx.x] += x;
    __syncthreads();
  }
  return lds[threadIdx.x];
}
#endif

}  // namespace dust
