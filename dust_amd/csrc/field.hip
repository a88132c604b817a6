// field.hip -- lookups in, and grid writes driven by, the per-voxel arrays of an editable model (field.hpp): dust_hip_model_flood_at,
// _distance_at, _island_of, _flood_apply, _distance_apply.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "field.hpp"

namespace dust {

// a thread per coordinate; kByKey: `values` is indexed by the public key (the island labels), otherwise brick-major
template <class T, bool kByKey>
__global__ void __launch_bounds__(256) k_lookup(const T* values, const uint32_t* xyz, T* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];  // (the host has checked the coordinates)
  out[i] = values[kByKey ? Voxel{x, y, z}.key() : voxel_index(x, y, z)];
}

// a workgroup per root cell of the box, a wave per 16 bricks
__global__ void __launch_bounds__(256) k_field_apply(FieldApplyArgs a) {
  const uint32_t cell = a.box.cell(blockIdx.x);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t n = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    const size_t at = ((size_t)cell * 64u + wave * 16u + k) * 64u + lane;
    const uint32_t v = a.field[at];
    const bool differs = v != kFieldNone && v >= a.lo && v <= a.hi && a.grid[at] != a.byte;
    if (differs) a.grid[at] = (uint8_t)a.byte;
    n += (uint32_t)__popcll(__ballot(differs));
  }
  if (n && lane == 0u) atomicAdd(a.changed, n);
}

hipError_t launch_lookup(const uint16_t* field, const uint32_t* xyz, uint16_t* out, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL((k_lookup<uint16_t, false>), dim3((n + 255u) / 256u), dim3(256), 0, s, field, xyz, out, n);
  return hipGetLastError();
}
hipError_t launch_lookup(const uint32_t* label, const uint32_t* xyz, uint32_t* out, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL((k_lookup<uint32_t, true>), dim3((n + 255u) / 256u), dim3(256), 0, s, label, xyz, out, n);
  return hipGetLastError();
}
hipError_t launch_field_apply(const FieldApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_field_apply, dim3(a.box.count()), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
