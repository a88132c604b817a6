// census.hip -- model censuses (dust_hip_model_census): what the voxels inside boxes, spheres and capsules hold, counted on the device
// without changing anything. The read-only sibling of k_edit_shapes (edit.hip) on the skeleton of cell_records.hpp: a workgroup per root
// cell that some shape's bounds reach, four waves of 16 bricks, lane = voxel bit, the bricks loaded once and kept in registers while the
// cell's shape list is walked by a wave-uniform id. Membership is shape_cover.hpp -- the text k_edit_shapes runs, so a census says
// exactly what the CARVE that follows it removes.
//
// Per (wave, shape) everything is reduced inside the wave first: covered and solid are popcounts of ballots (wave-uniform), the
// coordinate sums are u32 per lane (a wave's 1024 voxels times 255 at most) summed across the lanes, the bounds a wave min / max. The
// four waves of the workgroup then put their eleven-word partial records into LDS, meet at ONE barrier per shape (they walk the same
// list, so all of them reach it) and eleven lanes of wave 0 fold the four partials and issue one ordinary vector atomic per field:
// two 32-bit adds, three 64-bit adds, three atomicMin, three atomicMax, and nothing at all for a shape that covers no voxel of the
// cell. (The first form issued them per wave; a whole-tree box then sent 16 384 x 11 atomics to one 64-byte line and took 0.55 ms.)
// All integer: the result does not depend on the order the workgroups arrive in, and two runs give the same bytes.
//
// The per-material tables never see a per-voxel global atomic. The workgroup keeps 256 u32 counters per shape in LDS and the waves fill
// them per brick with one LDS add per DISTINCT grid byte among the covered lanes: the byte of the first remaining lane is read into a
// scalar, a ballot finds its equals, lane 0 adds the popcount. Terrain bricks hold one to three values. After the shape's barrier the
// table is flushed and cleared as one instruction per wave, lane = bin 64 wave + lane, only the non-zero bins active. The table and the
// partials exist twice and take turns from shape to shape (2 KiB + 384 bytes of LDS), so a wave that runs ahead fills the other half.
// (The atomic rates measured for this chip are for float adds of full rows; integer adds of a few scattered bins are unmeasured, which
// is why the design keeps their number small rather than counting on a rate.) A uniform flag skips the tables when none were asked for.
// No fences, spins or waits BETWEEN workgroups.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cell_records.hpp"
#include "census.hpp"
#include "shape_cover.hpp"

namespace dust {

namespace {
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = umin(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = umax(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
constexpr uint32_t kCensusFields = 11;  // a partial record: covered, solid, sum[3], lo[3], hi[3]
}  // namespace

__global__ void __launch_bounds__(256) k_census_init(CensusAcc* acc, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  CensusAcc z{};
  z.lo[0] = z.lo[1] = z.lo[2] = 255u;
  acc[i] = z;
}

__global__ void __launch_bounds__(256) k_census(CensusArgs a) {
  __shared__ uint32_t table[2][kCensusBins];  // the workgroup's counters for the shape being walked and for the one before it
  __shared__ uint32_t part[2][4][kCensusFields];
  const bool tables = a.tables != nullptr;  // uniform: a kernel argument
  const uint32_t wave = uniform(threadIdx.x >> 6);
  if (tables) table[0][threadIdx.x] = table[1][threadIdx.x] = 0u;  // (256 threads, 256 bins)
  __syncthreads();
  uint32_t turn = 0;  // which half of `table` and `part` this shape uses: the halves take turns, so one barrier per shape is enough
  read_cell_records(a, [&](const CellBricks& c, uint32_t id) {
    const DevEditShape s = a.shapes[id];
    const uint32_t lo_x = (s.lo & 255u) >> 2, lo_y = ((s.lo >> 8) & 255u) >> 2, lo_z = (s.lo >> 16) >> 2;
    const uint32_t hi_x = (s.hi & 255u) >> 2, hi_y = ((s.hi >> 8) & 255u) >> 2, hi_z = (s.hi >> 16) >> 2;
    uint32_t reach = 0;  // bit k: the shape's bounds reach brick k of this wave (uniform)
    if (c.bx >= lo_x && c.bx <= hi_x) {
#pragma unroll
      for (uint32_t q = 0; q < 4u; ++q) {
        if (c.by0 + q >= lo_y && c.by0 + q <= hi_y) reach |= 0xFu << (4u * q);
      }
#pragma unroll
      for (uint32_t q = 0; q < 4u; ++q) {
        if (c.bz0 + q < lo_z || c.bz0 + q > hi_z) reach &= ~(0x1111u << q);
      }
    }
    uint32_t* bins = table[turn];
    // voxel centres: small integers + 0.5, exact in float32
    const Voxel p = brick_voxel(c.bx, c.by0, c.bz0, c.lane);
    uint32_t covered = 0, solid = 0;                                                  // of the wave (uniform)
    uint32_t mine = 0, sy = 0, sz = 0, y_lo = 255u, y_hi = 0, z_lo = 255u, z_hi = 0;  // of this lane's solid covered voxels (x is p.x in all)
    if (reach != 0u) {
      const float cx = (float)p.x + 0.5f, cy0 = (float)p.y + 0.5f, cz0 = (float)p.z + 0.5f;
      const ShapeCover cover = shape_cover(s.a, s.b, s.kind, s.radius);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if (!((reach >> k) & 1u)) continue;
        const float cy = cy0 + (float)((k >> 2) * 4), cz = cz0 + (float)((k & 3) * 4);  // exact
        const bool in = shape_covers(cover, cx, cy, cz);
        const uint64_t m = __ballot(in);
        if (m == 0ull) continue;
        const uint32_t g = c.v[k];
        const bool hit = in && g != 0u;
        covered += (uint32_t)__popcll(m);
        solid += (uint32_t)__popcll(__ballot(hit));
        if (hit) {
          const uint32_t y = p.y + (uint32_t)((k >> 2) * 4), z = p.z + (uint32_t)((k & 3) * 4);
          mine += 1u; sy += y; sz += z;
          y_lo = umin(y_lo, y); y_hi = umax(y_hi, y); z_lo = umin(z_lo, z); z_hi = umax(z_hi, z);
        }
        if (tables) {  // one LDS add per distinct byte among the covered lanes
          for (uint64_t rest = m; rest != 0ull;) {
            const uint32_t byte = (uint32_t)__builtin_amdgcn_readlane((int)g, (int)__builtin_ctzll(rest));
            const uint64_t same = __ballot(in && g == byte);
            if (c.lane == 0u) atomicAdd(&bins[byte & (kCensusBins - 1u)], (uint32_t)__popcll(same));
            rest &= ~same;
          }
        }
      }
    }
    // the wave's partial record (covered, solid, three sums, three lower and three upper bounds), written by one lane
    uint32_t sum_x = 0, sum_y = 0, sum_z = 0, x_lo = 255u, x_hi = 0;
    if (solid != 0u) {  // (uniform)
      sum_x = wave_sum(mine * p.x); sum_y = wave_sum(sy); sum_z = wave_sum(sz);
      x_lo = wave_umin(mine ? p.x : 255u); x_hi = wave_umax(mine ? p.x : 0u);
      y_lo = wave_umin(y_lo); y_hi = wave_umax(y_hi); z_lo = wave_umin(z_lo); z_hi = wave_umax(z_hi);
    }
    if (c.lane == 0u) {
      uint32_t* mine_part = part[turn][wave];
      mine_part[0] = covered; mine_part[1] = solid;
      mine_part[2] = sum_x; mine_part[3] = sum_y; mine_part[4] = sum_z;
      mine_part[5] = x_lo; mine_part[6] = y_lo; mine_part[7] = z_lo;
      mine_part[8] = x_hi; mine_part[9] = y_hi; mine_part[10] = z_hi;
    }
    __syncthreads();  // every wave of the workgroup walks the same list: the barrier is reached by all of them, once per shape
    if (wave == 0u && c.lane < kCensusFields) {  // the four partials into one, and one atomic per field
      const uint32_t f = c.lane;
      const uint32_t p0 = part[turn][0][f], p1 = part[turn][1][f], p2 = part[turn][2][f], p3 = part[turn][3][f];
      const uint32_t any = part[turn][0][f < 2u ? 0u : 1u] | part[turn][1][f < 2u ? 0u : 1u] | part[turn][2][f < 2u ? 0u : 1u] | part[turn][3][f < 2u ? 0u : 1u];
      if (any != 0u) {  // the counts where something is covered, the rest where something covered is solid
        CensusAcc* acc = a.acc + id;
        if (f < 2u) atomicAdd(f == 0u ? &acc->covered : &acc->solid, p0 + p1 + p2 + p3);
        else if (f < 5u) atomicAdd(reinterpret_cast<unsigned long long*>(&acc->sum[f - 2u]), (unsigned long long)(p0 + p1 + p2 + p3));
        else if (f < 8u) atomicMin(&acc->lo[f - 5u], umin(umin(p0, p1), umin(p2, p3)));
        else atomicMax(&acc->hi[f - 8u], umax(umax(p0, p1), umax(p2, p3)));
      }
    }
    if (tables) {  // flush and clear: this wave's quarter of the bins, the non-zero ones only
      const uint32_t bin = 64u * wave + c.lane, n = bins[bin];
      if (n != 0u) {
        atomicAdd(&a.tables[(size_t)id * kCensusBins + bin], n);
        bins[bin] = 0u;
      }
    }
    turn ^= 1u;
  });
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_census_init(CensusAcc* acc, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_census_init, dim3((n + 255u) / 256u), dim3(256), 0, s, acc, n);
  return hipGetLastError();
}
hipError_t launch_census(const CensusArgs& a, hipStream_t s) {
  if (a.n_cells) hipLaunchKernelGGL(k_census, dim3(a.n_cells), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
