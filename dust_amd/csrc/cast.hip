// cast.hip -- dust_hip_model_cast: how many integer steps a piece of one model moves inside another before a voxel of it is blocked.
//
// Only solidity matters, so both kernels read the two models' brick masks (EditArgs::brick_mask, 2 MiB each) and never a grid byte.
// One workgroup per (cast, source root cell the sub-box reaches), listed by the host. Lane l of every wave loads the mask of the cell's
// brick l (one coalesced 512-byte load) and clips it to the sub-box; the ballot of non-empty bricks is the wave's work list, wave w
// taking the x slice of bricks 16 w .. 16 w + 15 as k_stamp does. Per brick the mask is broadcast (v_readlane) and lane = voxel bit.
//
// k_cast_walk: the range of placements a brick can touch anything in is closed-form and wave-uniform -- per axis the interval in
// which its 4^3 image meets the tree, cut to the record's k_lo..k_hi; under WALLS the walk begins at 0 and ends one past the last
// placement the brick is inside, where leaving the tree blocks it. Inside that range the wave walks k upward, four placements per
// round (four independent loads in flight): a lane whose voxel stands inside the tree loads the destination brick mask under it
// (at most 8 distinct words per wave-instruction) and tests one bit; outside the tree it is blocked exactly when WALLS is set. The
// first k at which any lane is blocked ends the brick's walk: a voxel is blocked at the cast's answer k* exactly when its own first
// blocked placement is k*, so min over voxels of (k << 24 | source key) gives k* and the smallest key at once. Lanes keep their own
// value, the wave reduces it with cross-lane moves and issues one 64-bit atomicMin into best[cast]. A relaxed read of best[cast]
// lowers the walk's upper end between rounds: a value there is some voxel's true first blocked placement, never below k*, and the
// walk still includes it, so it only prunes (the minimum is the same whatever the order the waves arrive in).
// k_cast_count: after the walk, placement k* alone is tested again; the ballots' popcounts give `contacts`, the masks' popcounts
// `voxels`, and a blocked voxel outside the tree sets the wall flag -- integer adds and an OR: order-independent.
// Every loop is bounded by the record: at most 16 bricks per wave and kCastMaxWalk placements per brick. No workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cast.hpp"
#include "edit.hpp"

namespace dust {

namespace {

__device__ __forceinline__ int32_t pick(int32_t x, int32_t y, int32_t z, uint32_t axis) { return axis == 0u ? x : axis == 1u ? y : z; }

// what both kernels know of a cast's source brick: per lane, where its voxel stands at placement 0, whether it belongs to the piece, its key
struct BrickView {
  int32_t d0[3];
  bool solid;
  uint32_t key;
};

struct CastView {
  DevCast c;
  int32_t lo[3], hi[3];  // the sub-box
  uint32_t p[3];
  bool g[3], walls;
  __device__ __forceinline__ explicit CastView(const DevCast& rec) : c(rec) {
    for (int r = 0; r < 3; ++r) {
      lo[r] = (int32_t)((c.lo >> (8 * r)) & 255u);
      hi[r] = (int32_t)((c.hi >> (8 * r)) & 255u);
      p[r] = (c.orient >> (2 * r)) & 3u;
      g[r] = (c.orient >> (6 + r)) & 1u;
    }
    walls = (c.orient & kCastWalls) != 0u;
  }
  // the mask of the cell's brick `lane`, clipped to the sub-box
  __device__ __forceinline__ uint64_t clipped(const uint64_t* src_mask, uint32_t cell, uint32_t lane) const {
    uint32_t bx, by, bz;
    cell_brick(cell, lane, bx, by, bz);
    const int32_t x0 = (int32_t)(bx * 4u), y0 = (int32_t)(by * 4u), z0 = (int32_t)(bz * 4u);  // the brick's first voxel
    uint64_t mx = 0, my = 0, mz = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (x0 + i >= lo[0] && x0 + i <= hi[0]) mx |= 0xFFFFull << (16 * i);
      if (y0 + i >= lo[1] && y0 + i <= hi[1]) my |= 0x000F000F000F000Full << (4 * i);
      if (z0 + i >= lo[2] && z0 + i <= hi[2]) mz |= 0x1111111111111111ull << i;
    }
    return src_mask[(size_t)cell * 64u + lane] & mx & my & mz;  // (cell < 4096: inside the lattice)
  }
  // brick b (0..63, wave-uniform) of the cell, whose mask is bm: this lane's voxel
  __device__ __forceinline__ BrickView brick(uint32_t cell, uint32_t b, uint64_t bm, uint32_t lane, int32_t s0[3]) const {
    uint32_t bx, by, bz;
    cell_brick(cell, b, bx, by, bz);
    const Voxel mine = brick_voxel(bx, by, bz, lane);
    s0[0] = (int32_t)(bx * 4u); s0[1] = (int32_t)(by * 4u); s0[2] = (int32_t)(bz * 4u);
    const int32_t sx = (int32_t)mine.x, sy = (int32_t)mine.y, sz = (int32_t)mine.z;
    BrickView v;
    v.solid = (bm >> lane) & 1ull;
    v.key = mine.key();
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int32_t sp = pick(sx, sy, sz, p[r]), lp = pick(lo[0], lo[1], lo[2], p[r]), hp = pick(hi[0], hi[1], hi[2], p[r]);
      v.d0[r] = c.off[r] + (g[r] ? hp - sp : sp - lp);  // (meaningful for the piece's voxels, the only ones that are used)
    }
    return v;
  }
  // is this lane's voxel blocked at placement k? `outside`: it stands outside the tree there
  __device__ __forceinline__ bool blocked(const BrickView& v, uint32_t k, const uint64_t* dst_mask, bool& outside) const {
    const int32_t dx = v.d0[0] + (int32_t)k * c.step[0], dy = v.d0[1] + (int32_t)k * c.step[1], dz = v.d0[2] + (int32_t)k * c.step[2];
    const bool inside = (uint32_t)(dx | dy | dz) < 256u;  // (a negative coordinate sets the high bits)
    outside = !inside;
    if (!v.solid) return false;
    if (!inside) return walls;
    const uint64_t w = dst_mask[leaf_code((uint32_t)dx >> 2, (uint32_t)dy >> 2, (uint32_t)dz >> 2)];  // (all three < 64: inside the lattice)
    return (w >> voxel_bit((uint32_t)dx, (uint32_t)dy, (uint32_t)dz)) & 1ull;
  }
};

__device__ __forceinline__ uint64_t read_lane(uint64_t v, uint32_t lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane);
  return ((uint64_t)hi << 32) | lo;
}

}  // namespace

__global__ void __launch_bounds__(256) k_cast_walk(CastArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform(threadIdx.x >> 6);
  const CastItem it = a.items[blockIdx.x];
  const CastView cv(a.casts[it.cast]);
  const DevCast& c = cv.c;
  if (c.k_lo > c.k_hi) return;
  const uint64_t m = cv.clipped(a.src_mask, it.cell, lane);
  uint64_t todo = (__ballot(m != 0ull) >> (16u * wave)) & 0xFFFFull;
  unsigned long long* best = a.best + it.cast;
  unsigned long long mine = kCastNoHit;
  uint32_t bound = c.k_hi;  // no placement above it can be the answer
  while (todo) {
    const uint32_t b = uniform(16u * wave + (uint32_t)__builtin_ctzll(todo));
    todo &= todo - 1ull;
    int32_t s0[3];
    const BrickView v = cv.brick(it.cell, b, read_lane(m, b), lane, s0);
    // the placements at which the brick's clipped 4^3 box meets the tree, per destination axis (wave-uniform, small integers)
    int64_t first = INT32_MIN, last = INT32_MAX;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int32_t sb = pick(s0[0], s0[1], s0[2], cv.p[r]), lp = pick(cv.lo[0], cv.lo[1], cv.lo[2], cv.p[r]), hp = pick(cv.hi[0], cv.hi[1], cv.hi[2], cv.p[r]);
      const int32_t smin = sb > lp ? sb : lp, smax = sb + 3 < hp ? sb + 3 : hp;
      const int32_t dmin = c.off[r] + (cv.g[r] ? hp - smax : smin - lp), dmax = c.off[r] + (cv.g[r] ? hp - smin : smax - lp);
      int64_t f, l;
      if (c.step[r] == 0) { const bool meets = dmax >= 0 && dmin <= 255; f = meets ? INT32_MIN : 1; l = meets ? INT32_MAX : 0; }
      else if (c.step[r] > 0) { f = -(int64_t)dmax; l = 255 - (int64_t)dmin; }
      else { f = (int64_t)dmin - 255; l = dmax; }
      first = f > first ? f : first;
      last = l < last ? l : last;
    }
    int64_t ka, kb;
    if (cv.walls) {  // from placement 0 until the brick has left the tree (or placement 0 alone when it begins outside)
      ka = 0;
      kb = (first <= 0 && last >= 0) ? last + 1 : 0;
    } else {
      ka = first > 0 ? first : 0;
      kb = last;
    }
    ka = ka > (int64_t)c.k_lo ? ka : (int64_t)c.k_lo;
    kb = kb < (int64_t)bound ? kb : (int64_t)bound;
    kb = kb < ka + (int64_t)kCastMaxWalk ? kb : ka + (int64_t)kCastMaxWalk;  // (never binds: the intervals above are shorter)
    if (ka > kb) continue;
    uint32_t k = (uint32_t)ka, end = (uint32_t)kb;
    uint32_t found = 0xFFFFFFFFu;
    while (k <= end) {
      const unsigned long long seen = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 24;  // prunes only
      if (seen < (unsigned long long)end) end = (uint32_t)seen;
      bool hit[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        bool outside;
        hit[j] = cv.blocked(v, k + j, a.dst_mask, outside) && k + j <= end;
      }
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        if (found == 0xFFFFFFFFu && __ballot(hit[j]) != 0ull) {
          found = k + j;
          if (hit[j]) {
            const unsigned long long mv = ((unsigned long long)found << 24) | v.key;
            mine = mv < mine ? mv : mine;
          }
        }
      }
      if (found != 0xFFFFFFFFu) break;
      k += 4u;
    }
    if (found < bound) bound = found;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long other = __shfl_xor(mine, d, 64);
    mine = other < mine ? other : mine;
  }
  if (lane == 0u && mine != kCastNoHit) atomicMin(best, mine);
}

__global__ void __launch_bounds__(256) k_cast_count(CastArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform(threadIdx.x >> 6);
  const CastItem it = a.items[blockIdx.x];
  const CastView cv(a.casts[it.cast]);
  const uint64_t m = cv.clipped(a.src_mask, it.cell, lane);
  uint64_t todo = (__ballot(m != 0ull) >> (16u * wave)) & 0xFFFFull;
  const unsigned long long best = a.best[it.cast];  // final: the walk has completed
  const bool has = best != kCastNoHit;
  const uint32_t k = (uint32_t)(best >> 24);
  uint32_t voxels = 0, contacts = 0, wall = 0;
  while (todo) {
    const uint32_t b = uniform(16u * wave + (uint32_t)__builtin_ctzll(todo));
    todo &= todo - 1ull;
    const uint64_t bm = read_lane(m, b);
    voxels += (uint32_t)__popcll(bm);
    if (!has) continue;
    int32_t s0[3];
    const BrickView v = cv.brick(it.cell, b, bm, lane, s0);
    bool outside;
    const bool blk = cv.blocked(v, k, a.dst_mask, outside);
    contacts += (uint32_t)__popcll(__ballot(blk));
    wall |= __ballot(blk && outside) != 0ull ? 1u : 0u;
  }
  if (lane == 0u) {
    CastAcc* acc = a.acc + it.cast;
    if (voxels) atomicAdd(&acc->voxels, voxels);
    if (contacts) atomicAdd(&acc->contacts, contacts);
    if (wall) atomicOr(&acc->wall, 1u);
  }
}

// a source that is not editable: its blocks' occupancy masks scattered into a zeroed lattice of the brick_mask layout
__global__ void __launch_bounds__(256) k_cast_masks(uint64_t* mask, const DustHipBlock* blocks, uint32_t n_blocks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_blocks) return;
  const DustHipBlock b = blocks[i];
  const uint32_t code = leaf_code(b.x >> 2, b.y >> 2, b.z >> 2);
  if (code < kLattice) mask[code] = b.mask;
}

hipError_t launch_cast_masks(uint64_t* mask, const DustHipBlock* blocks, uint32_t n_blocks, hipStream_t s) {
  if (n_blocks) hipLaunchKernelGGL(k_cast_masks, dim3((n_blocks + 255u) / 256u), dim3(256), 0, s, mask, blocks, n_blocks);
  return hipGetLastError();
}

hipError_t launch_cast(const CastArgs& a, hipStream_t s) {
  if (!a.n_items) return hipSuccess;
  hipLaunchKernelGGL(k_cast_walk, dim3(a.n_items), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_cast_count, dim3(a.n_items), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dust
