// edit.hip -- device-side voxel edits and tree (re)build for hierarchy!(4,2,2) models.
//
// The reference's VoxGeometry::set/get (crates/vox/src/geometry.rs:180-185) edit the CPU tree only -- the GPU buffers of a
// loaded model never change -- and Tree::set_value (crates/vdb/src/tree.rs:83-85) is a pointer-chasing insert per voxel.
// Here an edited model keeps its voxels as a dense grid ON THE DEVICE (one byte per voxel, palette index + 1, laid out
// brick-major in Tree::iter_leaf order: 16 MiB for a 256^3 model, created from the model's own blocks the first time it is
// edited); an edit batch is a scatter of bytes into that grid followed by a full rebuild of every array the traversal and
// shading kernels read, with data-parallel scans instead of per-voxel inserts:
//   k_edit_shapes        (dust_hip_model_edit_shapes) boxes, spheres and capsules written into the grid, a wavefront per brick
//   k_edit_brick_masks   one thread per 4^3 brick of the lattice: occupancy mask + voxel count, in both orders that matter
//                        (iter_leaf order for block indices, the collector's block-major order for material_ptr)
//   scan                 exclusive prefix sums of the two 262 144-entry tables (scan.hpp: k_table_scan_local, k_table_scan_sums)
//   k_edit_emit_blocks   Block records (position, mask, material_ptr, avg_albedo) + the compacted material stream
//   k_edit_upper_levels  root mask / rank prefixes, mid nodes, dense_mask, tight bounds, counts (one workgroup)
// The result is, array for array, what dust_hip_model_create builds on the host from the same voxels
// (loader.rs:244-274 + collector.rs + geometry.rs:68-128 + hierarchy.hpp build_hierarchy): tests compare them byte for byte -- the
// Block records and the material stream in tests/test_gpu_edit.py and the tests of the later edit calls, everything
// k_edit_upper_levels writes (root, mid nodes, dense_mask, n_mid, bounds) in tests/test_gpu_hierarchy.py.
// avg_albedo's linear->sRGB curve is a table the HOST evaluates (the same powf the host-side flatten calls), indexed by
// (voxel count, colour sum): the device only adds and looks up, so not one bit depends on a device transcendental.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cell_records.hpp"
#include "edit.hpp"
#include "scan.hpp"
#include "shape_cover.hpp"

namespace dust {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

namespace {

// (leaf_code / leaf_decode, the brick code in Tree::iter_leaf order: grid.hpp)
// collector.rs:25-27: block_index = bx + 64 by + 4096 bz -- the order the material stream is compacted in
__device__ __forceinline__ uint32_t major_code(uint32_t bx, uint32_t by, uint32_t bz) { return bx + 64u * by + 4096u * bz; }

}  // namespace

// first edit of a model: its blocks + material stream -> the dense grid (which the caller zeroed)
__global__ void k_edit_expand(EditArgs e, const DustHipBlock* blocks, const uint8_t* materials, uint32_t n_blocks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ((i >> 6) >= n_blocks) return;
  const DustHipBlock b = blocks[i >> 6];
  const uint32_t bit = i & 63u;
  if (!((b.mask >> bit) & 1ull)) return;
  const uint32_t rank = (uint32_t)__popcll(b.mask & ((1ull << bit) - 1ull));
  e.grid[(size_t)leaf_code(b.x >> 2, b.y >> 2, b.z >> 2) * 64 + bit] = (uint8_t)(materials[b.material_ptr + rank] + 1u);
}

// VoxGeometry::set: value >= 0 -> Some(true) with that palette index, value < 0 -> None
__global__ void k_edit_apply(EditArgs e) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= e.n_edits) return;
  const uint32_t x = e.xyz[i * 3], y = e.xyz[i * 3 + 1], z = e.xyz[i * 3 + 2];
  const int32_t v = e.values[i];
  e.grid[voxel_index(x, y, z)] = v < 0 ? 0u : (uint8_t)(v + 1);
}
// VoxGeometry::get
__global__ void k_edit_read(EditArgs e) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= e.n_edits) return;
  const uint32_t x = e.xyz[i * 3], y = e.xyz[i * 3 + 1], z = e.xyz[i * 3 + 2];
  e.values_out[i] = (int32_t)e.grid[voxel_index(x, y, z)] - 1;
}

// dust_hip_model_edit_shapes: carve / fill / paint / place boxes, spheres and capsules straight into the grid, on the skeleton of
// cell_records.hpp: a workgroup per root cell that some shape's bounds reach, the cell's shape list walked once in call order. Every
// shape record is wave-uniform and rejected by its integer brick bounds before any per-voxel arithmetic. Membership is the header's
// float32 contract, operation for operation: shape_cover.hpp, the text k_census (census.hip) runs too.
__global__ void __launch_bounds__(256) k_edit_shapes(EditShapeArgs a) {
  walk_cell_records(a, [&](CellBricks& c, uint32_t id) -> uint32_t {
    const DevEditShape s = a.shapes[id];
    const uint32_t lo_x = (s.lo & 255u) >> 2, lo_y = ((s.lo >> 8) & 255u) >> 2, lo_z = (s.lo >> 16) >> 2;
    const uint32_t hi_x = (s.hi & 255u) >> 2, hi_y = ((s.hi >> 8) & 255u) >> 2, hi_z = (s.hi >> 16) >> 2;
    if (c.bx < lo_x || c.bx > hi_x) return 0u;
    // voxel centres: small integers + 0.5, exact in float32
    const Voxel p = brick_voxel(c.bx, c.by0, c.bz0, c.lane);
    const float cx = (float)p.x + 0.5f, cy0 = (float)p.y + 0.5f, cz0 = (float)p.z + 0.5f;
    const ShapeCover cover = shape_cover(s.a, s.b, s.kind, s.radius);
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t by = c.by0 + (uint32_t)(k >> 2), bz = c.bz0 + (uint32_t)(k & 3);
      if (by < lo_y || by > hi_y || bz < lo_z || bz > hi_z) continue;
      const float cy = cy0 + (float)((k >> 2) * 4), cz = cz0 + (float)((k & 3) * 4);  // exact
      const bool in = shape_covers(cover, cx, cy, cz);
      const uint32_t g = c.v[k];
      const uint32_t to = g ? (s.solid_to == kEditKeep ? g : s.solid_to) : s.empty_to;
      n += c.set(k, in && to != g, to);
    }
    return n;
  });
}

__global__ void __launch_bounds__(256) k_edit_brick_masks(EditArgs e) {
  const uint32_t code = blockIdx.x * blockDim.x + threadIdx.x;  // iter_leaf order
  const u32x4_t* cells = reinterpret_cast<const u32x4_t*>(e.grid + (size_t)code * 64);
  uint64_t mask = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u32x4_t v = cells[q];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if ((w[k >> 2] >> ((k & 3) * 8)) & 0xFFu) mask |= 1ull << (q * 16 + k);
  }
  e.brick_mask[code] = mask;
  e.flag_leaf[code] = mask != 0 ? 1u : 0u;
  uint32_t bx, by, bz;
  leaf_decode(code, bx, by, bz);
  e.count_major[major_code(bx, by, bz)] = (uint32_t)__popcll(mask);
}

// the exclusive scan of scan.hpp: (1) local scan of 1024 entries per workgroup + block sum, (2) scan of a table's 256 sums
__global__ void __launch_bounds__(256) k_table_scan_local(TableScan t) {
  __shared__ uint32_t sums[256];
  uint32_t* v = t.table[blockIdx.y];
  const uint32_t base = blockIdx.x * 1024u + threadIdx.x * 4u;
  const uint32_t a0 = v[base], a1 = v[base + 1], a2 = v[base + 2], a3 = v[base + 3];
  const uint32_t s = a0 + a1 + a2 + a3;
  const uint32_t before = block_scan_inclusive<256>(sums, s) - s;
  v[base] = before; v[base + 1] = before + a0; v[base + 2] = before + a0 + a1; v[base + 3] = before + a0 + a1 + a2;
  if (threadIdx.x == 255) t.tmp[blockIdx.y * 256 + blockIdx.x] = sums[255];
}
__global__ void __launch_bounds__(256) k_table_scan_sums(TableScan t) {
  __shared__ uint32_t sums[256];
  uint32_t* b = t.tmp + blockIdx.x * 256;
  const uint32_t s = b[threadIdx.x];
  b[threadIdx.x] = block_scan_inclusive<256>(sums, s) - s;
  if (threadIdx.x == 255) *t.total[blockIdx.x] = sums[255];
}

// Block records + material stream (geometry.rs:68-128, collector.rs:50-60): one thread per brick of the lattice
__global__ void __launch_bounds__(256) k_edit_emit_blocks(EditArgs e) {
  const uint32_t code = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t mask = e.brick_mask[code];
  if (mask == 0) return;
  uint32_t bx, by, bz;
  leaf_decode(code, bx, by, bz);
  const uint32_t major = major_code(bx, by, bz);
  const uint32_t index = e.flag_leaf[code] + e.scan_tmp[code >> 10];                   // exclusive scans: local + block base
  const uint32_t ptr = e.count_major[major] + e.scan_tmp[256 + (major >> 10)];
  const uint8_t* cells = e.grid + (size_t)code * 64;
  uint32_t sum[4] = {0, 0, 0, 0}, n = 0;
  for (uint64_t m = mask; m; m &= m - 1ull) {  // ascending bit index: the collector's order inside a block
    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
    const uint32_t pal = (uint32_t)cells[bit] - 1u;
    e.materials[ptr + n] = (uint8_t)pal;
    const uint32_t c = e.palette[pal];
    sum[0] += c & 255u; sum[1] += (c >> 8) & 255u; sum[2] += (c >> 16) & 255u; sum[3] += c >> 24;
    ++n;
  }
  const uint16_t* row = e.srgb_lut + (size_t)(n - 1u) * kSrgbRow;
  const float alpha = (float)sum[3] / ((float)n * 255.0f);  // geometry.rs:97,109: no transfer curve on alpha
  DustHipBlock b;
  b.x = (uint16_t)(bx * 4u); b.y = (uint16_t)(by * 4u); b.z = (uint16_t)(bz * 4u); b.w = 0;
  b.mask = mask;
  b.material_ptr = ptr;
  b.avg_albedo = ((uint32_t)row[sum[0]] << 22) | ((uint32_t)row[sum[1]] << 12) | ((uint32_t)row[sum[2]] << 2) | (uint32_t)(alpha * 3.0f);
  e.blocks[index] = b;
}

// root node, mid nodes, dense_mask, bounds: one workgroup of 1024 threads, four root cells each (hierarchy.hpp build_hierarchy)
__global__ void __launch_bounds__(1024) k_edit_upper_levels(EditArgs e) {
  __shared__ uint32_t part[1024];
  __shared__ uint64_t root_mask[64];
  __shared__ int lo[3], hi[3];
  if (threadIdx.x < 64) root_mask[threadIdx.x] = 0;
  if (threadIdx.x < 3) { lo[threadIdx.x] = 1 << 30; hi[threadIdx.x] = -1; }
  __syncthreads();
  uint64_t child[4];
  uint32_t mine = 0;
  for (int k = 0; k < 4; ++k) {
    const uint32_t cell = threadIdx.x * 4u + k;  // root child index (x>>4)<<8 | (y>>4)<<4 | (z>>4)
    uint64_t m = 0;
    for (uint32_t c = 0; c < 64; ++c) m |= (uint64_t)(e.brick_mask[cell * 64u + c] != 0) << c;
    child[k] = m;
    if (m) {
      mine += 1;
      atomicOr((unsigned long long*)&root_mask[cell >> 6], 1ull << (cell & 63u));
      for (uint64_t mm = m; mm; mm &= mm - 1ull) {  // tight bounds over the bricks
        uint32_t bx, by, bz;
        leaf_decode(cell * 64u + (uint32_t)__builtin_ctzll(mm), bx, by, bz);
        atomicMin(&lo[0], (int)bx * 4); atomicMin(&lo[1], (int)by * 4); atomicMin(&lo[2], (int)bz * 4);
        atomicMax(&hi[0], (int)bx * 4 + 4); atomicMax(&hi[1], (int)by * 4 + 4); atomicMax(&hi[2], (int)bz * 4 + 4);
      }
    }
  }
  uint32_t mi = block_scan_inclusive<1024>(part, mine) - mine;  // mid nodes are stored in root-child order == depth first
  for (int k = 0; k < 4; ++k) {
    if (!child[k]) continue;
    const uint32_t cell = threadIdx.x * 4u + k;
    const uint32_t first_code = cell * 64u + (uint32_t)__builtin_ctzll(child[k]);
    DevN4 n;
    n.mask_lo = (uint32_t)child[k]; n.mask_hi = (uint32_t)(child[k] >> 32);
    n.first_block = e.flag_leaf[first_code] + e.scan_tmp[first_code >> 10];
    n.pad = 0;
    e.mid[mi] = n;
    for (uint32_t c = 0; c < 64; ++c) e.dense_mask[(size_t)mi * 64 + c] = e.brick_mask[cell * 64u + c];
    ++mi;
  }
  if (threadIdx.x < 64) {  // the N16 node: 64 mask words, 64 u16 rank prefixes, child_base 0
    reinterpret_cast<uint64_t*>(e.root)[threadIdx.x] = root_mask[threadIdx.x];
    uint32_t run = 0;
    for (uint32_t w = 0; w < threadIdx.x; ++w) run += (uint32_t)__popcll(root_mask[w]);
    reinterpret_cast<uint16_t*>(e.root + 512)[threadIdx.x] = (uint16_t)run;
  }
  if (threadIdx.x == 0) {
    *reinterpret_cast<uint32_t*>(e.root + 640) = 0u;
    e.header->n_mid = part[1023];
    const bool any = part[1023] != 0;
    for (int a = 0; a < 3; ++a) { e.header->bmin[a] = any ? (float)lo[a] : 0.0f; e.header->bmax[a] = any ? (float)hi[a] : 0.0f; }
  }
}

// ------------------------------------------------------------------ launchers (capi_model.cpp)
hipError_t launch_edit_expand(const EditArgs& e, const DustHipBlock* blocks, const uint8_t* materials, uint32_t n_blocks, hipStream_t s) {
  if (n_blocks) hipLaunchKernelGGL(k_edit_expand, dim3((n_blocks * 64u + 255u) / 256u), dim3(256), 0, s, e, blocks, materials, n_blocks);
  return hipGetLastError();
}
hipError_t launch_edit_apply(const EditArgs& e, bool read, hipStream_t s) {
  if (e.n_edits == 0) return hipSuccess;
  if (read) hipLaunchKernelGGL(k_edit_read, dim3((e.n_edits + 255u) / 256u), dim3(256), 0, s, e);
  else hipLaunchKernelGGL(k_edit_apply, dim3((e.n_edits + 255u) / 256u), dim3(256), 0, s, e);
  return hipGetLastError();
}
hipError_t launch_edit_shapes(const EditShapeArgs& a, hipStream_t s) {
  if (a.n_cells) hipLaunchKernelGGL(k_edit_shapes, dim3(a.n_cells), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_table_scan(const TableScan& t, uint32_t n_tables, hipStream_t s) {
  hipLaunchKernelGGL(k_table_scan_local, dim3(kLattice / 1024, n_tables), dim3(256), 0, s, t);
  hipLaunchKernelGGL(k_table_scan_sums, dim3(n_tables), dim3(256), 0, s, t);
  return hipGetLastError();
}
hipError_t launch_edit_rebuild(const EditArgs& e, hipStream_t s) {
  hipLaunchKernelGGL(k_edit_brick_masks, dim3(kLattice / 256), dim3(256), 0, s, e);
  const hipError_t err = launch_table_scan(TableScan{{e.flag_leaf, e.count_major}, {&e.header->n_blocks, &e.header->n_materials}, e.scan_tmp}, 2, s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_edit_emit_blocks, dim3(kLattice / 256), dim3(256), 0, s, e);
  hipLaunchKernelGGL(k_edit_upper_levels, dim3(1), dim3(1024), 0, s, e);
  return hipGetLastError();
}

}  // namespace dust
