// capi_model.cpp -- the model handle of the C ABI (include/dust_hip.h): the upload of the device hierarchy, device-side voxel and shape
// edits (edit.hip), model stamps (stamp.hip), model casts (cast.hip), model islands (island.hip), model floods (flood.hip), model
// distances (distance.hip), model reductions (reduce.hip), model censuses (census.hip), model surfaces (surface.hip), model meshes (mesh.hip), model boxes (boxes.hip), model deltas
// (delta.hip), model columns (column.hip) and model fracture (fracture.hip). What needs no device is in three headers: the hierarchy build itself
// (root, l2, mid, dense_mask, the per-cell table, bounds) in hierarchy.hpp, the arithmetic on the callers' records (conversion, chunks,
// cell lists, cast hits, census records, surface, mesh, delta and columns queries, a delta_apply's records) in model_records.hpp, a reduction's vote and the plan of its levels in reduce_rule.hpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_set>

#include "capi_internal.hpp"
#include "vdb.hpp"
#include "distance.hpp"
#include "field.hpp"
#include "flood.hpp"
#include "fracture.hpp"
#include "hierarchy.hpp"
#include "island.hpp"
#include "model_records.hpp"
#include "reduce.hpp"
#include "reduce_rule.hpp"
#include "scan.hpp"

void release(const DustHipModel* cm) {
  DustHipModel* m = const_cast<DustHipModel*>(cm);
  if (!m || m->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  DustHipContext* c = m->ctx;
  (void)hipSetDevice(c->device);
  (void)sync_stream(c);  // launches that read the arrays are done before they go
  delete m;
  release(c);
}

extern "C" {

DustStatus dust_hip_model_create(DustHipContext* ctx, const DustHipBlock* blocks, uint32_t n_blocks,
                                 const uint8_t* materials, uint64_t n_materials, const uint8_t* palette,
                                 uint32_t tree_extent_log2, DustHipModel** out) {
  if (!ctx || !out || (!blocks && n_blocks) || (!materials && n_materials) || !palette)
    return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (tree_extent_log2 != 8 && tree_extent_log2 != 12)
    return fail(DUST_ERR_INVALID_ARGUMENT, "tree_extent_log2 must be 8 (hierarchy 4,2,2) or 12 (hierarchy 4,4,2,2)");
  return guarded([&]() -> DustStatus {
    dust::Hierarchy h;
    const char* refusal = nullptr;
    const DustStatus s = dust::build_hierarchy(blocks, n_blocks, tree_extent_log2, h, &refusal);
    if (s != DUST_OK) return fail(s, refusal);
    dust::N16Builder& root = h.root;
    dust::N16Builder& l2 = h.l2;
    const std::vector<dust::DevN4>& mid = h.mid;
    const std::vector<uint64_t>& dense_mask = h.dense_mask;
    for (uint32_t i = 0; i < n_blocks; ++i) {
      const uint64_t need = uint64_t(blocks[i].material_ptr) + uint64_t(__builtin_popcountll(blocks[i].mask));
      if (need > n_materials) return fail(DUST_ERR_INVALID_ARGUMENT, "block material_ptr runs past the material buffer");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    // (owned through the reference count from here on: an early return releases it, and with it the context reference)
    struct Drop { DustHipModel* m; ~Drop() { release(m); } } owner{new DustHipModel};
    DustHipModel* m = owner.m;
    m->ctx = retain(ctx);
    const hipStream_t up = ctx->stream;
    HIP_TRY(m->root.upload(root.bytes.data(), root.bytes.size(), up));
    m->host_root.assign(root.bytes.begin(), root.bytes.begin() + dust::kN16LdsBytes);
    HIP_TRY(m->l2.upload(l2.bytes.data(), l2.bytes.size(), up));
    if (tree_extent_log2 == 12) {  // the per-cell table the DEEP kernel variants look 16-cells up in: {mid index, child mask} per cell
      dust::build_l2_cells(h);
      HIP_TRY(m->l2_cells.upload(h.l2_cells.data(), h.l2_cells.size() * sizeof(dust::DevL2Cell), up));
    }
    HIP_TRY(m->mid.upload(mid.data(), mid.size() * sizeof(dust::DevN4), up));
    HIP_TRY(m->dense_mask.upload(dense_mask.data(), dense_mask.size() * 8, up));
    HIP_TRY(m->blocks.upload(blocks, size_t(n_blocks) * sizeof(DustHipBlock), up));
    HIP_TRY(m->materials.upload(materials, size_t(n_materials), up));
    m->has_material_255 = n_materials && std::memchr(materials, 255, size_t(n_materials)) != nullptr;
    uint32_t pal[256];
    std::memset(pal, 0, sizeof(pal));
    std::memcpy(pal, palette, 255 * 4);  // loader.rs:214-218: entries 0..254
    HIP_TRY(m->palette.upload(pal, sizeof(pal), up));
    dust::DevModel& d = m->dev;
    d.root = static_cast<const uint8_t*>(m->root.p);
    d.l2 = tree_extent_log2 == 12 ? static_cast<const uint8_t*>(m->l2.p) : nullptr;
    d.l2_cells = tree_extent_log2 == 12 ? static_cast<const dust::DevL2Cell*>(m->l2_cells.p) : nullptr;
    d.mid = static_cast<const dust::DevN4*>(m->mid.p);
    d.dense_mask = static_cast<const uint64_t*>(m->dense_mask.p);
    d.blocks = static_cast<const DustHipBlock*>(m->blocks.p);
    d.materials = static_cast<const uint8_t*>(m->materials.p);
    d.palette = static_cast<const uint32_t*>(m->palette.p);
    std::memcpy(d.bmin, h.bmin, sizeof(h.bmin));
    std::memcpy(d.bmax, h.bmax, sizeof(h.bmax));
    d.extent = 1u << tree_extent_log2;
    d.n_levels = tree_extent_log2 == 12 ? 3 : 2;
    d.n_blocks = n_blocks;
    d.lds_slot = -1;
    m->n_materials = n_materials;
    m->n_mid = uint32_t(mid.size());
    m->n_l2 = uint32_t(l2.count());
    *out = retain(m);  // the caller's reference (the guard drops the builder's)
    return DUST_OK;
  });
}
void dust_hip_model_destroy(DustHipModel* m) { release(m); }  // (a scene that instances it keeps it alive)

// ---------------------------------------------------------------- device-side edits (edit.hip)
namespace {
float linear2srgb_host(float c) { return c <= 0.0031308f ? 12.92f * c : 1.055f * std::pow(c, 1.0f / 2.4f) - 0.055f; }  // geometry.rs:99-105

DustStatus ensure_srgb_lut(DustHipContext* ctx) {
  if (ctx->srgb_lut.p) return DUST_OK;
  std::vector<uint16_t> lut(size_t(64) * dust::kSrgbRow, 0);
  for (uint32_t n = 1; n <= 64; ++n) {
    const float denom = float(n) * 255.0f;
    for (uint32_t sum = 0; sum <= n * 255u; ++sum)
      lut[size_t(n - 1) * dust::kSrgbRow + sum] = uint16_t(uint32_t(linear2srgb_host(float(sum) / denom) * 1023.0f));
  }
  HIP_TRY(ctx->srgb_lut.upload(lut.data(), lut.size() * 2, ctx->stream));
  return DUST_OK;
}

dust::EditArgs edit_args(DustHipModel* m, EditState& st) {
  dust::EditArgs e{};
  e.grid = static_cast<uint8_t*>(st.grid.p);
  e.brick_mask = static_cast<uint64_t*>(st.brick_mask.p);
  e.flag_leaf = static_cast<uint32_t*>(st.flag_leaf.p);
  e.count_major = static_cast<uint32_t*>(st.count_major.p);
  e.scan_tmp = static_cast<uint32_t*>(st.scan_tmp.p);
  e.blocks = static_cast<DustHipBlock*>(m->blocks.p);
  e.materials = static_cast<uint8_t*>(m->materials.p);
  e.palette = static_cast<const uint32_t*>(m->palette.p);
  e.srgb_lut = static_cast<const uint16_t*>(m->ctx->srgb_lut.p);
  e.root = static_cast<uint8_t*>(m->root.p);
  e.mid = static_cast<dust::DevN4*>(m->mid.p);
  e.dense_mask = static_cast<uint64_t*>(m->dense_mask.p);
  e.header = static_cast<dust::EditHeader*>(st.header.p);
  return e;
}

// run the rebuild kernels and bring the model record up to date (sizes, bounds, the root the scene stages in LDS)
DustStatus rebuild_and_refresh(DustHipModel* m, EditState& es) {
  hipStream_t st = m->ctx->stream;
  HIP_TRY(dust::launch_edit_rebuild(edit_args(m, es), st));
  dust::EditHeader h{};
  HIP_TRY(hipMemcpyAsync(&h, es.header.p, sizeof(h), hipMemcpyDeviceToHost, st));
  m->host_root.resize(dust::kN16LdsBytes);
  HIP_TRY(hipMemcpyAsync(m->host_root.data(), m->root.p, dust::kN16LdsBytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  m->dev.n_blocks = h.n_blocks;
  m->n_materials = h.n_materials;
  m->n_mid = h.n_mid;
  std::memcpy(m->dev.bmin, h.bmin, sizeof(h.bmin));
  std::memcpy(m->dev.bmax, h.bmax, sizeof(h.bmax));
  m->generation += 1;
  return DUST_OK;
}

// first edit: move the model into full-capacity buffers and expand its voxels into the dense grid. The model becomes
// editable (m->edit set) only when every step has succeeded: a failure leaves it exactly as it was.
DustStatus editable_kind(const DustHipModel* m) {
  if (m->dev.extent != 256) return fail(DUST_ERR_UNSUPPORTED, "device-side edits cover hierarchy (4,2,2) models (256^3); rebuild larger trees with dust_hip_model_create");
  if (m->has_material_255) return fail(DUST_ERR_UNSUPPORTED, "the model holds material byte 255 (the edit grid stores palette index + 1 in a byte; dust_hip_model_set_voxels takes 0..254)");
  return DUST_OK;
}
// (`rebuild` false: the caller fills the grid and rebuilds itself -- a model born editable, dust_hip_model_detach_islands)
DustStatus make_editable(DustHipModel* m, bool rebuild = true) {
  if (m->edit) return DUST_OK;
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  s = ensure_srgb_lut(m->ctx);
  if (s != DUST_OK) return s;
  hipStream_t st = m->ctx->stream;
  std::unique_ptr<EditState> e(new EditState);
  const size_t L = dust::kLattice;
  HIP_TRY(e->grid.alloc(L * 64));
  HIP_TRY(hipMemsetAsync(e->grid.p, 0, L * 64, st));
  HIP_TRY(e->brick_mask.alloc(L * 8));
  HIP_TRY(e->flag_leaf.alloc(L * 4));
  HIP_TRY(e->count_major.alloc(L * 4));
  HIP_TRY(e->scan_tmp.alloc(512 * 4));
  HIP_TRY(e->header.alloc(sizeof(dust::EditHeader)));
  DeviceBuffer blocks, materials, mid, dense_mask;
  HIP_TRY(blocks.alloc(L * sizeof(DustHipBlock)));
  HIP_TRY(materials.alloc(L * 64));
  HIP_TRY(mid.alloc(4096 * sizeof(dust::DevN4)));
  HIP_TRY(dense_mask.alloc(size_t(4096) * 64 * 8));
  dust::EditArgs a = edit_args(m, *e);  // (expand only writes the grid)
  HIP_TRY(dust::launch_edit_expand(a, static_cast<const DustHipBlock*>(m->blocks.p), static_cast<const uint8_t*>(m->materials.p), m->dev.n_blocks, st));
  HIP_TRY(sync_stream(m->ctx));  // every launch that reads the old arrays is done (both streams of the context)
  auto swap_all = [&] {
    m->blocks.swap(blocks); m->materials.swap(materials); m->mid.swap(mid); m->dense_mask.swap(dense_mask);
    m->dev.mid = static_cast<const dust::DevN4*>(m->mid.p);
    m->dev.dense_mask = static_cast<const uint64_t*>(m->dense_mask.p);
    m->dev.blocks = static_cast<const DustHipBlock*>(m->blocks.p);
    m->dev.materials = static_cast<const uint8_t*>(m->materials.p);
  };
  swap_all();
  // the same voxels, now in the full-capacity arrays (bumps the generation: scenes holding the old addresses commit again)
  s = rebuild ? rebuild_and_refresh(m, *e) : DUST_OK;
  if (s != DUST_OK) { swap_all(); return s; }  // back to the tightly sized originals, untouched
  m->edit = std::move(e);
  return DUST_OK;
}
// what every call that works on the grid begins with
DustStatus begin_edit(DustHipModel* m) {
  HIP_TRY(hipSetDevice(m->ctx->device));
  HIP_TRY(join_side(m->ctx));  // (a surfel pass on the second stream still traces the model as it is)
  return make_editable(m);
}
void invalidate_fields(EditState& es) { es.flood.valid = es.distance.valid = es.fracture.valid = false; }  // (the fields describe the voxels as they were)
// a call that may change a voxel is about to run
void invalidate_derived(EditState& es) {
  es.labels_valid = false;  // (dust_hip_model_find_islands' labelling describes the voxels as they were)
  invalidate_fields(es);
}
// a buffer of one fixed size, allocated by the first call that needs it; out of device memory leaves it released
DustStatus lazy_alloc(DeviceBuffer& b, size_t bytes, const char* what) {
  if (b.p) return DUST_OK;
  const hipError_t e = b.alloc(bytes);
  if (e == hipSuccess) return DUST_OK;
  b.release();
  return hip_fail(e, what);
}

DustStatus check_coordinates(const uint32_t* xyz, uint32_t n, uint32_t extent = 256u) {
  for (uint32_t i = 0; i < n; ++i)
    if (xyz[i * 3] >= extent || xyz[i * 3 + 1] >= extent || xyz[i * 3 + 2] >= extent)
      return fail(DUST_ERR_INVALID_ARGUMENT, "voxel coordinate outside the tree extent");
  return DUST_OK;
}
DustStatus no_labelling() { return fail(DUST_ERR_NOT_READY, "the model has no valid island labelling: call dust_hip_model_find_islands (again after an edit)"); }
DustStatus no_distance() { return fail(DUST_ERR_NOT_READY, "the model has no valid distance field: call dust_hip_model_distance (again after an edit)"); }
DustStatus no_field() { return fail(DUST_ERR_NOT_READY, "the model has no valid flood field: call dust_hip_model_flood (again after an edit)"); }
DustStatus no_cells() { return fail(DUST_ERR_NOT_READY, "the model has no valid cell labelling: call dust_hip_model_fracture (again after an edit)"); }

DustStatus upload_batch(DustHipModel* m, const uint32_t* xyz, const int32_t* values, uint32_t n, bool with_values) {
  EditState& e = *m->edit;
  DustStatus s = grow(m->ctx, e.xyz, size_t(n) * 12);
  if (s == DUST_OK) s = grow(m->ctx, e.values, size_t(n) * 4);
  if (s != DUST_OK) return s;
  HIP_TRY(hipMemcpyAsync(e.xyz.p, xyz, size_t(n) * 12, hipMemcpyHostToDevice, m->ctx->stream));
  if (with_values) HIP_TRY(hipMemcpyAsync(e.values.p, values, size_t(n) * 4, hipMemcpyHostToDevice, m->ctx->stream));
  return DUST_OK;
}

extern "C++" {  // (templates: no C linkage)
// dust_hip_model_island_of / field_at: n coordinates up, one launch over them, n elements of type T back
template <class T, class Launch>
DustStatus lookup_call(DustHipModel* m, const uint32_t* xyz, T* out, uint32_t n, Launch&& launch) {
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    DustStatus s;
    if ((s = grow(ctx, ctx->stage_in, size_t(n) * 12)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_out, size_t(n) * sizeof(T))) != DUST_OK) return s;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, xyz, size_t(n) * 12, hipMemcpyHostToDevice, st));
    if ((s = launch(static_cast<const uint32_t*>(ctx->stage_in.p), static_cast<T*>(ctx->stage_out.p), st)) != DUST_OK) return s;
    HIP_TRY(hipMemcpyAsync(out, ctx->stage_out.p, size_t(n) * sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DUST_OK;
  });
}

// dust_hip_model_flood_at / _distance_at: the values of field `which` at n coordinates; `none`: the refusal while it is not valid
DustStatus field_at(DustHipModel* m, VoxelField EditState::*which, DustStatus (*none)(), const uint32_t* xyz, uint16_t* out, uint32_t n) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (n && (!xyz || !out)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if ((s = check_coordinates(xyz, n)) != DUST_OK) return s;
  if (!m->edit || !(*m->edit.*which).valid) return none();
  if (n == 0) return DUST_OK;
  return lookup_call(m, xyz, out, n, [&](const uint32_t* in, uint16_t* values, hipStream_t st) -> DustStatus {
    HIP_TRY(dust::launch_lookup(static_cast<const uint16_t*>((*m->edit.*which).values.p), in, values, n, st));
    return DUST_OK;
  });
}

// dust_hip_model_flood_apply / _distance_apply: the voxels whose value in field `which` lies in lo..hi take `value`; then the rebuild
DustStatus field_apply(DustHipModel* m, VoxelField EditState::*which, DustStatus (*none)(), uint32_t lo, uint32_t hi, int32_t value, uint32_t* changed) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (value > 254) return fail(DUST_ERR_INVALID_ARGUMENT, "palette index must be 0..254 (or negative to clear the voxels)");
  if (!m->edit || !(*m->edit.*which).valid) return none();
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(join_side(ctx));  // (a surfel pass on the second stream still traces the model as it is)
    EditState& es = *m->edit;
    const VoxelField& f = es.*which;
    hipStream_t st = ctx->stream;
    invalidate_derived(es);
    uint32_t n = 0;
    if (f.count && lo <= hi) {
      if ((s = grow(ctx, es.changed, 4)) != DUST_OK) return s;
      dust::FieldApplyArgs a{};
      a.grid = static_cast<uint8_t*>(es.grid.p);
      a.field = static_cast<const uint16_t*>(f.values.p);
      a.lo = lo; a.hi = hi;
      a.byte = value < 0 ? 0u : uint32_t(value) + 1u;
      a.box = f.box;
      a.changed = static_cast<uint32_t*>(es.changed.p);
      HIP_TRY(hipMemsetAsync(a.changed, 0, 4, st));
      HIP_TRY(dust::launch_field_apply(a, st));
      HIP_TRY(hipMemcpyAsync(&n, a.changed, 4, hipMemcpyDeviceToHost, st));
    }
    s = rebuild_and_refresh(m, es);  // synchronises
    if (s != DUST_OK) return s;
    if (changed) *changed = n;
    return DUST_OK;
  });
}

// The chunks of a call batched by root cell (shape edits, stamps, censuses), from the records that cover something (`dev`, in call
// order) to one launch each. Order-preserving chunks: a chunk's records binned into the 4096 root cells, an ascending list of u16
// record ids per cell in CSR form, uploaded into `cells` / `starts` / `ids` (the caller's buffers: an EditState's, or the context's for a
// model that has none); one workgroup per non-empty cell. `launch(c0, a)` gets the chunk's first record and arguments with the cell
// lists filled in (cells, cell_start, ids, n_cells); it adds its own and launches. `lists` is the caller's: the last chunk's copies read
// it until the caller has waited for the stream.
template <class Args, class Rec, class Launch>
DustStatus for_each_chunk(DustHipContext* ctx, const std::vector<Rec>& dev, dust::CellLists& lists, DeviceBuffer& cells, DeviceBuffer& starts, DeviceBuffer& ids,
                          Launch&& launch) {
  hipStream_t st = ctx->stream;
  DustStatus s;
  for (size_t c0 = 0; c0 < dev.size();) {
    const size_t c1 = dust::chunk_end(dev, c0, dust::kShapeChunkIds, dust::kShapeChunkRecords);
    if (c0 != 0) HIP_TRY(hipStreamSynchronize(st));  // the previous chunk's copies have left the host lists
    lists.bin(dev, c0, c1);
    if ((s = grow(ctx, cells, lists.cells.size() * 4)) != DUST_OK) return s;
    if ((s = grow(ctx, starts, lists.starts.size() * 4)) != DUST_OK) return s;
    if ((s = grow(ctx, ids, lists.ids.size() * 2)) != DUST_OK) return s;
    HIP_TRY(hipMemcpyAsync(cells.p, lists.cells.data(), lists.cells.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(starts.p, lists.starts.data(), lists.starts.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ids.p, lists.ids.data(), lists.ids.size() * 2, hipMemcpyHostToDevice, st));
    Args a{};
    a.cells = static_cast<const uint32_t*>(cells.p);
    a.cell_start = static_cast<const uint32_t*>(starts.p);
    a.ids = static_cast<const uint16_t*>(ids.p);
    a.n_cells = uint32_t(lists.cells.size());
    if ((s = launch(c0, a)) != DUST_OK) return s;
    c0 = c1;
  }
  return DUST_OK;
}

// The calls that write the grid (shape edits, stamps): index[k] is record k's place among the caller's n. The chunks as above; `launch`
// gets the grid and the chunk's part of `changed` besides. Then the rebuild, and the counts to the caller's `changed`.
template <class Args, class Rec, class Launch>
DustStatus batched_edit(DustHipModel* m, const std::vector<Rec>& dev, const std::vector<uint32_t>& index, uint32_t n, uint32_t* changed, Launch&& launch) {
  DustHipContext* ctx = m->ctx;
  EditState& es = *m->edit;
  hipStream_t st = ctx->stream;
  const size_t live = dev.size();
  std::vector<uint32_t> counts(live, 0u);
  DustStatus s;
  if (live) {
    if ((s = grow(ctx, es.shapes, live * sizeof(Rec))) != DUST_OK) return s;
    if ((s = grow(ctx, es.changed, live * 4)) != DUST_OK) return s;
    HIP_TRY(hipMemcpyAsync(es.shapes.p, dev.data(), live * sizeof(Rec), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(es.changed.p, 0, live * 4, st));
  }
  dust::CellLists lists;
  s = for_each_chunk<Args>(ctx, dev, lists, es.shape_cells, es.shape_starts, es.shape_ids, [&](size_t c0, Args& a) -> DustStatus {
    a.grid = static_cast<uint8_t*>(es.grid.p);
    a.changed = static_cast<uint32_t*>(es.changed.p) + c0;
    return launch(c0, a);
  });
  if (s != DUST_OK) return s;
  if (live) HIP_TRY(hipMemcpyAsync(counts.data(), es.changed.p, live * 4, hipMemcpyDeviceToHost, st));
  s = rebuild_and_refresh(m, es);  // synchronises: the host vectors above stay alive until the copies are done
  if (s != DUST_OK) return s;
  if (changed) {
    std::fill(changed, changed + n, 0u);
    for (size_t k = 0; k < live; ++k) changed[index[k]] = counts[k];
  }
  return DUST_OK;
}
}  // extern "C++"
}  // namespace

DustStatus dust_hip_model_set_voxels(DustHipModel* m, const uint32_t* xyz, const int32_t* values, uint32_t n) {
  if (!m || (n && (!xyz || !values))) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  for (uint32_t i = 0; i < n; ++i) {  // (voxel by voxel: the first voxel that is wrong in either way is the one refused)
    const DustStatus s = check_coordinates(xyz + size_t(i) * 3, 1, m->dev.extent);
    if (s != DUST_OK) return s;
    if (values[i] > 254) return fail(DUST_ERR_INVALID_ARGUMENT, "palette index must be 0..254 (or negative to clear the voxel)");
  }
  return guarded([&]() -> DustStatus {
    DustStatus s = begin_edit(m);
    if (s != DUST_OK || n == 0) return s;
    // a voxel named more than once takes its LAST value (what a sequence of set calls would leave): keep the last entry
    std::vector<uint32_t> ux;
    std::vector<int32_t> uv;
    std::unordered_set<uint32_t> seen;
    ux.reserve(size_t(n) * 3); uv.reserve(n);
    for (uint32_t k = n; k-- > 0;) {
      const uint32_t key = (xyz[k * 3] << 16) | (xyz[k * 3 + 1] << 8) | xyz[k * 3 + 2];
      if (!seen.insert(key).second) continue;
      ux.push_back(xyz[k * 3]); ux.push_back(xyz[k * 3 + 1]); ux.push_back(xyz[k * 3 + 2]);
      uv.push_back(values[k]);
    }
    const uint32_t un = uint32_t(uv.size());
    invalidate_derived(*m->edit);
    s = upload_batch(m, ux.data(), uv.data(), un, true);
    if (s != DUST_OK) return s;
    dust::EditArgs a = edit_args(m, *m->edit);
    a.xyz = static_cast<const uint32_t*>(m->edit->xyz.p);
    a.values = static_cast<const int32_t*>(m->edit->values.p);
    a.n_edits = un;
    HIP_TRY(dust::launch_edit_apply(a, false, m->ctx->stream));
    return rebuild_and_refresh(m, *m->edit);  // synchronises: the host vectors above stay alive until the copies are done
  });
}

// ---- shape edits (edit.hip k_edit_shapes)
DustStatus dust_hip_model_edit_shapes(DustHipModel* m, const DustHipEditShape* shapes, uint32_t n, uint32_t* changed) {
  if (!m || (n && !shapes)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (n > DUST_HIP_MAX_EDIT_SHAPES) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_EDIT_SHAPES shapes in one call");
  for (uint32_t i = 0; i < n; ++i) {
    if (shapes[i].kind > DUST_HIP_SHAPE_CAPSULE) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown shape kind");
    if (shapes[i].op > DUST_HIP_EDIT_PLACE) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown edit op");
    if (shapes[i].op != DUST_HIP_EDIT_CARVE && (shapes[i].palette < 0 || shapes[i].palette > 254))
      return fail(DUST_ERR_INVALID_ARGUMENT, "palette index must be 0..254");
  }
  return guarded([&]() -> DustStatus {
    DustStatus s = begin_edit(m);
    if (s != DUST_OK || n == 0) return s;
    EditState& es = *m->edit;
    invalidate_derived(es);
    std::vector<dust::DevEditShape> dev;
    std::vector<uint32_t> index;
    dust::live_records<dust::device_shape>(shapes, n, dev, index);
    return batched_edit<dust::EditShapeArgs>(m, dev, index, n, changed, [&](size_t c0, dust::EditShapeArgs& a) -> DustStatus {
      a.shapes = static_cast<const dust::DevEditShape*>(es.shapes.p) + c0;
      HIP_TRY(dust::launch_edit_shapes(a, m->ctx->stream));
      return DUST_OK;
    });
  });
}

// ---- model stamps (stamp.hip k_stamp)
namespace {
// A source model as it stands now, as a grid, for a call that only reads it (stamps, reductions): its own when it is editable (read
// in place), expanded into a scratch grid when it is not (the source itself is not touched), and a copy of the grid of `m`,
// the editable model the call writes (null: none), when that is the source too -- a model stamped onto itself. `scratch`: the
// context's stamp_grid unless the call holds two expansions at once (dust_hip_model_delta)
DustStatus source_grid(DustHipContext* ctx, const DustHipModel* m, const DustHipModel* src, const uint8_t** source, DeviceBuffer* scratch = nullptr) {
  hipStream_t st = ctx->stream;
  if (src != m && src->edit) {
    *source = static_cast<const uint8_t*>(src->edit->grid.p);
    return DUST_OK;
  }
  DeviceBuffer& grid = scratch ? *scratch : ctx->stamp_grid;
  const size_t grid_bytes = size_t(dust::kLattice) * 64;
  DustStatus s = lazy_alloc(grid, grid_bytes, "the source grid (16 MiB)");
  if (s != DUST_OK) return s;
  if (src == m) {
    HIP_TRY(hipMemcpyAsync(grid.p, m->edit->grid.p, grid_bytes, hipMemcpyDeviceToDevice, st));
  } else {
    HIP_TRY(hipMemsetAsync(grid.p, 0, grid_bytes, st));
    dust::EditArgs e{};  // (expand only writes the grid)
    e.grid = static_cast<uint8_t*>(grid.p);
    HIP_TRY(dust::launch_edit_expand(e, static_cast<const DustHipBlock*>(src->blocks.p), static_cast<const uint8_t*>(src->materials.p), src->dev.n_blocks, st));
  }
  *source = static_cast<const uint8_t*>(grid.p);
  return DUST_OK;
}
}  // namespace

DustStatus dust_hip_model_stamp(DustHipModel* m, const DustHipModel* src, const DustHipStamp* stamps, uint32_t n, const uint8_t* palette_map,
                                uint32_t* changed) {
  if (!m || !src || (n && !stamps)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (n > DUST_HIP_MAX_STAMPS) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_STAMPS stamps in one call");
  if (m->ctx != src->ctx) return fail(DUST_ERR_INVALID_ARGUMENT, "the source and the destination belong to different contexts");
  DustStatus s = editable_kind(m);  // (before the stamps are looked at)
  if (s == DUST_OK) s = editable_kind(src);
  if (s != DUST_OK) return s;
  for (uint32_t i = 0; i < n; ++i) {
    if (!dust::valid_orient(stamps[i].orient)) return fail(DUST_ERR_INVALID_ARGUMENT, "orient is not a signed axis permutation (p a permutation of 0, 1, 2; bits 9 and above zero)");
    if (stamps[i].op > DUST_HIP_STAMP_PAINT) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown stamp op");
  }
  uint8_t map[256];  // grid byte (palette index + 1, 0 = None) -> grid byte
  map[0] = 0;
  for (uint32_t i = 0; i < 255; ++i) {
    if (palette_map && palette_map[i] > 254) return fail(DUST_ERR_INVALID_ARGUMENT, "palette_map entries must be 0..254");
    map[i + 1] = uint8_t((palette_map ? palette_map[i] : i) + 1u);
  }
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    DustStatus s = begin_edit(m);
    if (s != DUST_OK || n == 0) return s;
    EditState& es = *m->edit;
    invalidate_derived(es);
    std::vector<dust::DevStamp> dev;
    std::vector<uint32_t> index;
    dust::live_records<dust::device_stamp>(stamps, n, dev, index);
    const uint8_t* source = nullptr;
    if (!dev.empty()) {
      if ((s = source_grid(ctx, m, src, &source)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_aux, sizeof(map))) != DUST_OK) return s;
      HIP_TRY(hipMemcpyAsync(ctx->stage_aux.p, map, sizeof(map), hipMemcpyHostToDevice, ctx->stream));
    }
    return batched_edit<dust::StampArgs>(m, dev, index, n, changed, [&](size_t c0, dust::StampArgs& a) -> DustStatus {
      a.src = source;
      a.stamps = static_cast<const dust::DevStamp*>(es.shapes.p) + c0;
      a.palette_map = static_cast<const uint8_t*>(ctx->stage_aux.p);
      HIP_TRY(dust::launch_stamp(a, ctx->stream));
      return DUST_OK;
    });
  });
}

// ---- model resampling (resample.hip k_resample / k_resample_count): a stamp whose geometry is a fixed-point affine map. The real call
// goes through batched_edit as a stamp does -- `changed` in its one word per record, the three further counts in stage_out beside it --,
// the dry run through the read-only chunking on the destination's own lists, with no rebuild and nothing invalidated
DustStatus dust_hip_model_resample(DustHipModel* m, const DustHipModel* src, const DustHipResample* records, uint32_t n, const uint8_t* palette_map,
                                   uint32_t flags, DustHipResampleCount* counts) {
  if (!m || !src || (n && !records)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (n > DUST_HIP_MAX_RESAMPLES) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_RESAMPLES records in one call");
  if (m->ctx != src->ctx) return fail(DUST_ERR_INVALID_ARGUMENT, "the source and the destination belong to different contexts");
  DustStatus s = editable_kind(m);  // (before the records are looked at)
  if (s == DUST_OK) s = editable_kind(src);
  if (s != DUST_OK) return s;
  for (uint32_t i = 0; i < n; ++i)
    if (const char* why = dust::resample_op_refusal(records[i])) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  if (flags & ~DUST_HIP_RESAMPLE_DRY_RUN) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown resample flags");
  for (uint32_t i = 0; i < n; ++i)
    if (const char* why = dust::resample_map_refusal(records[i])) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  uint8_t map[256];  // grid byte (palette index + 1, 0 = None) -> grid byte
  map[0] = 0;
  for (uint32_t i = 0; i < 255; ++i) {
    if (palette_map && palette_map[i] > 254) return fail(DUST_ERR_INVALID_ARGUMENT, "palette_map entries must be 0..254");
    map[i + 1] = uint8_t((palette_map ? palette_map[i] : i) + 1u);
  }
  const bool dry = (flags & DUST_HIP_RESAMPLE_DRY_RUN) != 0u;
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    DustStatus s = begin_edit(m);
    if (s != DUST_OK || n == 0) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    if (!dry) invalidate_derived(es);
    std::vector<dust::DevResample> dev;
    std::vector<uint32_t> index;
    dust::live_records<dust::device_resample>(records, n, dev, index);
    const size_t live = dev.size();
    const size_t extra_bytes = live * dust::kResampleExtra * 4;
    std::vector<uint32_t> changed(counts ? n : 0u, 0u), extra(live * dust::kResampleExtra, 0u);
    const uint8_t* source = nullptr;
    if (live) {
      // (a dry run writes nothing: a model held against itself is read in place)
      if ((s = source_grid(ctx, dry ? nullptr : m, src, &source)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_aux, sizeof(map))) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, extra_bytes)) != DUST_OK) return s;
      HIP_TRY(hipMemcpyAsync(ctx->stage_aux.p, map, sizeof(map), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemsetAsync(ctx->stage_out.p, 0, extra_bytes, st));
    }
    auto launch = [&](size_t c0, dust::ResampleArgs& a) -> DustStatus {
      a.src = source;
      a.records = static_cast<const dust::DevResample*>(es.shapes.p) + c0;
      a.extra = static_cast<uint32_t*>(ctx->stage_out.p) + c0 * dust::kResampleExtra;
      a.palette_map = static_cast<const uint8_t*>(ctx->stage_aux.p);
      HIP_TRY(dust::launch_resample(a, dry, st));
      return DUST_OK;
    };
    if (dry) {
      if (live) {
        if ((s = grow(ctx, es.shapes, live * sizeof(dust::DevResample))) != DUST_OK) return s;
        if ((s = grow(ctx, es.changed, live * 4)) != DUST_OK) return s;
        HIP_TRY(hipMemcpyAsync(es.shapes.p, dev.data(), live * sizeof(dust::DevResample), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(es.changed.p, 0, live * 4, st));
        dust::CellLists lists;
        s = for_each_chunk<dust::ResampleArgs>(ctx, dev, lists, es.shape_cells, es.shape_starts, es.shape_ids, [&](size_t c0, dust::ResampleArgs& a) -> DustStatus {
          a.grid = static_cast<uint8_t*>(es.grid.p);
          a.changed = static_cast<uint32_t*>(es.changed.p) + c0;
          return launch(c0, a);
        });
        if (s != DUST_OK) return s;
        std::vector<uint32_t> would(live, 0u);
        HIP_TRY(hipMemcpyAsync(would.data(), es.changed.p, live * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(extra.data(), ctx->stage_out.p, extra_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));  // (the host vectors and lists above stay alive until the copies are done)
        if (counts)
          for (size_t k = 0; k < live; ++k) changed[index[k]] = would[k];
      }
    } else {
      if ((s = batched_edit<dust::ResampleArgs>(m, dev, index, n, counts ? changed.data() : nullptr, launch)) != DUST_OK) return s;
      if (live) HIP_TRY(hipMemcpy(extra.data(), ctx->stage_out.p, extra_bytes, hipMemcpyDeviceToHost));  // (the rebuild has waited for the stream)
    }
    if (counts) {
      for (uint32_t i = 0; i < n; ++i) counts[i] = dust::resample_count(0u, nullptr);
      for (size_t k = 0; k < live; ++k) counts[index[k]] = dust::resample_count(changed[index[k]], extra.data() + k * dust::kResampleExtra);
    }
    return DUST_OK;
  });
}

// ---- model casts (cast.hip k_cast_walk / k_cast_count): both models are only read, through their brick masks
namespace {
// The source's brick masks: its own when it is editable (dst itself included); otherwise its blocks' masks scattered into a scratch
// array -- the source is not touched. `scratch`: the context's cast_mask unless the call holds two such arrays at once
// (dust_hip_model_delta)
DustStatus cast_source_masks(DustHipContext* ctx, const DustHipModel* src, const uint64_t** src_mask, DeviceBuffer* scratch = nullptr) {
  if (src->edit) {
    *src_mask = static_cast<const uint64_t*>(src->edit->brick_mask.p);
    return DUST_OK;
  }
  DeviceBuffer& mask = scratch ? *scratch : ctx->cast_mask;
  const size_t bytes = size_t(dust::kLattice) * 8;
  DustStatus s = lazy_alloc(mask, bytes, "the cast source masks (2 MiB)");
  if (s != DUST_OK) return s;
  HIP_TRY(hipMemsetAsync(mask.p, 0, bytes, ctx->stream));
  HIP_TRY(dust::launch_cast_masks(static_cast<uint64_t*>(mask.p), static_cast<const DustHipBlock*>(src->blocks.p), src->dev.n_blocks, ctx->stream));
  *src_mask = static_cast<const uint64_t*>(mask.p);
  return DUST_OK;
}
}  // namespace

DustStatus dust_hip_model_cast(DustHipModel* m, const DustHipModel* src, const DustHipCast* casts, uint32_t n, DustHipCastHit* hits) {
  if (!m || !src || (n && (!casts || !hits))) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (n > DUST_HIP_MAX_CASTS) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_CASTS casts in one call");
  if (m->ctx != src->ctx) return fail(DUST_ERR_INVALID_ARGUMENT, "the source and the destination belong to different contexts");
  DustStatus s = editable_kind(m);  // (before the casts are looked at)
  if (s == DUST_OK) s = editable_kind(src);
  if (s != DUST_OK) return s;
  for (uint32_t i = 0; i < n; ++i) {
    const DustHipCast& c = casts[i];
    if (!dust::valid_orient(c.orient)) return fail(DUST_ERR_INVALID_ARGUMENT, "orient is not a signed axis permutation (p a permutation of 0, 1, 2; bits 9 and above zero)");
    for (int r = 0; r < 3; ++r)
      if (c.step[r] < -1 || c.step[r] > 1) return fail(DUST_ERR_INVALID_ARGUMENT, "a step component must be -1, 0 or 1");
    if (c.max_steps > DUST_HIP_CAST_MAX_STEPS) return fail(DUST_ERR_INVALID_ARGUMENT, "max_steps above DUST_HIP_CAST_MAX_STEPS");
    if (c.flags & ~DUST_HIP_CAST_WALLS) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown cast flags");
  }
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    DustStatus s = begin_edit(m);
    if (s != DUST_OK || n == 0) return s;
    hipStream_t st = ctx->stream;
    std::vector<dust::DevCast> dev;  // the casts with a sub-box
    std::vector<uint32_t> index;
    dust::live_records<dust::device_cast>(casts, n, dev, index);
    const size_t live = dev.size();
    std::vector<unsigned long long> best(live, dust::kCastNoHit);
    std::vector<dust::CastAcc> acc(live);
    if (live) {
      const uint64_t* src_mask = nullptr;
      if ((s = cast_source_masks(ctx, src, &src_mask)) != DUST_OK) return s;
      const size_t best_bytes = live * sizeof(unsigned long long);
      if ((s = grow(ctx, ctx->stage_in, live * sizeof(dust::DevCast))) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, best_bytes + live * sizeof(dust::CastAcc))) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_aux, std::max(dust::kCastChunkItems, size_t(4096)) * sizeof(dust::CastItem))) != DUST_OK) return s;
      uint8_t* out = static_cast<uint8_t*>(ctx->stage_out.p);
      HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, dev.data(), live * sizeof(dust::DevCast), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemsetAsync(out, 0xFF, best_bytes, st));                          // kCastNoHit
      HIP_TRY(hipMemsetAsync(out + best_bytes, 0, live * sizeof(dust::CastAcc), st));
      // chunks of casts, each one pair of launches: a chunk ends where its work items would pass kCastChunkItems
      std::vector<dust::CastItem> items;
      for (size_t c0 = 0; c0 < live;) {
        const size_t c1 = dust::chunk_end(dev, c0, dust::kCastChunkItems, dust::kNoRecordCap);
        if (c0 != 0) HIP_TRY(hipStreamSynchronize(st));  // the previous chunk's copy has left the host list
        dust::cast_items(dev, c0, c1, items);
        HIP_TRY(hipMemcpyAsync(ctx->stage_aux.p, items.data(), items.size() * sizeof(dust::CastItem), hipMemcpyHostToDevice, st));
        dust::CastArgs a{};
        a.src_mask = src_mask;
        a.dst_mask = static_cast<const uint64_t*>(m->edit->brick_mask.p);
        a.casts = static_cast<const dust::DevCast*>(ctx->stage_in.p) + c0;
        a.items = static_cast<const dust::CastItem*>(ctx->stage_aux.p);
        a.best = reinterpret_cast<unsigned long long*>(out) + c0;
        a.acc = reinterpret_cast<dust::CastAcc*>(out + best_bytes) + c0;
        a.n_items = uint32_t(items.size());
        HIP_TRY(dust::launch_cast(a, st));
        c0 = c1;
      }
      HIP_TRY(hipMemcpyAsync(best.data(), out, best_bytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(acc.data(), out + best_bytes, live * sizeof(dust::CastAcc), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));  // (the host vectors above stay alive until the copies are done)
    }
    for (uint32_t i = 0; i < n; ++i) hits[i] = dust::cast_hit(casts[i], dust::kCastNoHit, dust::CastAcc{});
    for (size_t j = 0; j < live; ++j) hits[index[j]] = dust::cast_hit(casts[index[j]], best[j], acc[j]);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_get_voxels(DustHipModel* m, const uint32_t* xyz, int32_t* values, uint32_t n) {
  if (!m || (n && (!xyz || !values))) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  DustStatus s = check_coordinates(xyz, n, m->dev.extent);
  if (s != DUST_OK) return s;
  return guarded([&]() -> DustStatus {
    s = begin_edit(m);
    if (s != DUST_OK || n == 0) return s;
    s = upload_batch(m, xyz, nullptr, n, false);
    if (s != DUST_OK) return s;
    dust::EditArgs a = edit_args(m, *m->edit);
    a.xyz = static_cast<const uint32_t*>(m->edit->xyz.p);
    a.values_out = static_cast<int32_t*>(m->edit->values.p);
    a.n_edits = n;
    HIP_TRY(dust::launch_edit_apply(a, true, m->ctx->stream));
    HIP_TRY(hipMemcpyAsync(values, m->edit->values.p, size_t(n) * 4, hipMemcpyDeviceToHost, m->ctx->stream));
    HIP_TRY(sync_stream(m->ctx));
    return DUST_OK;
  });
}

// ---- model islands (island.hip): label the grid's connected voxels, look labels up, move whole islands into a model of their own
static_assert(sizeof(DustHipIslandQuery) == 32 && sizeof(DustHipIsland) == 40 && sizeof(DustHipIsland) == sizeof(dust::DevIsland), "island records");

DustStatus dust_hip_model_find_islands(DustHipModel* m, const DustHipIslandQuery* q, uint32_t* n_islands, DustHipIsland* islands, uint32_t capacity) {
  if (!m || !q || !n_islands || (!islands && capacity)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipIslandQuery");
  if (q->connectivity > DUST_HIP_ISLANDS_CORNERS) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown island connectivity");
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    DustStatus s = begin_edit(m);
    if (s != DUST_OK) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    const uint32_t corners = q->connectivity == DUST_HIP_ISLANDS_CORNERS ? 1u : 0u;
    // a labelling that still stands (no edit since; detached islands only left it) is not computed again: a count-only call followed by
    // a call with room for every record labels once
    const bool relabel = !(es.labels_valid && es.labels_corners == corners);
    es.labels_valid = false;  // until this labelling is complete
    if ((s = lazy_alloc(es.labels, size_t(dust::kIslandKeys) * 4, "the island label array (64 MiB)")) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->island_mask, size_t(dust::kIslandRows) * 8)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->island_count, size_t(dust::kIslandRows) * 4)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->island_tmp, 260 * 4)) != DUST_OK) return s;
    dust::IslandArgs a{};
    a.grid = static_cast<const uint8_t*>(es.grid.p);
    a.label = static_cast<uint32_t*>(es.labels.p);
    a.root_mask = static_cast<uint64_t*>(ctx->island_mask.p);
    a.root_count = static_cast<uint32_t*>(ctx->island_count.p);
    a.scan_tmp = static_cast<uint32_t*>(ctx->island_tmp.p);
    a.corners = corners;
    for (int r = 0; r < 3; ++r) { a.anchor_lo[r] = q->anchor_lo[r]; a.anchor_hi[r] = std::min(q->anchor_hi[r], 255u); }
    HIP_TRY(dust::launch_island_label(a, relabel, st));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, a.scan_tmp + 256, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    a.capacity = std::min(total, capacity);
    if (a.capacity) {
      if ((s = grow(ctx, ctx->island_acc, size_t(a.capacity) * sizeof(dust::IslandAcc))) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->island_records, size_t(a.capacity) * sizeof(dust::DevIsland))) != DUST_OK) return s;
      a.acc = static_cast<dust::IslandAcc*>(ctx->island_acc.p);
      a.records = static_cast<dust::DevIsland*>(ctx->island_records.p);
      HIP_TRY(hipMemsetAsync(a.acc, 0, size_t(a.capacity) * sizeof(dust::IslandAcc), st));
      HIP_TRY(dust::launch_island_records(a, st));
      HIP_TRY(hipMemcpyAsync(islands, a.records, size_t(a.capacity) * sizeof(dust::DevIsland), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    es.labels_valid = true;
    es.labels_corners = corners;
    *n_islands = total;
    return DUST_OK;
  });
}

DustStatus dust_hip_model_island_of(DustHipModel* m, const uint32_t* xyz, uint32_t* keys, uint32_t n) {
  if (!m || (n && (!xyz || !keys))) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if ((s = check_coordinates(xyz, n)) != DUST_OK) return s;
  if (!m->edit || !m->edit->labels_valid) return no_labelling();
  if (n == 0) return DUST_OK;
  return lookup_call(m, xyz, keys, n, [&](const uint32_t* in, uint32_t* out, hipStream_t st) -> DustStatus {
    HIP_TRY(dust::launch_lookup(static_cast<const uint32_t*>(m->edit->labels.p), in, out, n, st));
    return DUST_OK;
  });
}

DustStatus dust_hip_model_detach_islands(DustHipModel* m, const uint32_t* keys, uint32_t n, uint32_t flags, DustHipModel** out) {
  if (!m || (n && !keys)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (flags & ~DUST_HIP_DETACH_KEEP_SOURCE) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown detach flags");
  const bool keep = (flags & DUST_HIP_DETACH_KEEP_SOURCE) != 0;
  if (keep && !out) return fail(DUST_ERR_INVALID_ARGUMENT, "DUST_HIP_DETACH_KEEP_SOURCE without a model to receive the islands does nothing");
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (n == 0) { if (out) *out = nullptr; return DUST_OK; }
  if (!m->edit || !m->edit->labels_valid) return no_labelling();
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(join_side(ctx));  // (a surfel pass on the second stream still traces the model as it is)
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    // which keys name an island: a bit per selected key, and the number of keys that name none
    if ((s = grow(ctx, ctx->island_mask, size_t(dust::kIslandRows) * 8)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->island_tmp, 260 * 4)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_in, size_t(n) * 4)) != DUST_OK) return s;
    uint32_t* bad_dev = static_cast<uint32_t*>(ctx->island_tmp.p) + 257;
    HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, keys, size_t(n) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(ctx->island_mask.p, 0, size_t(dust::kIslandRows) * 8, st));
    HIP_TRY(hipMemsetAsync(bad_dev, 0, 4, st));
    HIP_TRY(dust::launch_island_select(static_cast<const uint32_t*>(es.labels.p), static_cast<const uint32_t*>(ctx->stage_in.p), n,
                                       static_cast<uint64_t*>(ctx->island_mask.p), bad_dev, st));
    uint32_t bad = 0;
    uint32_t pal[256];
    HIP_TRY(hipMemcpyAsync(&bad, bad_dev, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pal, m->palette.p, sizeof(pal), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(DUST_ERR_INVALID_ARGUMENT, "a key does not name an island of the model's current labelling");
    // the new model: empty, editable, its grid filled by the detach kernel and then rebuilt like any edit
    struct Drop { DustHipModel* m; ~Drop() { release(m); } } fresh{nullptr};
    if (out) {
      s = dust_hip_model_create(ctx, nullptr, 0, nullptr, 0, reinterpret_cast<const uint8_t*>(pal), 8, &fresh.m);
      if (s == DUST_OK) s = make_editable(fresh.m, false);
      if (s != DUST_OK) return s;
    }
    dust::IslandDetachArgs a{};
    a.src = static_cast<uint8_t*>(es.grid.p);
    a.dst = fresh.m ? static_cast<uint8_t*>(fresh.m->edit->grid.p) : nullptr;
    a.label = static_cast<uint32_t*>(es.labels.p);
    a.selected = static_cast<const uint64_t*>(ctx->island_mask.p);
    // copy first and build the new model from the copy; the source is carved only once the voxels have somewhere to live, so a failure
    // up to there leaves it as it was
    if (fresh.m) {
      a.carve = 0u;
      HIP_TRY(dust::launch_island_detach(a, st));
      if ((s = rebuild_and_refresh(fresh.m, *fresh.m->edit)) != DUST_OK) return s;
    }
    if (!keep) {
      a.dst = nullptr;
      a.carve = 1u;
      invalidate_fields(es);
      HIP_TRY(dust::launch_island_detach(a, st));
      // (whole islands left: the labelling of the rest stands.) A failure in here is that of a shape edit's rebuild: the grid is
      // changed, the arrays are not; the new model is dropped with the error
      if ((s = rebuild_and_refresh(m, es)) != DUST_OK) { es.labels_valid = false; return s; }
    }
    if (out) *out = retain(fresh.m);  // the caller's reference (the guard drops the builder's)
    return DUST_OK;
  });
}

// ---- model floods (flood.hip): step distances from seeds through the empty or the solid voxels, kept on the device with the model
static_assert(sizeof(DustHipFloodQuery) == 40 && sizeof(DustHipFloodResult) == 32, "flood records");
static_assert(dust::kFieldNone == DUST_HIP_FLOOD_UNREACHED && dust::kFieldNone == DUST_HIP_DISTANCE_FAR, "one value means none in both fields");
DustStatus dust_hip_model_flood(DustHipModel* m, const DustHipFloodQuery* q, const uint32_t* seeds_xyz, uint32_t n_seeds, DustHipFloodResult* out) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);  // (before anything else is looked at)
  if (s != DUST_OK) return s;
  if (!q || (n_seeds && !seeds_xyz)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipFloodQuery");
  if (q->medium > DUST_HIP_FLOOD_MATERIAL) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown flood medium");
  if (q->medium == DUST_HIP_FLOOD_MATERIAL && (q->palette < 0 || q->palette > 254)) return fail(DUST_ERR_INVALID_ARGUMENT, "palette index must be 0..254");
  if (q->max_steps > DUST_HIP_FLOOD_MAX_STEPS) return fail(DUST_ERR_INVALID_ARGUMENT, "max_steps above DUST_HIP_FLOOD_MAX_STEPS");
  if (n_seeds > DUST_HIP_MAX_FLOOD_SEEDS) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_FLOOD_SEEDS seeds in one call");
  if ((s = check_coordinates(seeds_xyz, n_seeds)) != DUST_OK) return s;
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    DustStatus s = begin_edit(m);
    if (s != DUST_OK) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    es.flood.valid = false;  // until this field is complete
    if ((s = lazy_alloc(es.flood.values, size_t(dust::kLattice) * 64 * 2, "the flood field (32 MiB)")) != DUST_OK) return s;
    const size_t L = dust::kLattice;
    if ((s = grow(ctx, ctx->flood_work, (4 * L + dust::kFloodWorkWords) * 4)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_in, size_t(n_seeds) * 12)) != DUST_OK) return s;
    uint32_t* work = static_cast<uint32_t*>(ctx->flood_work.p);
    uint32_t* flag[2] = {work + dust::kFloodFlag * L, work + (dust::kFloodFlag + 1) * L};
    uint32_t* list[2] = {work + dust::kFloodList * L, work + (dust::kFloodList + 1) * L};
    uint32_t* count = work + dust::kFloodCount * L;  // three, taking turns
    dust::FloodArgs a{};
    a.grid = static_cast<const uint8_t*>(es.grid.p);
    a.field = static_cast<uint16_t*>(es.flood.values.p);
    a.medium = q->medium;
    a.byte = q->medium == DUST_HIP_FLOOD_MATERIAL ? uint32_t(q->palette) + 1u : 0u;
    a.max_steps = q->max_steps;
    bool nothing = false;  // lo > hi on an axis: nothing is passable
    for (int r = 0; r < 3; ++r) {
      a.lo[r] = q->lo[r];
      a.hi[r] = std::min(q->hi[r], 255u);
      nothing |= a.lo[r] > a.hi[r];
    }
    a.seeds = static_cast<const uint32_t*>(ctx->stage_in.p);
    a.n_seeds = nothing ? 0u : n_seeds;
    a.acc = count + dust::kFloodAcc;
    // the flags (a flood that stopped at its ceiling leaves some set), the three counts and the accumulator
    HIP_TRY(hipMemsetAsync(flag[0], 0, 2 * L * 4, st));
    HIP_TRY(hipMemsetAsync(count, 0, dust::kFloodWorkWords * 4, st));
    if (a.n_seeds) HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, seeds_xyz, size_t(n_seeds) * 12, hipMemcpyHostToDevice, st));
    a.next_list = list[0]; a.next_flag = flag[0]; a.next_count = count;
    HIP_TRY(dust::launch_flood_seed(a, st));
    uint32_t acc[dust::kFloodAccWords] = {};
    if (a.n_seeds) {
      // Passes until one wakes no brick, in batches (a pass over an empty list exits at once), and never more than max_steps + 1: after
      // pass p every voxel with steps < p is final, and no value is above max_steps
      uint32_t listed = 0;
      HIP_TRY(hipMemcpyAsync(&listed, count, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const uint32_t ceiling = q->max_steps + 1u;
      for (uint32_t pass = 0; listed != 0u && pass < ceiling;) {
        const uint32_t batch = std::min(dust::kFloodBatch, ceiling - pass);
        const uint32_t workgroups = std::min(2048u, std::max(32u, listed));  // (bricks / 4 would do for this pass; the next ones may list more)
        for (uint32_t k = 0; k < batch; ++k, ++pass) {
          a.list = list[pass & 1u]; a.flag = flag[pass & 1u]; a.count = count + pass % 3u;
          a.next_list = list[(pass + 1u) & 1u]; a.next_flag = flag[(pass + 1u) & 1u]; a.next_count = count + (pass + 1u) % 3u;
          a.zero_count = count + (pass + 2u) % 3u;
          a.first = pass == 0u ? 1u : 0u;
          HIP_TRY(dust::launch_flood_relax(a, workgroups, st));
        }
        HIP_TRY(hipMemcpyAsync(&listed, count + pass % 3u, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
      HIP_TRY(dust::launch_flood_result(a, st));
      HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));  // (the seeds have left the caller's array)
    DustHipFloodResult r{};
    r.reached = acc[0];
    if (r.reached) {
      r.farthest = acc[1]; r.seeds_used = acc[2]; r.boundary = acc[3];
      for (int k = 0; k < 3; ++k) { r.lo[k] = uint8_t(255u - acc[4 + k]); r.hi[k] = uint8_t(acc[7 + k]); }
    }
    es.flood.count = r.reached;
    for (int k = 0; k < 3; ++k) { es.flood.box.lo[k] = r.lo[k] >> 4; es.flood.box.hi[k] = r.hi[k] >> 4; }
    es.flood.valid = true;
    if (out) *out = r;
    return DUST_OK;
  });
}

DustStatus dust_hip_model_flood_at(DustHipModel* m, const uint32_t* xyz, uint16_t* steps, uint32_t n) {
  return field_at(m, &EditState::flood, no_field, xyz, steps, n);
}

DustStatus dust_hip_model_flood_paths(DustHipModel* m, const uint32_t* starts_xyz, uint32_t n, uint32_t capacity, uint32_t* keys, uint32_t* lengths) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (!lengths || (n && !starts_xyz) || (n && capacity && !keys)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if ((s = check_coordinates(starts_xyz, n)) != DUST_OK) return s;
  if (!m->edit || !m->edit->flood.valid) return no_field();
  if (n == 0) return DUST_OK;
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t slots = size_t(n) * capacity;
    if ((s = grow(ctx, ctx->stage_in, size_t(n) * 12)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_out, slots * 4)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_aux, size_t(n) * 4)) != DUST_OK) return s;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, starts_xyz, size_t(n) * 12, hipMemcpyHostToDevice, st));
    HIP_TRY(dust::launch_flood_paths(static_cast<const uint16_t*>(m->edit->flood.values.p), static_cast<const uint32_t*>(ctx->stage_in.p), n, capacity,
                                     static_cast<uint32_t*>(ctx->stage_out.p), static_cast<uint32_t*>(ctx->stage_aux.p), st));
    // the slots past a path's end stay the caller's: the device rows come back beside them and only their written part is copied over
    std::vector<uint32_t> rows(slots);
    if (slots) HIP_TRY(hipMemcpyAsync(rows.data(), ctx->stage_out.p, slots * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lengths, ctx->stage_aux.p, size_t(n) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < n && capacity; ++i)
      std::memcpy(keys + i * capacity, rows.data() + i * capacity, size_t(std::min(lengths[i], capacity)) * 4);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_flood_apply(DustHipModel* m, uint32_t max_steps, int32_t value, uint32_t* changed) {
  return field_apply(m, &EditState::flood, no_field, 0u, max_steps, value, changed);
}

// ---- model fracture (fracture.hip): every counted voxel labelled with its nearest seed, kept on the device with the model as a third
// per-voxel field; whole cells detached as islands are; the seams or the labelled voxels given a value
DustStatus dust_hip_model_fracture(DustHipModel* m, const DustHipFractureQuery* q, const DustHipFractureSeed* seeds, uint32_t n_seeds,
                                   DustHipFractureResult* result, DustHipFractureCell* cells) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);  // (before anything else is looked at)
  if (s != DUST_OK) return s;
  if (!q || (n_seeds && !seeds)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipFractureQuery");
  if (n_seeds > DUST_HIP_MAX_FRACTURE_SEEDS) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_FRACTURE_SEEDS seeds in one call");
  dust::FractureArgs a{};
  bool empty = false;
  if (const char* why = dust::device_fracture(*q, a, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  if (const char* why = dust::fracture_seeds(seeds, n_seeds)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    DustStatus s = begin_edit(m);
    if (s != DUST_OK) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    es.fracture.valid = false;  // until this labelling is complete
    if ((s = lazy_alloc(es.fracture.values, size_t(dust::kLattice) * 64 * 2, "the cell field (32 MiB)")) != DUST_OK) return s;
    // the context's scratch: the seeds; the result accumulator, the cells' accumulators and their records
    const size_t acc_bytes = dust::kFractureAccWords * 4, cell_bytes = size_t(n_seeds) * sizeof(dust::FractureAcc);
    if ((s = grow(ctx, ctx->stage_in, size_t(n_seeds) * sizeof(DustHipFractureSeed))) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_aux, acc_bytes + cell_bytes)) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_out, size_t(n_seeds) * sizeof(dust::DevFractureCell))) != DUST_OK) return s;
    a.grid = static_cast<const uint8_t*>(es.grid.p);
    a.brick_mask = static_cast<const uint64_t*>(es.brick_mask.p);  // as the last rebuild left it
    a.field = static_cast<uint16_t*>(es.fracture.values.p);
    a.seeds = static_cast<const dust::DevFractureSeed*>(ctx->stage_in.p);
    a.n_seeds = n_seeds;
    a.cull = diag_env("NO_FRACTURE_CULL") ? 0u : 1u;  // (the measurement's switch: every seed a candidate of every cell)
    a.acc = static_cast<uint32_t*>(ctx->stage_aux.p);
    a.cells = reinterpret_cast<dust::FractureAcc*>(a.acc + dust::kFractureAccWords);
    a.records = static_cast<dust::DevFractureCell*>(ctx->stage_out.p);
    const bool describe = result || cells;
    uint32_t acc[dust::kFractureAccWords] = {};
    if (empty) {
      HIP_TRY(hipMemsetAsync(a.field, 0xFF, size_t(dust::kLattice) * 64 * 2, st));  // every voxel DUST_HIP_NO_CELL
    } else {
      if (n_seeds) HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, seeds, size_t(n_seeds) * sizeof(DustHipFractureSeed), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemsetAsync(a.acc, 0, acc_bytes + (describe ? cell_bytes : 0), st));
      HIP_TRY(dust::launch_fracture_label(a, st));
      if (describe) {
        HIP_TRY(dust::launch_fracture_records(a, st));
        HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
        if (cells && n_seeds) HIP_TRY(hipMemcpyAsync(cells, a.records, size_t(n_seeds) * sizeof(dust::DevFractureCell), hipMemcpyDeviceToHost, st));
      }
    }
    HIP_TRY(hipStreamSynchronize(st));  // (the seeds have left the caller's array)
    if (empty && cells) std::fill(cells, cells + n_seeds, dust::fracture_empty_cell());
    es.fracture.count = 1;  // (an apply visits the region's cells whatever they hold)
    es.fracture.box = empty ? dust::CellBox{{0, 0, 0}, {0, 0, 0}} : a.box;
    es.fracture_seeds = n_seeds;
    es.fracture.valid = true;
    if (result) *result = dust::fracture_result(empty ? nullptr : acc);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_fracture_at(DustHipModel* m, const uint32_t* xyz, uint16_t* cells, uint32_t n) {
  return field_at(m, &EditState::fracture, no_cells, xyz, cells, n);
}

DustStatus dust_hip_model_fracture_detach(DustHipModel* m, const uint32_t* cells, uint32_t n, uint32_t flags, DustHipModel** out) {
  if (!m || (n && !cells)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (flags & ~DUST_HIP_DETACH_KEEP_SOURCE) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown detach flags");
  const bool keep = (flags & DUST_HIP_DETACH_KEEP_SOURCE) != 0;
  if (keep && !out) return fail(DUST_ERR_INVALID_ARGUMENT, "DUST_HIP_DETACH_KEEP_SOURCE without a model to receive the cells does nothing");
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (n == 0) { if (out) *out = nullptr; return DUST_OK; }
  if (!m->edit || !m->edit->fracture.valid) return no_cells();
  uint64_t selected[dust::kFractureSelectWords];
  if (const char* why = dust::fracture_selection(cells, n, m->edit->fracture_seeds, selected)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(join_side(ctx));  // (a surfel pass on the second stream still traces the model as it is)
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    if ((s = grow(ctx, ctx->stage_in, sizeof(selected))) != DUST_OK) return s;
    uint32_t pal[256];
    HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, selected, sizeof(selected), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(pal, m->palette.p, sizeof(pal), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the new model: empty, editable, its grid filled by the detach kernel and then rebuilt like any edit
    struct Drop { DustHipModel* m; ~Drop() { release(m); } } fresh{nullptr};
    if (out) {
      s = dust_hip_model_create(ctx, nullptr, 0, nullptr, 0, reinterpret_cast<const uint8_t*>(pal), 8, &fresh.m);
      if (s == DUST_OK) s = make_editable(fresh.m, false);
      if (s != DUST_OK) return s;
    }
    dust::FractureDetachArgs a{};
    a.src = static_cast<uint8_t*>(es.grid.p);
    a.dst = fresh.m ? static_cast<uint8_t*>(fresh.m->edit->grid.p) : nullptr;
    a.field = static_cast<uint16_t*>(es.fracture.values.p);
    a.selected = static_cast<const uint64_t*>(ctx->stage_in.p);
    // copy first and build the new model from the copy; the source is carved only once the voxels have somewhere to live, so a failure
    // up to there leaves it as it was
    if (fresh.m) {
      a.carve = 0u;
      HIP_TRY(dust::launch_fracture_detach(a, st));
      if ((s = rebuild_and_refresh(fresh.m, *fresh.m->edit)) != DUST_OK) return s;
    }
    if (!keep) {
      a.dst = nullptr;
      a.carve = 1u;
      invalidate_derived(es);  // (a cell's voxels left their islands: the island labelling goes with the flood and distance fields)
      HIP_TRY(dust::launch_fracture_detach(a, st));
      if ((s = rebuild_and_refresh(m, es)) != DUST_OK) return s;
      es.fracture.valid = true;  // whole cells left and their voxels answer DUST_HIP_NO_CELL: the labelling of the rest stands
    }
    if (out) *out = retain(fresh.m);  // the caller's reference (the guard drops the builder's)
    return DUST_OK;
  });
}

DustStatus dust_hip_model_fracture_apply(DustHipModel* m, uint32_t where, int32_t value, uint32_t* changed) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (const char* why = dust::fracture_apply_arguments(where, value)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  if (!m->edit || !m->edit->fracture.valid) return no_cells();
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(join_side(ctx));  // (a surfel pass on the second stream still traces the model as it is)
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    invalidate_derived(es);
    if ((s = grow(ctx, es.changed, 4)) != DUST_OK) return s;
    dust::FractureApplyArgs a{};
    a.grid = static_cast<uint8_t*>(es.grid.p);
    a.field = static_cast<const uint16_t*>(es.fracture.values.p);
    a.seams = where == DUST_HIP_FRACTURE_SEAMS ? 1u : 0u;
    a.byte = value < 0 ? 0u : uint32_t(value) + 1u;
    a.box = es.fracture.box;
    a.changed = static_cast<uint32_t*>(es.changed.p);
    uint32_t n = 0;
    HIP_TRY(hipMemsetAsync(a.changed, 0, 4, st));
    HIP_TRY(dust::launch_fracture_apply(a, st));
    HIP_TRY(hipMemcpyAsync(&n, a.changed, 4, hipMemcpyDeviceToHost, st));
    s = rebuild_and_refresh(m, es);  // synchronises; k_edit_brick_masks makes the masks again from the grid
    if (s != DUST_OK) return s;
    if (changed) *changed = n;
    return DUST_OK;
  });
}

// ---- model bodies (body.hip): mass, first and second moments per group of voxels -- the whole model, a palette index, an island of the
// standing labelling, a cell of the standing fracture. Nothing is written but the context's scratch; no rebuild
DustStatus dust_hip_model_bodies(const DustHipModel* m, const DustHipBodyQuery* q, const uint16_t* weights, uint32_t* n_bodies, DustHipBody* bodies,
                                 uint32_t capacity) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);  // (before the query is looked at)
  if (s != DUST_OK) return s;
  if (!q || !n_bodies) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipBodyQuery");
  dust::BodyArgs a{};
  bool empty = false;
  if (const char* why = dust::device_bodies(*q, a, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  if (capacity && !bodies) return fail(DUST_ERR_INVALID_ARGUMENT, "null bodies with capacity > 0");
  // (a model that is not editable holds neither a labelling nor a cell field)
  if (a.group == dust::kBodiesIslands && (!m->edit || !m->edit->labels_valid)) return no_labelling();
  if (a.group == dust::kBodiesCells && (!m->edit || !m->edit->fracture.valid)) return no_cells();
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(join_side(ctx));
    hipStream_t st = ctx->stream;
    uint32_t total = 1;
    if (a.group == dust::kBodiesMaterials) total = dust::kBodyMaterials;
    if (a.group == dust::kBodiesCells) total = m->edit->fracture_seeds;
    if (a.group == dust::kBodiesIslands) {
      // the roots, their counts and the scan are the context's, shared by its models: found again, as a repeated find_islands does
      EditState& es = *m->edit;
      if ((s = grow(ctx, ctx->island_mask, size_t(dust::kIslandRows) * 8)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->island_count, size_t(dust::kIslandRows) * 4)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->island_tmp, 260 * 4)) != DUST_OK) return s;
      dust::IslandArgs ia{};
      ia.grid = static_cast<const uint8_t*>(es.grid.p);
      ia.label = static_cast<uint32_t*>(es.labels.p);  // flat already: the pass writes no word of it
      ia.root_mask = static_cast<uint64_t*>(ctx->island_mask.p);
      ia.root_count = static_cast<uint32_t*>(ctx->island_count.p);
      ia.scan_tmp = static_cast<uint32_t*>(ctx->island_tmp.p);
      ia.corners = es.labels_corners;
      HIP_TRY(dust::launch_island_label(ia, false, st));
      HIP_TRY(hipMemcpyAsync(&total, ia.scan_tmp + 256, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      a.label = ia.label;
      a.root_mask = ia.root_mask;
      a.root_count = ia.root_count;
      a.scan_tmp = ia.scan_tmp;
    }
    a.capacity = std::min(total, capacity);
    if (a.capacity) {
      if (!empty) {
        if ((s = cast_source_masks(ctx, m, &a.brick_mask)) != DUST_OK) return s;
        // the grid only where a material is needed
        if ((weights || a.byte != 0u || a.group == dust::kBodiesMaterials) && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
        if (a.group == dust::kBodiesCells) a.field = static_cast<const uint16_t*>(m->edit->fracture.values.p);
        if (weights) {
          if ((s = grow(ctx, ctx->stage_in, dust::kBodyMaterials * sizeof(uint16_t))) != DUST_OK) return s;
          HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, weights, dust::kBodyMaterials * sizeof(uint16_t), hipMemcpyHostToDevice, st));
          a.weights = static_cast<const uint16_t*>(ctx->stage_in.p);
        }
      }
      if ((s = grow(ctx, ctx->stage_aux, size_t(a.capacity) * sizeof(dust::BodyAcc))) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, size_t(a.capacity) * sizeof(dust::BodyRecord))) != DUST_OK) return s;
      a.acc = static_cast<dust::BodyAcc*>(ctx->stage_aux.p);
      a.records = static_cast<dust::BodyRecord*>(ctx->stage_out.p);
      HIP_TRY(hipMemsetAsync(a.acc, 0, size_t(a.capacity) * sizeof(dust::BodyAcc), st));
      if (a.group == dust::kBodiesIslands) HIP_TRY(dust::launch_body_keys(a, st));
      if (!empty) HIP_TRY(dust::launch_bodies(a, st));
      HIP_TRY(dust::launch_bodies_emit(a, st));
      HIP_TRY(hipMemcpyAsync(bodies, a.records, size_t(a.capacity) * sizeof(dust::BodyRecord), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));  // (the weights have left the caller's array)
    }
    *n_bodies = total;
    return DUST_OK;
  });
}

// ---- model joints (joint.hip): one record per pair of groups -- palette indices, or the cells of the standing fracture and REST -- that
// share a voxel face. Nothing is written but the context's scratch; no rebuild. The pairs are collected in a hash table in stage_aux
// (counters in front); a table that turns out too small is doubled and the pass repeated on a cleared one
DustStatus dust_hip_model_joints(const DustHipModel* m, const DustHipJointQuery* q, uint32_t* n_joints, DustHipJoint* joints, uint32_t capacity) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);  // (before the query is looked at)
  if (s != DUST_OK) return s;
  if (!q || !n_joints) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipJointQuery");
  dust::JointArgs a{};
  bool empty = false;
  if (const char* why = dust::device_joints(*q, a, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  if (capacity && !joints) return fail(DUST_ERR_INVALID_ARGUMENT, "null joints with capacity > 0");
  // (a model that is not editable holds no cell field)
  if (a.group == dust::kJointsCells && (!m->edit || !m->edit->fracture.valid)) return no_cells();
  if (empty) { *n_joints = 0; return DUST_OK; }
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(join_side(ctx));
    hipStream_t st = ctx->stream;
    if ((s = cast_source_masks(ctx, m, &a.brick_mask)) != DUST_OK) return s;
    if (a.group == dust::kJointsMaterials && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
    if (a.group == dust::kJointsCells) a.field = static_cast<const uint16_t*>(m->edit->fracture.values.p);
    constexpr size_t head = 64;  // the counters, then the slots
    uint32_t counters[dust::kJointCounterWords] = {};
    for (a.slots_log2 = dust::joint_first_slots_log2(a.box.count());; ++a.slots_log2) {
      if (a.slots_log2 > dust::kJointMaxSlotsLog2) return fail(DUST_ERR_OUT_OF_MEMORY, "the largest joint table overflowed");  // (it cannot)
      const size_t bytes = head + (size_t(1) << a.slots_log2) * sizeof(dust::JointSlot);
      if ((s = grow(ctx, ctx->stage_aux, bytes)) != DUST_OK) return s;
      a.counters = static_cast<uint32_t*>(ctx->stage_aux.p);
      a.slots = reinterpret_cast<dust::JointSlot*>(static_cast<uint8_t*>(ctx->stage_aux.p) + head);
      HIP_TRY(hipMemsetAsync(ctx->stage_aux.p, 0, bytes, st));
      HIP_TRY(dust::launch_joints(a, st));
      HIP_TRY(hipMemcpyAsync(counters, a.counters, sizeof(counters), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (counters[dust::kJointOverflow] == 0u) break;
    }
    a.n = counters[dust::kJointClaims];
    a.capacity = std::min(a.n, capacity);
    if (a.capacity) {
      // the claimed slots as (key, slot) pairs, sorted by key: four arrays of n words and the sort's scratch in stage_in
      const size_t words = (size_t(a.n) + 63) & ~size_t(63);
      if ((s = grow(ctx, ctx->stage_in, words * 16 + dust::radix_sort_scratch_bytes(a.n))) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, size_t(a.capacity) * sizeof(dust::JointRecord))) != DUST_OK) return s;
      uint32_t* base = static_cast<uint32_t*>(ctx->stage_in.p);
      uint32_t* keys[2] = {base, base + 2 * words};
      uint32_t* vals[2] = {base + words, base + 3 * words};
      a.keys = keys[0]; a.vals = vals[0];
      a.records = static_cast<dust::JointRecord*>(ctx->stage_out.p);
      HIP_TRY(dust::launch_joints_compact(a, st));
      bool in_b = false;
      HIP_TRY(dust::radix_sort_pairs(base + 4 * words, keys[0], vals[0], keys[1], vals[1], a.n, dust::kJointKeyBits, &in_b, st));
      a.sorted_keys = keys[in_b ? 1 : 0]; a.sorted_vals = vals[in_b ? 1 : 0];
      HIP_TRY(dust::launch_joints_emit(a, st));
      HIP_TRY(hipMemcpyAsync(joints, a.records, size_t(a.capacity) * sizeof(dust::JointRecord), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    *n_joints = a.n;
    return DUST_OK;
  });
}

// ---- model distances (distance.hip): the exact distance from every voxel to the nearest target voxel, kept on the device with the model
static_assert(sizeof(DustHipDistanceQuery) == 32 && sizeof(DustHipDistanceResult) == 32 && sizeof(dust::DistanceAcc) == 16, "distance records");
DustStatus dust_hip_model_distance(DustHipModel* m, const DustHipDistanceQuery* q, DustHipDistanceResult* out) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);  // (before anything else is looked at)
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipDistanceQuery");
  if (q->target > DUST_HIP_DISTANCE_TO_MATERIAL) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown distance target");
  if (q->metric > DUST_HIP_DISTANCE_CHEBYSHEV) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown distance metric");
  if (q->flags & ~DUST_HIP_DISTANCE_WALLS) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown distance flag");
  if (q->target == DUST_HIP_DISTANCE_TO_MATERIAL && (q->palette < 0 || q->palette > 254)) return fail(DUST_ERR_INVALID_ARGUMENT, "palette index must be 0..254");
  if (q->max_radius == 0 || q->max_radius > DUST_HIP_DISTANCE_MAX_RADIUS) return fail(DUST_ERR_INVALID_ARGUMENT, "max_radius must be 1..DUST_HIP_DISTANCE_MAX_RADIUS");
  dust::DistanceArgs a{};
  if (!dust::device_distance(*q, a)) return fail(DUST_ERR_INVALID_ARGUMENT, "invalid distance query");
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    DustStatus s = begin_edit(m);
    if (s != DUST_OK) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    es.distance.valid = false;  // until this field is complete
    if ((s = lazy_alloc(es.distance.values, size_t(dust::kLattice) * 64 * 2, "the distance field (32 MiB)")) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_aux, sizeof(dust::DistanceAcc))) != DUST_OK) return s;
    a.grid = static_cast<const uint8_t*>(es.grid.p);
    a.brick_mask = static_cast<const uint64_t*>(es.brick_mask.p);
    a.field = static_cast<uint16_t*>(es.distance.values.p);
    a.acc = static_cast<dust::DistanceAcc*>(ctx->stage_aux.p);
    HIP_TRY(hipMemsetAsync(a.acc, 0, sizeof(dust::DistanceAcc), st));
    HIP_TRY(dust::launch_distance_field(a, st));
    dust::DistanceAcc acc{};
    HIP_TRY(hipMemcpyAsync(&acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const DustHipDistanceResult r = dust::distance_result(acc);
    es.distance.count = r.targets + r.near;
    es.distance.box = dust::CellBox{{0, 0, 0}, {15, 15, 15}};  // (the field keeps no bounds)
    es.distance.valid = true;
    if (out) *out = r;
    return DUST_OK;
  });
}

DustStatus dust_hip_model_distance_at(DustHipModel* m, const uint32_t* xyz, uint16_t* values, uint32_t n) {
  return field_at(m, &EditState::distance, no_distance, xyz, values, n);
}

DustStatus dust_hip_model_distance_apply(DustHipModel* m, uint32_t lo, uint32_t hi, int32_t value, uint32_t* changed) {
  return field_apply(m, &EditState::distance, no_distance, lo, hi, value, changed);
}

// ---- model reductions (reduce.hip): a new model that holds the source at 1 / 2^levels of its resolution, voted level by level
static_assert(sizeof(DustHipReduce) == 16 && sizeof(DustHipReduceResult) == 16, "reduce records");
DustStatus dust_hip_model_reduce(const DustHipModel* src, const DustHipReduce* q, DustHipModel** out, DustHipReduceResult* result) {
  if (!src || !q || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipReduce");
  DustStatus s = editable_kind(src);  // (before the query's values are looked at)
  if (s != DUST_OK) return s;
  dust::ReducePlan plan{};
  if (!dust::device_reduce(*q, plan)) return fail(DUST_ERR_INVALID_ARGUMENT, "levels must be 1..DUST_HIP_REDUCE_MAX_LEVELS, min_solid 1..8 and flags 0");
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = src->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(join_side(ctx));
    hipStream_t st = ctx->stream;
    const uint8_t* source = nullptr;
    if ((s = source_grid(ctx, nullptr, src, &source)) != DUST_OK) return s;
    if (dust::reduce_needs_scratch(plan) && (s = lazy_alloc(ctx->reduce_grid, size_t(dust::kLattice) * 64, "the reduction's second grid (16 MiB)")) != DUST_OK) return s;
    if ((s = grow(ctx, ctx->stage_aux, 8)) != DUST_OK) return s;
    uint32_t pal[256];
    HIP_TRY(hipMemcpyAsync(pal, src->palette.p, sizeof(pal), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the new model: empty, editable, its grid filled by the last level and then rebuilt like any edit
    struct Drop { DustHipModel* m; ~Drop() { release(m); } } fresh{nullptr};
    s = dust_hip_model_create(ctx, nullptr, 0, nullptr, 0, reinterpret_cast<const uint8_t*>(pal), 8, &fresh.m);
    if (s == DUST_OK) s = make_editable(fresh.m, false);
    if (s != DUST_OK) return s;
    uint32_t* counts = static_cast<uint32_t*>(ctx->stage_aux.p);  // {the source's solid voxels, the new model's}
    HIP_TRY(hipMemsetAsync(counts, 0, 8, st));
    uint8_t* grids[3] = {nullptr, static_cast<uint8_t*>(fresh.m->edit->grid.p), static_cast<uint8_t*>(ctx->reduce_grid.p)};
    for (uint32_t k = 0; k < plan.n; ++k) {
      const dust::ReduceLevel& l = plan.level[k];
      dust::ReduceArgs a{};
      a.src = l.from == dust::kReduceSource ? source : grids[l.from];
      a.dst = grids[l.to];
      a.extent = l.extent;
      a.cover_log2 = 0;
      while ((4u << a.cover_log2) < l.cover) ++a.cover_log2;
      a.min_solid = plan.min_solid;
      a.fresh = l.fresh;
      a.count_src = l.count_src ? counts : nullptr;
      a.count_dst = l.count_dst ? counts + 1 : nullptr;
      HIP_TRY(dust::launch_reduce_level(a, st));
    }
    uint32_t n[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(n, counts, 8, hipMemcpyDeviceToHost, st));
    if ((s = rebuild_and_refresh(fresh.m, *fresh.m->edit)) != DUST_OK) return s;  // synchronises
    if (result) *result = dust::reduce_result(plan, n[0], n[1]);
    *out = retain(fresh.m);  // the caller's reference (the guard drops the builder's)
    return DUST_OK;
  });
}

// ---- model censuses (census.hip k_census): the shapes of edit_shapes held against the grid, nothing written, no rebuild
DustStatus dust_hip_model_census(const DustHipModel* m, const DustHipEditShape* shapes, uint32_t n, DustHipCensus* records, uint32_t* counts) {
  if (!m || (n && !shapes)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (n > DUST_HIP_MAX_CENSUS_SHAPES) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_CENSUS_SHAPES shapes in one call");
  if (counts && n > DUST_HIP_MAX_CENSUS_TABLES) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_CENSUS_TABLES shapes in a call that asks for tables");
  DustStatus s = editable_kind(m);  // (before the shapes are looked at)
  if (s != DUST_OK) return s;
  for (uint32_t i = 0; i < n; ++i)
    if (shapes[i].kind > DUST_HIP_SHAPE_CAPSULE) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown shape kind");
  if (n == 0 || (!records && !counts)) return DUST_OK;
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    std::vector<dust::DevEditShape> dev;
    std::vector<uint32_t> index;
    dust::live_records<dust::device_census_shape>(shapes, n, dev, index);
    const size_t live = dev.size();
    std::vector<dust::CensusAcc> acc(live);
    std::vector<uint32_t> rows(counts ? live * dust::kCensusBins : 0);
    if (live) {
      HIP_TRY(hipSetDevice(ctx->device));
      HIP_TRY(join_side(ctx));
      hipStream_t st = ctx->stream;
      const uint8_t* grid = nullptr;
      if ((s = source_grid(ctx, nullptr, m, &grid)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_in, live * sizeof(dust::DevEditShape))) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, live * sizeof(dust::CensusAcc))) != DUST_OK) return s;
      if (counts && (s = grow(ctx, ctx->stage_aux, rows.size() * 4)) != DUST_OK) return s;
      dust::CensusAcc* dev_acc = static_cast<dust::CensusAcc*>(ctx->stage_out.p);
      uint32_t* dev_rows = counts ? static_cast<uint32_t*>(ctx->stage_aux.p) : nullptr;
      HIP_TRY(hipMemcpyAsync(ctx->stage_in.p, dev.data(), live * sizeof(dust::DevEditShape), hipMemcpyHostToDevice, st));
      HIP_TRY(dust::launch_census_init(dev_acc, uint32_t(live), st));
      if (counts) HIP_TRY(hipMemsetAsync(dev_rows, 0, rows.size() * 4, st));
      dust::CellLists lists;
      s = for_each_chunk<dust::CensusArgs>(ctx, dev, lists, ctx->census_cells, ctx->census_starts, ctx->census_ids, [&](size_t c0, dust::CensusArgs& a) -> DustStatus {
        a.grid = grid;
        a.shapes = static_cast<const dust::DevEditShape*>(ctx->stage_in.p) + c0;
        a.acc = dev_acc + c0;
        a.tables = counts ? dev_rows + c0 * dust::kCensusBins : nullptr;
        HIP_TRY(dust::launch_census(a, st));
        return DUST_OK;
      });
      if (s != DUST_OK) return s;
      HIP_TRY(hipMemcpyAsync(acc.data(), dev_acc, live * sizeof(dust::CensusAcc), hipMemcpyDeviceToHost, st));
      if (counts) HIP_TRY(hipMemcpyAsync(rows.data(), dev_rows, rows.size() * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));  // (the host vectors and lists above stay alive until the copies are done)
    }
    if (records) dust::census_records(acc.data(), index, n, records);
    if (counts) dust::census_tables(rows.data(), index, n, counts);
    return DUST_OK;
  });
}

// ---- model surfaces (surface.hip): the exposed faces of the solid voxels, decided from the brick masks; counted and listed without
// writing anything (k_surface_count, k_surface_list), or repainted with the rebuild of an edit behind it (k_surface_apply)
namespace {
// what both calls refuse, in the order the header gives: the model's kind before anything of the query is looked at
DustStatus surface_query(const DustHipModel* m, const DustHipSurfaceQuery* q, dust::SurfaceArgs& a, bool& empty) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  const DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipSurfaceQuery");
  if (const char* why = dust::device_surface(*q, a, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return DUST_OK;
}
}  // namespace

DustStatus dust_hip_model_surface(const DustHipModel* m, const DustHipSurfaceQuery* q, DustHipSurfaceResult* result, DustHipSurfaceVoxel* voxels,
                                  uint32_t capacity, uint32_t* counts) {
  dust::SurfaceArgs a{};
  bool empty = false;
  DustStatus s = surface_query(m, q, a, empty);
  if (s != DUST_OK) return s;
  if (capacity && !voxels) return fail(DUST_ERR_INVALID_ARGUMENT, "null voxels with capacity > 0");
  return guarded([&]() -> DustStatus {
    const size_t table_words = size_t(dust::kSurfaceFaces) * dust::kSurfaceBins;
    uint32_t acc[dust::kSurfaceAccWords] = {};
    std::vector<uint32_t> rows(counts ? table_words : 0, 0u);
    if (!empty) {
      DustHipContext* ctx = m->ctx;
      HIP_TRY(hipSetDevice(ctx->device));
      HIP_TRY(join_side(ctx));
      hipStream_t st = ctx->stream;
      if ((s = cast_source_masks(ctx, m, &a.brick_mask)) != DUST_OK) return s;
      // the grid only where a material is needed: for the count pass under a filter or with tables, for the list pass once it is
      // known that something is listed
      if ((a.byte != 0u || counts) && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, (dust::kSurfaceAccWords + table_words) * 4)) != DUST_OK) return s;
      const size_t L = dust::kLattice;
      if (capacity && (s = lazy_alloc(ctx->surface_table, (L + dust::kSurfaceScanWords) * 4, "the surface list's per-brick table (1 MiB)")) != DUST_OK) return s;
      a.acc = static_cast<uint32_t*>(ctx->stage_out.p);
      a.tables = counts ? a.acc + dust::kSurfaceAccWords : nullptr;
      a.brick_count = capacity ? static_cast<uint32_t*>(ctx->surface_table.p) : nullptr;
      HIP_TRY(hipMemsetAsync(a.acc, 0, (dust::kSurfaceAccWords + table_words) * 4, st));
      if (capacity) HIP_TRY(hipMemsetAsync(a.brick_count, 0, L * 4, st));
      HIP_TRY(dust::launch_surface_count(a, st));
      HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
      if (counts) HIP_TRY(hipMemcpyAsync(rows.data(), a.tables, table_words * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const uint32_t staged = std::min(acc[0], capacity);
      if (staged) {
        if (!a.grid && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
        if ((s = grow(ctx, ctx->stage_aux, size_t(staged) * sizeof(DustHipSurfaceVoxel))) != DUST_OK) return s;
        uint32_t* scan_tmp = a.brick_count + L;  // 256 block sums, then the total (acc[0] again)
        HIP_TRY(dust::launch_table_scan(dust::TableScan{{a.brick_count, nullptr}, {scan_tmp + 256, nullptr}, scan_tmp}, 1, st));
        a.scan_tmp = scan_tmp;
        a.voxels = static_cast<uint64_t*>(ctx->stage_aux.p);
        a.capacity = staged;
        HIP_TRY(dust::launch_surface_list(a, st));
        HIP_TRY(hipMemcpyAsync(voxels, a.voxels, size_t(staged) * sizeof(DustHipSurfaceVoxel), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    if (result) *result = dust::surface_result(empty ? nullptr : acc);
    if (counts) std::memcpy(counts, rows.data(), table_words * 4);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_surface_apply(DustHipModel* m, const DustHipSurfaceQuery* q, int32_t value, uint32_t* changed) {
  dust::SurfaceApplyArgs a{};
  bool empty = false;
  DustStatus s = surface_query(m, q, a.q, empty);
  if (s != DUST_OK) return s;
  if (value > 254) return fail(DUST_ERR_INVALID_ARGUMENT, "palette index must be 0..254 (or negative to clear the voxels)");
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    s = begin_edit(m);
    if (s != DUST_OK) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    invalidate_derived(es);
    uint32_t n = 0;
    if (!empty) {
      if ((s = grow(ctx, es.changed, 4)) != DUST_OK) return s;
      a.q.brick_mask = static_cast<const uint64_t*>(es.brick_mask.p);  // as the last rebuild left it: nothing writes it before the next
      a.grid = static_cast<uint8_t*>(es.grid.p);
      a.to = value < 0 ? 0u : uint32_t(value) + 1u;
      a.changed = static_cast<uint32_t*>(es.changed.p);
      HIP_TRY(hipMemsetAsync(a.changed, 0, 4, st));
      HIP_TRY(dust::launch_surface_apply(a, st));
      HIP_TRY(hipMemcpyAsync(&n, a.changed, 4, hipMemcpyDeviceToHost, st));
    }
    s = rebuild_and_refresh(m, es);  // synchronises; k_edit_brick_masks makes the masks again from the grid
    if (s != DUST_OK) return s;
    if (changed) *changed = n;
    return DUST_OK;
  });
}

// ---- model meshes (mesh.hip): the exposed faces merged into rectangles under mesh_rule.hpp's rule, counted (k_mesh_count) and listed
// (k_mesh_list) without writing anything. Reads the model as dust_hip_model_surface does; the per-slice table is the surface list's.
DustStatus dust_hip_model_mesh(const DustHipModel* m, const DustHipMeshQuery* q, DustHipMeshResult* result, DustHipMeshQuad* quads, uint32_t capacity) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);  // (before the query is looked at)
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipMeshQuery");
  dust::MeshArgs a{};
  bool empty = false;
  if (const char* why = dust::device_mesh(*q, a, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  if (capacity && !quads) return fail(DUST_ERR_INVALID_ARGUMENT, "null quads with capacity > 0");
  return guarded([&]() -> DustStatus {
    uint32_t acc[dust::kMeshAccWords] = {};
    if (!empty) {
      DustHipContext* ctx = m->ctx;
      HIP_TRY(hipSetDevice(ctx->device));
      HIP_TRY(join_side(ctx));
      hipStream_t st = ctx->stream;
      if ((s = cast_source_masks(ctx, m, &a.brick_mask)) != DUST_OK) return s;
      // the grid only where a material is needed: for the count pass under a filter or where runs stop at a change of material, for
      // the list pass (a record's palette) once it is known that something is listed
      if ((a.byte != 0u || !a.any_palette) && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, dust::kMeshAccWords * 4)) != DUST_OK) return s;
      const size_t L = dust::kLattice;
      static_assert(dust::kMeshScanWords <= dust::kSurfaceScanWords && dust::kMeshSlices <= dust::kLattice, "the mesh list fits the surface list's table");
      if (capacity && (s = lazy_alloc(ctx->surface_table, (L + dust::kSurfaceScanWords) * 4, "the surface and mesh lists' table (1 MiB)")) != DUST_OK) return s;
      a.acc = static_cast<uint32_t*>(ctx->stage_out.p);
      a.slice_count = capacity ? static_cast<uint32_t*>(ctx->surface_table.p) : nullptr;
      HIP_TRY(hipMemsetAsync(a.acc, 0, dust::kMeshAccWords * 4, st));
      if (capacity) HIP_TRY(hipMemsetAsync(a.slice_count, 0, L * 4, st));
      HIP_TRY(dust::launch_mesh_count(a, st));
      HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const DustHipMeshResult counted = dust::mesh_result(acc);
      const uint32_t staged = std::min(counted.quads, capacity);
      if (staged) {
        if (!a.grid && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
        if ((s = grow(ctx, ctx->stage_aux, size_t(staged) * sizeof(DustHipMeshQuad))) != DUST_OK) return s;
        uint32_t* scan_tmp = a.slice_count + L;  // 256 block sums, then the total (the quads again)
        HIP_TRY(dust::launch_table_scan(dust::TableScan{{a.slice_count, nullptr}, {scan_tmp + 256, nullptr}, scan_tmp}, 1, st));
        a.scan_tmp = scan_tmp;
        a.quads = static_cast<uint64_t*>(ctx->stage_aux.p);
        a.capacity = staged;
        HIP_TRY(dust::launch_mesh_list(a, st));
        HIP_TRY(hipMemcpyAsync(quads, a.quads, size_t(staged) * sizeof(DustHipMeshQuad), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    if (result) *result = dust::mesh_result(empty ? nullptr : acc);
    return DUST_OK;
  });
}

// ---- model boxes (boxes.hip): the solid voxels merged into boxes under boxes_rule.hpp's rule, counted (k_boxes_count, which also leaves
// every slice's D plane in the context's D volume) and listed (k_boxes_list) without writing anything to the model. Reads the model
// as dust_hip_model_mesh does; the per-slice table is the surface list's.
DustStatus dust_hip_model_boxes(const DustHipModel* m, const DustHipBoxesQuery* q, DustHipBoxesResult* result, DustHipBox* boxes, uint32_t capacity) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);  // (before the query is looked at)
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipBoxesQuery");
  dust::BoxesArgs a{};
  bool empty = false;
  if (const char* why = dust::device_boxes(*q, a, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  if (capacity && !boxes) return fail(DUST_ERR_INVALID_ARGUMENT, "null boxes with capacity > 0");
  return guarded([&]() -> DustStatus {
    uint32_t acc[dust::kBoxesAccWords] = {};
    if (!empty) {
      DustHipContext* ctx = m->ctx;
      HIP_TRY(hipSetDevice(ctx->device));
      HIP_TRY(join_side(ctx));
      hipStream_t st = ctx->stream;
      if ((s = cast_source_masks(ctx, m, &a.brick_mask)) != DUST_OK) return s;
      // the grid only where a byte is needed: for the count pass under a filter or where runs stop at a change of material, for the
      // list pass (a record's palette) once it is known that something is listed
      if ((a.byte != 0u || !a.any_palette) && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, dust::kBoxesAccWords * 4)) != DUST_OK) return s;
      if ((s = lazy_alloc(ctx->boxes_volume, dust::kBoxesVolumeWords * 4, "the boxes' D volume (2 MiB)")) != DUST_OK) return s;
      const size_t L = dust::kLattice;
      static_assert(dust::kBoxesSlices <= 1024u && dust::kBoxesSlices <= dust::kLattice, "the boxes list fits the first block of the surface list's table");
      if (capacity && (s = lazy_alloc(ctx->surface_table, (L + dust::kSurfaceScanWords) * 4, "the surface, mesh and boxes lists' table (1 MiB)")) != DUST_OK) return s;
      a.acc = static_cast<uint32_t*>(ctx->stage_out.p);
      a.dvol = static_cast<uint32_t*>(ctx->boxes_volume.p);
      a.slice_count = capacity ? static_cast<uint32_t*>(ctx->surface_table.p) : nullptr;
      HIP_TRY(hipMemsetAsync(a.acc, 0, dust::kBoxesAccWords * 4, st));
      if (capacity) HIP_TRY(hipMemsetAsync(a.slice_count, 0, L * 4, st));
      HIP_TRY(dust::launch_boxes_count(a, st));
      HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const uint32_t staged = std::min(dust::boxes_result(acc).boxes, capacity);
      if (staged) {
        if (!a.grid && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
        if ((s = grow(ctx, ctx->stage_aux, size_t(staged) * sizeof(DustHipBox))) != DUST_OK) return s;
        uint32_t* scan_tmp = a.slice_count + L;  // 256 block sums, then the total (the boxes again)
        HIP_TRY(dust::launch_table_scan(dust::TableScan{{a.slice_count, nullptr}, {scan_tmp + 256, nullptr}, scan_tmp}, 1, st));
        a.scan_tmp = scan_tmp;
        a.boxes = static_cast<uint64_t*>(ctx->stage_aux.p);
        a.capacity = staged;
        HIP_TRY(dust::launch_boxes_list(a, st));
        HIP_TRY(hipMemcpyAsync(boxes, a.boxes, size_t(staged) * sizeof(DustHipBox), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    if (result) *result = dust::boxes_result(empty ? nullptr : acc);
    return DUST_OK;
  });
}

// ---- model deltas (delta.hip): the voxels two models differ in, decided from both models' brick masks and, where only they can tell,
// their grid bytes; counted and listed without writing anything (k_delta_count, k_delta_list), or a list played onto a model with the
// rebuild of an edit behind it (k_delta_apply). The per-brick table is the surface list's.
DustStatus dust_hip_model_delta(const DustHipModel* before, const DustHipModel* after, const DustHipDeltaQuery* q, DustHipDeltaResult* result,
                                DustHipDeltaVoxel* voxels, uint32_t capacity, uint32_t* counts) {
  if (!before || !after) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(before);  // (before the query is looked at)
  if (s == DUST_OK) s = editable_kind(after);
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (before->ctx != after->ctx) return fail(DUST_ERR_INVALID_ARGUMENT, "the two models belong to different contexts");
  STRUCT_TRY(q, "DustHipDeltaQuery");
  dust::DeltaArgs a{};
  bool empty = false;
  if (const char* why = dust::device_delta(*q, a, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  if (capacity && !voxels) return fail(DUST_ERR_INVALID_ARGUMENT, "null voxels with capacity > 0");
  empty |= before == after;  // the same handle: nothing differs, and nothing is looked at
  return guarded([&]() -> DustStatus {
    const size_t table_words = size_t(dust::kDeltaRows) * dust::kDeltaBins;
    uint32_t acc[dust::kDeltaAccWords] = {};
    std::vector<uint32_t> rows(counts ? table_words : 0, 0u);
    if (!empty) {
      DustHipContext* ctx = before->ctx;
      HIP_TRY(hipSetDevice(ctx->device));
      HIP_TRY(join_side(ctx));
      hipStream_t st = ctx->stream;
      // a model that is not editable is read through the context's scratch arrays; `after` through the second pair when `before` holds the first
      DeviceBuffer* second_mask = before->edit ? nullptr : &ctx->delta_mask;
      DeviceBuffer* second_grid = before->edit ? nullptr : &ctx->delta_grid;
      auto grids = [&]() -> DustStatus {
        if (a.grid_a) return DUST_OK;
        DustStatus g = source_grid(ctx, nullptr, before, &a.grid_a);
        if (g == DUST_OK) g = source_grid(ctx, nullptr, after, &a.grid_b, second_grid);
        return g;
      };
      if ((s = cast_source_masks(ctx, before, &a.mask_a)) != DUST_OK) return s;
      if ((s = cast_source_masks(ctx, after, &a.mask_b, second_mask)) != DUST_OK) return s;
      // the grids only where a byte is needed: for the count pass to tell a repaint, under a filter or with tables, for the list pass
      // once it is known that something is listed
      if (((a.kinds & dust::kDeltaRepainted) || a.byte != 0u || counts) && (s = grids()) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, (dust::kDeltaAccWords + table_words) * 4)) != DUST_OK) return s;
      const size_t L = dust::kLattice;
      if (capacity && (s = lazy_alloc(ctx->surface_table, (L + dust::kSurfaceScanWords) * 4, "the surface, mesh and delta lists' table (1 MiB)")) != DUST_OK) return s;
      a.acc = static_cast<uint32_t*>(ctx->stage_out.p);
      a.tables = counts ? a.acc + dust::kDeltaAccWords : nullptr;
      a.brick_count = capacity ? static_cast<uint32_t*>(ctx->surface_table.p) : nullptr;
      HIP_TRY(hipMemsetAsync(a.acc, 0, (dust::kDeltaAccWords + table_words) * 4, st));
      if (capacity) HIP_TRY(hipMemsetAsync(a.brick_count, 0, L * 4, st));
      HIP_TRY(dust::launch_delta_count(a, st));
      HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
      if (counts) HIP_TRY(hipMemcpyAsync(rows.data(), a.tables, table_words * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const uint32_t staged = std::min(dust::delta_result(acc).voxels, capacity);
      if (staged) {
        if ((s = grids()) != DUST_OK) return s;
        if ((s = grow(ctx, ctx->stage_aux, size_t(staged) * sizeof(DustHipDeltaVoxel))) != DUST_OK) return s;
        uint32_t* scan_tmp = a.brick_count + L;  // 256 block sums, then the total (the listed voxels again)
        HIP_TRY(dust::launch_table_scan(dust::TableScan{{a.brick_count, nullptr}, {scan_tmp + 256, nullptr}, scan_tmp}, 1, st));
        a.scan_tmp = scan_tmp;
        a.voxels = static_cast<uint64_t*>(ctx->stage_aux.p);
        a.capacity = staged;
        HIP_TRY(dust::launch_delta_list(a, st));
        HIP_TRY(hipMemcpyAsync(voxels, a.voxels, size_t(staged) * sizeof(DustHipDeltaVoxel), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    if (result) *result = dust::delta_result(empty ? nullptr : acc);
    if (counts) std::memcpy(counts, rows.data(), table_words * 4);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_delta_apply(DustHipModel* m, const DustHipDeltaVoxel* records, uint32_t n, uint32_t flags, uint32_t* changed,
                                      uint32_t* conflicts) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);  // (before the records are looked at)
  if (s != DUST_OK) return s;
  if ((flags & ~DUST_HIP_DELTA_BACKWARD) != 0u) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown delta_apply flag");
  if (n && !records) return fail(DUST_ERR_INVALID_ARGUMENT, "null records with n > 0");
  if (n > DUST_HIP_MAX_DELTA_RECORDS) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_DELTA_RECORDS records in one call");
  return guarded([&]() -> DustStatus {
    std::vector<uint64_t> words;
    if (const char* why = dust::delta_apply_records(records, n, words)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
    DustHipContext* ctx = m->ctx;
    s = begin_edit(m);
    if (s != DUST_OK) return s;
    uint32_t counters[2] = {0u, 0u};
    if (n != 0) {
      EditState& es = *m->edit;
      hipStream_t st = ctx->stream;
      invalidate_derived(es);
      if ((s = grow(ctx, es.shapes, words.size() * 8)) != DUST_OK) return s;
      if ((s = grow(ctx, es.changed, sizeof(counters))) != DUST_OK) return s;
      dust::DeltaApplyArgs a{};
      a.records = static_cast<const uint64_t*>(es.shapes.p);
      a.n = uint32_t(words.size());
      a.backward = (flags & DUST_HIP_DELTA_BACKWARD) ? 1u : 0u;
      a.grid = static_cast<uint8_t*>(es.grid.p);
      a.counters = static_cast<uint32_t*>(es.changed.p);
      HIP_TRY(hipMemcpyAsync(es.shapes.p, words.data(), words.size() * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemsetAsync(a.counters, 0, sizeof(counters), st));
      HIP_TRY(dust::launch_delta_apply(a, st));
      HIP_TRY(hipMemcpyAsync(counters, a.counters, sizeof(counters), hipMemcpyDeviceToHost, st));
      s = rebuild_and_refresh(m, es);  // synchronises: `words` stays alive until the copy is done
      if (s != DUST_OK) return s;
    }
    if (changed) *changed = counters[0];
    if (conflicts) *conflicts = counters[1];
    return DUST_OK;
  });
}

// ---- model columns (column.hip): run `layer` of every voxel column along an axis, decided from the brick masks (and the grid bytes
// under a palette filter); mapped and counted without writing anything (k_columns), or written into with the rebuild of an edit
// behind it (k_columns_apply). Reads the model as dust_hip_model_surface does.
namespace {
// what both calls refuse, in the order the header gives: the model's kind before anything of the query is looked at
DustStatus columns_query(const DustHipModel* m, const DustHipColumnsQuery* q, dust::ColumnArgs& a, bool& empty, uint32_t& nu, uint32_t& nv) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  const DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipColumnsQuery");
  if (const char* why = dust::device_columns(*q, a, empty, nu, nv)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return DUST_OK;
}
}  // namespace

DustStatus dust_hip_model_columns(const DustHipModel* m, const DustHipColumnsQuery* q, DustHipColumnsResult* result, DustHipColumnCell* cells,
                                  uint32_t capacity, uint32_t* counts) {
  dust::ColumnArgs a{};
  bool empty = false;
  uint32_t nu = 0, nv = 0;
  DustStatus s = columns_query(m, q, a, empty, nu, nv);
  if (s != DUST_OK) return s;
  const uint32_t columns = nu * nv;
  if (cells && capacity < columns) return fail(DUST_ERR_INVALID_ARGUMENT, "capacity below the columns of the clipped region");
  return guarded([&]() -> DustStatus {
    uint32_t acc[dust::kColumnAccWords] = {};
    std::vector<uint32_t> bins(counts ? dust::kColumnBins : 0, 0u);
    if (!empty) {
      DustHipContext* ctx = m->ctx;
      HIP_TRY(hipSetDevice(ctx->device));
      HIP_TRY(join_side(ctx));
      hipStream_t st = ctx->stream;
      if ((s = cast_source_masks(ctx, m, &a.brick_mask)) != DUST_OK) return s;
      // the grid only where a byte is needed: under a filter, or for the hit voxels' palette in the map or the table
      if ((a.byte != 0u || cells || counts) && (s = source_grid(ctx, nullptr, m, &a.grid)) != DUST_OK) return s;
      if ((s = grow(ctx, ctx->stage_out, (dust::kColumnAccWords + dust::kColumnBins) * 4)) != DUST_OK) return s;
      if (cells && (s = grow(ctx, ctx->stage_aux, size_t(columns) * sizeof(DustHipColumnCell))) != DUST_OK) return s;
      a.acc = static_cast<uint32_t*>(ctx->stage_out.p);
      a.bins = counts ? a.acc + dust::kColumnAccWords : nullptr;
      a.cells = cells ? static_cast<uint32_t*>(ctx->stage_aux.p) : nullptr;
      HIP_TRY(hipMemsetAsync(a.acc, 0, (dust::kColumnAccWords + dust::kColumnBins) * 4, st));
      HIP_TRY(dust::launch_columns(a, st));
      HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
      if (counts) HIP_TRY(hipMemcpyAsync(bins.data(), a.bins, dust::kColumnBins * 4, hipMemcpyDeviceToHost, st));
      if (cells) HIP_TRY(hipMemcpyAsync(cells, a.cells, size_t(columns) * sizeof(DustHipColumnCell), hipMemcpyDeviceToHost, st));  // (every cell of the map is written)
      HIP_TRY(hipStreamSynchronize(st));
    }
    if (result) *result = dust::columns_result(empty ? nullptr : acc, nu, nv);
    if (counts) std::memcpy(counts, bins.data(), dust::kColumnBins * 4);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_columns_apply(DustHipModel* m, const DustHipColumnsQuery* q, uint32_t where, uint32_t depth, int32_t value, uint32_t* changed) {
  dust::ColumnApplyArgs a{};
  bool empty = false;
  uint32_t nu = 0, nv = 0;
  DustStatus s = columns_query(m, q, a.q, empty, nu, nv);
  if (s != DUST_OK) return s;
  if (const char* why = dust::columns_apply_arguments(where, depth, value)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    s = begin_edit(m);
    if (s != DUST_OK) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    invalidate_derived(es);
    uint32_t n = 0;
    if (!empty) {
      if ((s = grow(ctx, es.changed, 4)) != DUST_OK) return s;
      a.q.brick_mask = static_cast<const uint64_t*>(es.brick_mask.p);  // as the last rebuild left it: nothing writes it before the next
      a.q.grid = static_cast<const uint8_t*>(es.grid.p);               // (the filter's bytes: a lane reads its own column's only)
      a.grid = static_cast<uint8_t*>(es.grid.p);
      a.where = where;
      a.depth = depth;
      a.to = value < 0 ? 0u : uint32_t(value) + 1u;
      a.changed = static_cast<uint32_t*>(es.changed.p);
      HIP_TRY(hipMemsetAsync(a.changed, 0, 4, st));
      HIP_TRY(dust::launch_columns_apply(a, st));
      HIP_TRY(hipMemcpyAsync(&n, a.changed, 4, hipMemcpyDeviceToHost, st));
    }
    s = rebuild_and_refresh(m, es);  // synchronises; k_edit_brick_masks makes the masks again from the grid
    if (s != DUST_OK) return s;
    if (changed) *changed = n;
    return DUST_OK;
  });
}

// ---- model neighbourhoods (neighbour.hip): how many of a voxel's 6, 18 or 26 neighbours are solid, decided from the brick masks alone;
// counted, with what one generation of a birth / survive rule would do, without writing anything (k_neighbours), or run generation by
// generation between the model's grid and masks and the context's scratch pair, with ONE rebuild behind them (k_neighbours_step).
namespace {
// what both calls refuse, in the order the header gives: the model's kind before anything of the query is looked at
DustStatus neighbours_query(const DustHipModel* m, const DustHipNeighboursQuery* q, dust::NeighbourArgs& a, uint32_t& byte, uint32_t& majority, bool& empty) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  const DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipNeighboursQuery");
  if (const char* why = dust::device_neighbours(*q, a, byte, majority, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return DUST_OK;
}
}  // namespace

DustStatus dust_hip_model_neighbours(const DustHipModel* m, const DustHipNeighboursQuery* q, DustHipNeighboursResult* result, uint32_t* counts) {
  dust::NeighbourArgs a{};
  bool empty = false;
  uint32_t byte = 0, majority = 0;  // (an apply's)
  DustStatus s = neighbours_query(m, q, a, byte, majority, empty);
  if (s != DUST_OK) return s;
  return guarded([&]() -> DustStatus {
    uint32_t acc[dust::kNeighbourAccWords + dust::kNeighbourTableWords] = {};
    if (!empty) {
      DustHipContext* ctx = m->ctx;
      HIP_TRY(hipSetDevice(ctx->device));
      HIP_TRY(join_side(ctx));
      hipStream_t st = ctx->stream;
      if ((s = cast_source_masks(ctx, m, &a.brick_mask)) != DUST_OK) return s;  // the masks are all this call reads: no grid is made
      if ((s = grow(ctx, ctx->stage_out, sizeof(acc))) != DUST_OK) return s;
      a.acc = static_cast<uint32_t*>(ctx->stage_out.p);
      a.table = counts ? a.acc + dust::kNeighbourAccWords : nullptr;
      HIP_TRY(hipMemsetAsync(a.acc, 0, sizeof(acc), st));
      HIP_TRY(dust::launch_neighbours(a, st));
      HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    if (result) *result = dust::neighbours_result(empty ? nullptr : acc);
    if (counts) std::memcpy(counts, acc + dust::kNeighbourAccWords, dust::kNeighbourTableWords * 4);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_neighbours_apply(DustHipModel* m, const DustHipNeighboursQuery* q, uint32_t generations, DustHipNeighboursApplied* applied,
                                           uint32_t* per_generation) {
  dust::NeighbourStepArgs a{};
  bool empty = false;
  DustStatus s = neighbours_query(m, q, a.q, a.byte, a.majority, empty);
  if (s != DUST_OK) return s;
  if (const char* why = dust::neighbours_apply_arguments(generations)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    s = begin_edit(m);
    if (s != DUST_OK) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    invalidate_derived(es);
    std::vector<uint32_t> slots(empty ? 0 : dust::kNeighbourApplyWords, 0u);
    if (!empty) {
      const size_t L = dust::kLattice;
      if ((s = lazy_alloc(ctx->reduce_grid, L * 64, "the generations' second grid (16 MiB)")) != DUST_OK) return s;
      if ((s = lazy_alloc(ctx->delta_mask, L * 8, "the generations' second masks (2 MiB)")) != DUST_OK) return s;
      if ((s = grow(ctx, es.changed, slots.size() * 4)) != DUST_OK) return s;
      // The generations take turns between the model's grid and masks (0) and the scratch pair (1). Both start equal -- so outside the
      // region they stay equal, and a generation writes only the bricks the region reaches --, and the first generation reads the side
      // that makes the last one write the model's own grid.
      uint8_t* grids[2] = {static_cast<uint8_t*>(es.grid.p), static_cast<uint8_t*>(ctx->reduce_grid.p)};
      uint64_t* masks[2] = {static_cast<uint64_t*>(es.brick_mask.p), static_cast<uint64_t*>(ctx->delta_mask.p)};
      uint32_t* dev_slots = static_cast<uint32_t*>(es.changed.p);
      HIP_TRY(hipMemcpyAsync(grids[1], grids[0], L * 64, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(masks[1], masks[0], L * 8, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemsetAsync(dev_slots, 0, slots.size() * 4, st));
      for (uint32_t g = 0; g < generations; ++g) {
        const uint32_t to = (generations - 1u - g) & 1u;  // the last generation writes side 0
        a.q.brick_mask = masks[to ^ 1u];
        a.grid = grids[to ^ 1u];
        a.grid_out = grids[to];
        a.mask_out = masks[to];
        a.slot = dev_slots + size_t(g) * dust::kNeighbourSlotWords;
        a.solid = g == 0 ? dev_slots + size_t(dust::kNeighbourMaxGenerations) * dust::kNeighbourSlotWords : nullptr;
        HIP_TRY(dust::launch_neighbours_step(a, st));
        // Every kNeighbourCheckEvery generations: has one of them changed nothing? Then the model is at a fixed point, both sides hold it
        // and no later generation would change anything -- their slots stay 0, which is what they would have added.
        if ((g + 1u) % dust::kNeighbourCheckEvery == 0u && g + 1u < generations) {
          HIP_TRY(hipMemcpyAsync(slots.data(), dev_slots, size_t(g + 1u) * dust::kNeighbourSlotWords * 4, hipMemcpyDeviceToHost, st));
          HIP_TRY(hipStreamSynchronize(st));
          bool still = false;
          for (uint32_t k = 0; k <= g; ++k) still |= slots[size_t(k) * dust::kNeighbourSlotWords] + slots[size_t(k) * dust::kNeighbourSlotWords + 1] == 0u;
          if (still) break;
        }
      }
      HIP_TRY(hipMemcpyAsync(slots.data(), dev_slots, slots.size() * 4, hipMemcpyDeviceToHost, st));
    }
    s = rebuild_and_refresh(m, es);  // synchronises; k_edit_brick_masks makes the masks again from the grid
    if (s != DUST_OK) return s;
    const DustHipNeighboursApplied record =
        dust::neighbours_applied(empty ? nullptr : slots.data(), generations, empty ? 0u : slots[size_t(dust::kNeighbourMaxGenerations) * dust::kNeighbourSlotWords], per_generation);
    if (applied) *applied = record;
    return DUST_OK;
  });
}

// ---- model settling (settle.hip): loose voxels fall along an axis and slide down 45 degree slopes. What is loose is a second set of
// brick masks made from the grid bytes (k_settle_masks), so that every decision is made from masks; counted without writing anything
// (k_settle), or run step by step -- falls in place, slides between the model's grid and the context's scratch grid -- with ONE
// rebuild behind them (k_settle_fall, k_settle_slide).
namespace {
// what both calls refuse, in the order the header gives: the model's kind before anything of the query is looked at
DustStatus settle_query(const DustHipModel* m, const DustHipSettleQuery* q, dust::SettleArgs& a, dust::CellBox& box, bool& all_loose, bool& empty, uint32_t& nu,
                        uint32_t& nv) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  const DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipSettleQuery");
  if (const char* why = dust::device_settle(*q, a, box, all_loose, empty, nu, nv)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return DUST_OK;
}
// the loose voxels of every brick of `box` (and the solid ones, unless `solid` is null) from a grid's bytes
DustStatus settle_masks(const DustHipSettleQuery* q, const dust::CellBox& box, const uint8_t* grid, uint64_t* solid, uint64_t* loose, hipStream_t st) {
  dust::SettleMaskArgs ma{};
  ma.grid = grid;
  ma.brick_mask = solid;
  ma.loose_mask = loose;
  std::memcpy(ma.loose, q->loose, sizeof(ma.loose));
  ma.box = box;
  HIP_TRY(dust::launch_settle_masks(ma, st));
  return DUST_OK;
}
}  // namespace

DustStatus dust_hip_model_settle(const DustHipModel* m, const DustHipSettleQuery* q, DustHipSettleResult* result) {
  dust::SettleArgs a{};
  dust::CellBox box{};
  bool all_loose = false, empty = false;
  uint32_t nu = 0, nv = 0;
  DustStatus s = settle_query(m, q, a, box, all_loose, empty, nu, nv);
  if (s != DUST_OK) return s;
  return guarded([&]() -> DustStatus {
    uint32_t acc[dust::kSettleAccWords] = {};
    if (!empty) {
      DustHipContext* ctx = m->ctx;
      HIP_TRY(hipSetDevice(ctx->device));
      HIP_TRY(join_side(ctx));
      hipStream_t st = ctx->stream;
      if ((s = cast_source_masks(ctx, m, &a.brick_mask)) != DUST_OK) return s;
      a.loose_mask = a.brick_mask;  // every index is loose: the masks are all the call reads, no grid is made
      if (!all_loose) {
        const uint8_t* grid = nullptr;
        if ((s = source_grid(ctx, nullptr, m, &grid)) != DUST_OK) return s;
        if ((s = lazy_alloc(ctx->settle_masks, size_t(dust::kLattice) * 8 * 3, "the settle masks (6 MiB)")) != DUST_OK) return s;
        uint64_t* loose = static_cast<uint64_t*>(ctx->settle_masks.p);
        if ((s = settle_masks(q, box, grid, nullptr, loose, st)) != DUST_OK) return s;
        a.loose_mask = loose;
      }
      if ((s = grow(ctx, ctx->stage_out, sizeof(acc))) != DUST_OK) return s;
      a.acc = static_cast<uint32_t*>(ctx->stage_out.p);
      HIP_TRY(hipMemsetAsync(a.acc, 0, sizeof(acc), st));
      HIP_TRY(dust::launch_settle(a, st));
      HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    if (result) *result = dust::settle_result(empty ? nullptr : acc, nu, nv);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_settle_apply(DustHipModel* m, const DustHipSettleQuery* q, uint32_t generations, DustHipSettleApplied* applied,
                                       uint32_t* per_generation) {
  dust::SettleArgs a{};
  dust::SettleSlideArgs sl{};
  bool all_loose = false, empty = false;
  uint32_t nu = 0, nv = 0;
  DustStatus s = settle_query(m, q, a, sl.box, all_loose, empty, nu, nv);
  if (s != DUST_OK) return s;
  if (const char* why = dust::settle_apply_arguments(generations)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    s = begin_edit(m);
    if (s != DUST_OK) return s;
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    invalidate_derived(es);
    std::vector<uint32_t> slots(empty ? 0 : dust::kSettleApplyWords, 0u);
    if (!empty) {
      const size_t L = dust::kLattice;
      if (generations != 0u && (s = lazy_alloc(ctx->reduce_grid, L * 64, "the slides' second grid (16 MiB)")) != DUST_OK) return s;
      if ((s = lazy_alloc(ctx->settle_masks, L * 8 * 3, "the settle masks (6 MiB)")) != DUST_OK) return s;
      if ((s = grow(ctx, es.changed, slots.size() * 4)) != DUST_OK) return s;
      // A fall moves bytes in place; a slide reads one grid and writes the other, so the two take turns. Both start equal -- so outside
      // the region they stay equal, and a slide writes only the bricks the region reaches. Masks 0 (the model's own and the loose ones
      // beside them) are made from the grid at hand before every slide, which writes masks 1 for the fall behind it.
      uint8_t* grids[2] = {static_cast<uint8_t*>(es.grid.p), static_cast<uint8_t*>(ctx->reduce_grid.p)};
      uint64_t* solid0 = static_cast<uint64_t*>(es.brick_mask.p);
      uint64_t* loose0 = static_cast<uint64_t*>(ctx->settle_masks.p);
      uint64_t *solid1 = loose0 + L, *loose1 = loose0 + 2 * L;
      uint32_t* dev_slots = static_cast<uint32_t*>(es.changed.p);
      if (generations != 0u) HIP_TRY(hipMemcpyAsync(grids[1], grids[0], L * 64, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemsetAsync(dev_slots, 0, slots.size() * 4, st));
      for (int r = 0; r < 3; ++r) { sl.lo[r] = q->lo[r]; sl.hi[r] = q->hi[r]; }
      sl.g_axis = a.axis;
      sl.g_up = a.from_high;
      if ((s = settle_masks(q, sl.box, grids[0], nullptr, loose0, st)) != DUST_OK) return s;  // (the solid masks stand since the last rebuild)
      a.brick_mask = solid0;
      a.loose_mask = loose0;
      a.grid = grids[0];
      a.acc = dev_slots;
      HIP_TRY(dust::launch_settle_fall(a, st));
      uint32_t at = 0;  // the grid that holds the model
      for (uint32_t g = 0; g < generations; ++g) {
        uint32_t* slot = dev_slots + size_t(1u + 2u * g) * dust::kSettleAccWords;
        if ((s = settle_masks(q, sl.box, grids[at], solid0, loose0, st)) != DUST_OK) return s;
        dust::settle_slide_direction(a.axis, g, sl.d_axis, sl.d_up);
        sl.brick_mask = solid0; sl.loose_mask = loose0; sl.grid = grids[at];
        sl.grid_out = grids[at ^ 1u]; sl.mask_out = solid1; sl.loose_out = loose1;
        sl.acc = slot;
        HIP_TRY(dust::launch_settle_slide(sl, st));
        at ^= 1u;
        a.brick_mask = solid1;
        a.loose_mask = loose1;
        a.grid = grids[at];
        a.acc = slot + dust::kSettleAccWords;
        HIP_TRY(dust::launch_settle_fall(a, st));
        // Every kSettleCheckEvery generations: have four in a row moved nothing? Then the model is at rest and no later generation would
        // move anything -- their records stay 0, which is what they would have added.
        if ((g + 1u) % dust::kSettleCheckEvery == 0u && g + 1u < generations) {
          HIP_TRY(hipMemcpyAsync(slots.data(), dev_slots, size_t(1u + 2u * (g + 1u)) * dust::kSettleAccWords * 4, hipMemcpyDeviceToHost, st));
          HIP_TRY(hipStreamSynchronize(st));
          if (dust::settle_at_rest(slots.data(), g + 1u)) break;
        }
      }
      if (at != 0u) HIP_TRY(hipMemcpyAsync(grids[0], grids[1], L * 64, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(slots.data(), dev_slots, slots.size() * 4, hipMemcpyDeviceToHost, st));
    }
    s = rebuild_and_refresh(m, es);  // synchronises; k_edit_brick_masks makes the masks again from the grid
    if (s != DUST_OK) return s;
    const DustHipSettleApplied record = dust::settle_applied(empty ? nullptr : slots.data(), generations, per_generation);
    if (applied) *applied = record;
    return DUST_OK;
  });
}

// ---- model voxelisation (triangle.hip): the voxels triangles touch, on edit_shapes' path (k_edit_triangles), and the voxels whose
// centres lie inside a mesh -- the columns' crossings XORed into the context's bit volume chunk by chunk (k_fill_columns), then the
// operation on the region's inside voxels (k_fill_apply) -- with ONE rebuild behind either.
DustStatus dust_hip_model_edit_triangles(DustHipModel* m, const DustHipTriangle* triangles, uint32_t n, uint32_t* changed) {
  if (!m || (n && !triangles)) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (n > DUST_HIP_MAX_EDIT_TRIANGLES) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_EDIT_TRIANGLES triangles in one call");
  for (uint32_t i = 0; i < n; ++i) {
    if (triangles[i].op > DUST_HIP_EDIT_PLACE) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown edit op");
    if (triangles[i].op != DUST_HIP_EDIT_CARVE && (triangles[i].palette < 0 || triangles[i].palette > 254))
      return fail(DUST_ERR_INVALID_ARGUMENT, "palette index must be 0..254");
  }
  return guarded([&]() -> DustStatus {
    DustStatus s = begin_edit(m);
    if (s != DUST_OK || n == 0) return s;
    EditState& es = *m->edit;
    invalidate_derived(es);
    std::vector<dust::DevTriangle> dev;
    std::vector<uint32_t> index;
    dust::live_records<dust::device_triangle>(triangles, n, dev, index);
    return batched_edit<dust::EditTriangleArgs>(m, dev, index, n, changed, [&](size_t c0, dust::EditTriangleArgs& a) -> DustStatus {
      a.triangles = static_cast<const dust::DevTriangle*>(es.shapes.p) + c0;
      HIP_TRY(dust::launch_edit_triangles(a, m->ctx->stream));
      return DUST_OK;
    });
  });
}

DustStatus dust_hip_model_fill_mesh(DustHipModel* m, const DustHipTriangle* triangles, uint32_t n, const DustHipFillMeshQuery* q,
                                    DustHipFillMeshResult* result) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  DustStatus s = editable_kind(m);
  if (s != DUST_OK) return s;
  if (!q) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(q, "DustHipFillMeshQuery");
  if (n && !triangles) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (n > DUST_HIP_MAX_MESH_TRIANGLES) return fail(DUST_ERR_INVALID_ARGUMENT, "more than DUST_HIP_MAX_MESH_TRIANGLES triangles in one call");
  dust::FillApplyArgs a{};
  bool empty = false;
  if (const char* why = dust::device_fill_mesh(*q, a, empty)) return fail(DUST_ERR_INVALID_ARGUMENT, why);
  return guarded([&]() -> DustStatus {
    DustHipContext* ctx = m->ctx;
    s = begin_edit(m);
    if (s != DUST_OK) return s;
    if (n == 0 || empty) {  // nothing is looked at and nothing can change: no rebuild, and what is derived from the voxels stands
      if (result) *result = dust::fill_mesh_result(nullptr, 0, 0);
      return DUST_OK;
    }
    EditState& es = *m->edit;
    hipStream_t st = ctx->stream;
    invalidate_derived(es);
    uint32_t acc[dust::kFillAccWords] = {};
    uint32_t live = 0, crossing = 0;
    std::vector<dust::DevTriangle> dev;
    dust::CellLists lists;  // (the last chunk's copies read it until rebuild_and_refresh has waited for the stream)
    for (uint32_t i = 0; i < n; ++i) {
      dust::DevTriangle d{};
      bool is_live = false, is_crossing = false;
      if (dust::device_fill_triangle(triangles[i], a.lo, a.hi, d, is_live, is_crossing)) dev.push_back(d);
      live += is_live ? 1u : 0u;
      crossing += is_crossing ? 1u : 0u;
    }
    const size_t words = dust::kLattice;
    if ((s = lazy_alloc(ctx->fill_volume, words * 8, "the fill volume (2 MiB)")) != DUST_OK) return s;
    if ((s = grow(ctx, es.changed, dust::kFillAccWords * 4)) != DUST_OK) return s;
    HIP_TRY(hipMemsetAsync(ctx->fill_volume.p, 0, words * 8, st));
    if (!dev.empty()) {
      if ((s = grow(ctx, es.shapes, dev.size() * sizeof(dust::DevTriangle))) != DUST_OK) return s;
      HIP_TRY(hipMemcpyAsync(es.shapes.p, dev.data(), dev.size() * sizeof(dust::DevTriangle), hipMemcpyHostToDevice, st));
    }
    s = for_each_chunk<dust::FillColumnsArgs>(ctx, dev, lists, es.shape_cells, es.shape_starts, es.shape_ids, [&](size_t c0, dust::FillColumnsArgs& f) -> DustStatus {
      f.volume = static_cast<uint64_t*>(ctx->fill_volume.p);
      f.triangles = static_cast<const dust::DevTriangle*>(es.shapes.p) + c0;
      HIP_TRY(dust::launch_fill_columns(f, st));
      return DUST_OK;
    });
    if (s != DUST_OK) return s;
    a.grid = static_cast<uint8_t*>(es.grid.p);
    a.volume = static_cast<const uint64_t*>(ctx->fill_volume.p);
    a.acc = static_cast<uint32_t*>(es.changed.p);
    HIP_TRY(hipMemsetAsync(a.acc, 0, sizeof(acc), st));
    HIP_TRY(dust::launch_fill_apply(a, st));
    HIP_TRY(hipMemcpyAsync(acc, a.acc, sizeof(acc), hipMemcpyDeviceToHost, st));
    s = rebuild_and_refresh(m, es);  // synchronises: the host vectors above stay alive until the copies are done
    if (s != DUST_OK) return s;
    if (result) *result = dust::fill_mesh_result(acc, live, crossing);
    return DUST_OK;
  });
}

DustStatus dust_hip_model_info(const DustHipModel* m, uint32_t* n_blocks, uint64_t* n_materials) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  if (n_blocks) *n_blocks = m->dev.n_blocks;
  if (n_materials) *n_materials = m->n_materials;
  return DUST_OK;
}

DustStatus dust_hip_model_read(const DustHipModel* m, DustHipBlock* blocks, uint32_t block_capacity, uint8_t* materials, uint64_t material_capacity) {
  if (!m) return fail(DUST_ERR_INVALID_ARGUMENT, "null model");
  if ((blocks && block_capacity < m->dev.n_blocks) || (materials && material_capacity < m->n_materials))
    return fail(DUST_ERR_INVALID_ARGUMENT, "destination too small (see dust_hip_model_info)");
  HIP_TRY(hipSetDevice(m->ctx->device));
  const hipStream_t st = m->ctx->stream;
  if (blocks && m->dev.n_blocks) HIP_TRY(hipMemcpyAsync(blocks, m->blocks.p, size_t(m->dev.n_blocks) * sizeof(DustHipBlock), hipMemcpyDeviceToHost, st));
  if (materials && m->n_materials) HIP_TRY(hipMemcpyAsync(materials, m->materials.p, size_t(m->n_materials), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DUST_OK;
}

// ---- the upper levels as they stand on the device (what tests/test_gpu_hierarchy.py holds to the host build and to a witness)
static_assert(sizeof(DustHipHierarchyInfo) == 48 && sizeof(DustHipMidNode) == sizeof(dust::DevN4) && sizeof(DustHipL2Cell) == sizeof(dust::DevL2Cell) &&
              DUST_HIP_N16_BYTES == dust::kN16Bytes && DUST_HIP_N16_ROOT_BYTES == dust::kN16LdsBytes, "hierarchy records");
DustStatus dust_hip_model_read_hierarchy(const DustHipModel* m, DustHipHierarchyInfo* info, DustHipMidNode* mid, uint32_t mid_capacity,
                                         uint64_t* dense_mask, uint64_t dense_mask_capacity, uint8_t* root, uint8_t* host_root,
                                         uint8_t* l2, uint32_t l2_capacity, DustHipL2Cell* l2_cells, uint64_t l2_cell_capacity) {
  if (!m || !info) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  STRUCT_TRY(info, "DustHipHierarchyInfo");
  const uint32_t n_mid = m->n_mid, n_l2 = m->n_l2;
  if ((mid && mid_capacity < n_mid) || (dense_mask && dense_mask_capacity < uint64_t(n_mid) * 64) || (l2 && l2_capacity < n_l2) ||
      (l2_cells && l2_cell_capacity < uint64_t(n_l2) * 4096))
    return fail(DUST_ERR_INVALID_ARGUMENT, "destination too small (call with the info record alone for the sizes)");
  HIP_TRY(hipSetDevice(m->ctx->device));
  const hipStream_t st = m->ctx->stream;
  if (mid && n_mid) HIP_TRY(hipMemcpyAsync(mid, m->mid.p, size_t(n_mid) * sizeof(dust::DevN4), hipMemcpyDeviceToHost, st));
  if (dense_mask && n_mid) HIP_TRY(hipMemcpyAsync(dense_mask, m->dense_mask.p, size_t(n_mid) * 64 * 8, hipMemcpyDeviceToHost, st));
  if (root) HIP_TRY(hipMemcpyAsync(root, m->root.p, dust::kN16Bytes, hipMemcpyDeviceToHost, st));
  if (l2 && n_l2) HIP_TRY(hipMemcpyAsync(l2, m->l2.p, size_t(n_l2) * dust::kN16Bytes, hipMemcpyDeviceToHost, st));
  if (l2_cells && n_l2) HIP_TRY(hipMemcpyAsync(l2_cells, m->l2_cells.p, size_t(n_l2) * 4096 * sizeof(dust::DevL2Cell), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (host_root) std::memcpy(host_root, m->host_root.data(), dust::kN16LdsBytes);
  info->extent_log2 = m->dev.extent == 256 ? 8u : 12u;
  info->n_mid = n_mid;
  info->n_l2 = n_l2;
  std::memcpy(info->bmin, m->dev.bmin, sizeof(info->bmin));
  std::memcpy(info->bmax, m->dev.bmax, sizeof(info->bmax));
  info->reserved[0] = info->reserved[1] = 0;
  return DUST_OK;
}

}  // extern "C"
