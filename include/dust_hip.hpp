// dust_hip.hpp -- header-only C++ mirror of the reference's plugin/operator surface over the C ABI.
//
// Same names, argument meaning and error behaviour as the Rust items they stand for, so that host code
// (and the parity tests) read like the reference's own:
//   dust::Tree                 dust_vdb::Tree<hierarchy!(..)>       crates/vdb/src/tree.rs:7-124
//   dust::Tree::Accessor       dust_vdb::Accessor                   crates/vdb/src/accessor.rs:5-57
//   dust::VoxLoader::load      VoxLoader::load                      crates/vox/src/loader.rs:322-415
//   dust::VoxGeometry          VoxGeometry (+ PaletteMaterial)      crates/vox/src/geometry.rs:30-179, material.rs:9-120
//   dust::PinholeProjection    PinholeProjection                    crates/render/src/projection.rs:3-29
//   dust::Sunlight             Sunlight + bake()                    crates/render/src/pipeline/sky.rs:6-23,90-132
//   dust::ReblurSettings       ReblurSettings (the knobs this filter has)   crates/render/src/pipeline/nrd.rs:693-785
//   dust::RenderContext        what RenderPlugin::build sets up     crates/render/src/lib.rs:58-134
//   dust::Scene                TLASStore + instance vec             crates/render/src/accel_struct/tlas.rs:28-180
//   dust::StandardPipeline     StandardPipeline + GBuffer           crates/render/src/pipeline/standard.rs:51-60,222-240,881-917
// Rust `Option`/`Result` become std::optional / dust::Error exceptions; nothing throws across the C ABI itself.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "dust_hip.h"

namespace dust {

struct Error : std::runtime_error {
  DustStatus status;
  Error(DustStatus s, const std::string& m) : std::runtime_error(m), status(s) {}
};
inline void check(DustStatus s) {
  if (s != DUST_OK) throw Error(s, dust_hip_last_error());
}

using UVec3 = std::array<uint32_t, 3>;

// ----------------------------------------------------------------------------- dust_vdb
class Tree {
 public:
  // hierarchy!(4,2,2) -> Tree({4,2,2})
  explicit Tree(std::vector<uint32_t> fanout_log2) { check(dust_vdb_tree_create(fanout_log2.data(), uint32_t(fanout_log2.size()), &h_)); }
  ~Tree() { dust_vdb_tree_destroy(h_); }
  Tree(const Tree&) = delete;
  Tree& operator=(const Tree&) = delete;

  void set_value(UVec3 c, std::optional<bool> v) { check(dust_vdb_tree_set(h_, c[0], c[1], c[2], v ? (*v ? 1 : 0) : -1)); }
  std::optional<bool> get_value(UVec3 c) const {
    int32_t v;
    check(dust_vdb_tree_get(h_, c[0], c[1], c[2], &v));
    return v < 0 ? std::nullopt : std::optional<bool>(v != 0);
  }
  std::vector<UVec3> iter() const {
    size_t n = 0;
    check(dust_vdb_tree_iter(h_, nullptr, 0, &n));
    std::vector<UVec3> out(n);
    check(dust_vdb_tree_iter(h_, n ? out[0].data() : nullptr, n, &n));
    return out;
  }
  struct Leaf { UVec3 origin; uint64_t occupancy; uint32_t material_ptr; };
  std::vector<Leaf> iter_leaf() const {
    size_t n = 0;
    check(dust_vdb_tree_iter_leaf(h_, nullptr, nullptr, nullptr, 0, &n));
    std::vector<uint32_t> xyz(n * 3 + 1), mp(n + 1);
    std::vector<uint64_t> occ(n + 1);
    check(dust_vdb_tree_iter_leaf(h_, xyz.data(), occ.data(), mp.data(), n, &n));
    std::vector<Leaf> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = Leaf{{xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]}, occ[i], mp[i]};
    return out;
  }
  uint32_t meta_mask() const { uint32_t m; check(dust_vdb_tree_meta(h_, &m, nullptr)); return m; }
  uint32_t root_level() const { uint32_t l; check(dust_vdb_tree_meta(h_, nullptr, &l)); return l; }

  class Accessor {
   public:
    explicit Accessor(const Tree& t) { check(dust_vdb_accessor_create(t.h_, &h_)); }
    ~Accessor() { dust_vdb_accessor_destroy(h_); }
    Accessor(const Accessor&) = delete;
    std::optional<bool> get(UVec3 c) {
      int32_t v;
      check(dust_vdb_accessor_get(h_, c[0], c[1], c[2], &v));
      return v < 0 ? std::nullopt : std::optional<bool>(v != 0);
    }
   private:
    DustVdbAccessor* h_ = nullptr;
  };
  Accessor accessor() const { return Accessor(*this); }

 private:
  DustVdbTree* h_ = nullptr;
};

// ----------------------------------------------------------------------------- dust_render context
class RenderContext {
 public:
  explicit RenderContext(int device = -1, bool timing = false, void* stream = nullptr) {
    DustHipConfig cfg{};
    cfg.struct_size = sizeof(cfg);
    cfg.device = device;
    cfg.stream = stream;
    cfg.flags = timing ? DUST_HIP_CONTEXT_TIMING : 0;
    check(dust_hip_context_create(&cfg, &h_));
  }
  ~RenderContext() { dust_hip_context_destroy(h_); }
  RenderContext(const RenderContext&) = delete;
  void sync() { check(dust_hip_sync(h_)); }
  DustHipContext* raw() const { return h_; }
 private:
  DustHipContext* h_ = nullptr;
};

// ----------------------------------------------------------------------------- dust_vox
// VoxGeometry + PaletteMaterial of one model, resident on the device.
class VoxGeometry {
 public:
  VoxGeometry(RenderContext& ctx, const DustHipBlock* blocks, uint32_t n_blocks, const uint8_t* materials,
              uint64_t n_materials, const uint8_t* palette_rgba, uint32_t tree_extent_log2 = 8)
      : num_blocks(n_blocks) {
    check(dust_hip_model_create(ctx.raw(), blocks, n_blocks, materials, n_materials, palette_rgba, tree_extent_log2, &h_));
  }
  ~VoxGeometry() { dust_hip_model_destroy(h_); }
  VoxGeometry(const VoxGeometry&) = delete;
  DustHipModel* raw() const { return h_; }
  // VoxGeometry::set / get (geometry.rs:180-185) -- on the device copy, batched; Some(true) carries the palette index the
  // voxel is shaded with (the reference's call edits the CPU tree only and has no material to give). Scenes that instance the
  // geometry must commit() again before they render.
  void set(const std::vector<UVec3>& coords, const std::vector<std::optional<uint8_t>>& palette_index) {
    std::vector<uint32_t> xyz;
    std::vector<int32_t> val;
    for (size_t i = 0; i < coords.size(); ++i) {
      xyz.insert(xyz.end(), coords[i].begin(), coords[i].end());
      val.push_back(palette_index[i] ? int32_t(*palette_index[i]) : -1);
    }
    check(dust_hip_model_set_voxels(h_, xyz.data(), val.data(), uint32_t(val.size())));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
  }
  void set(UVec3 c, std::optional<uint8_t> palette_index) { set(std::vector<UVec3>{c}, {palette_index}); }
  // Shape edits (dust_hip_model_edit_shapes): boxes, spheres and capsules in tree coordinates, carved, filled, painted or placed in
  // array order; returns, per shape, the voxels whose value it changed. Scenes that instance the geometry must commit() again.
  std::vector<uint32_t> edit_shapes(const std::vector<DustHipEditShape>& shapes) {
    std::vector<uint32_t> changed(shapes.size());
    check(dust_hip_model_edit_shapes(h_, shapes.data(), uint32_t(shapes.size()), changed.data()));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  // Model islands (dust_hip_model_find_islands / island_of / detach_islands): every connected set of solid voxels in ascending key
  // order; the key of the island a voxel belongs to (DUST_HIP_NO_ISLAND where it is empty); and the named islands moved into a
  // geometry of their own, at the same tree coordinates -- or only removed with want_geometry = false (nullptr comes back, as it
  // does for no keys). Unless DUST_HIP_DETACH_KEEP_SOURCE is given, scenes that instance this geometry must commit() again.
  std::vector<DustHipIsland> find_islands(DustHipIslandQuery query) {
    query.struct_size = sizeof(query);
    uint32_t n = 0;
    check(dust_hip_model_find_islands(h_, &query, &n, nullptr, 0));  // labels and counts
    std::vector<DustHipIsland> islands(n);                          // (the second call keeps that labelling: it only describes)
    if (n) check(dust_hip_model_find_islands(h_, &query, &n, islands.data(), uint32_t(islands.size())));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return islands;
  }
  std::vector<uint32_t> island_of(const std::vector<UVec3>& coords) {
    std::vector<uint32_t> xyz, keys(coords.size());
    for (const UVec3& c : coords) xyz.insert(xyz.end(), c.begin(), c.end());
    check(dust_hip_model_island_of(h_, xyz.data(), keys.data(), uint32_t(keys.size())));
    return keys;
  }
  std::unique_ptr<VoxGeometry> detach_islands(const std::vector<uint32_t>& keys, uint32_t flags = 0, bool want_geometry = true) {
    DustHipModel* piece = nullptr;
    check(dust_hip_model_detach_islands(h_, keys.data(), uint32_t(keys.size()), flags, want_geometry ? &piece : nullptr));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return piece ? std::unique_ptr<VoxGeometry>(new VoxGeometry(piece)) : nullptr;
  }
  // Model stamps (dust_hip_model_stamp): the voxels of `source` (which may be this geometry) pasted into this one, rotated or mirrored,
  // in array order; palette_map, if given, renames the source's palette indices. Returns, per stamp, the voxels whose value it
  // changed. The source is not modified; scenes that instance this geometry must commit() again.
  std::vector<uint32_t> stamp(const VoxGeometry& source, const std::vector<DustHipStamp>& stamps, const std::array<uint8_t, 255>* palette_map = nullptr) {
    std::vector<uint32_t> changed(stamps.size());
    check(dust_hip_model_stamp(h_, source.h_, stamps.data(), uint32_t(stamps.size()), palette_map ? palette_map->data() : nullptr, changed.data()));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  // Model resampling (dust_hip_model_resample): stamp() under any rotation, scale or shear -- each record's fixed-point inverse map takes
  // a destination voxel's centre to the source voxel it reads; voxels that land outside the record's source sub-box keep their value.
  // Returns changed, covered, solid and blocked per record. dry_run: nothing is written, every record is counted against this
  // geometry as it stands (blocked == 0: the piece fits).
  std::vector<DustHipResampleCount> resample(const VoxGeometry& source, const std::vector<DustHipResample>& records,
                                             const std::array<uint8_t, 255>* palette_map = nullptr, bool dry_run = false) {
    std::vector<DustHipResampleCount> counts(records.size());
    check(dust_hip_model_resample(h_, source.h_, records.data(), uint32_t(records.size()), palette_map ? palette_map->data() : nullptr,
                                  dry_run ? DUST_HIP_RESAMPLE_DRY_RUN : 0u, counts.data()));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return counts;
  }
  // Model casts (dust_hip_model_cast): how far pieces of `source` (which may be this geometry) move inside this one before a voxel of
  // them is blocked, each cast on its own: hits[i].steps free steps (the piece rests at offset + steps * step, ready for stamp()),
  // flags, contacts and the first contact. Both geometries are only read (this one is moved into its editable form by the first call).
  std::vector<DustHipCastHit> cast(const VoxGeometry& source, const std::vector<DustHipCast>& casts) {
    std::vector<DustHipCastHit> hits(casts.size());
    check(dust_hip_model_cast(h_, source.h_, casts.data(), uint32_t(casts.size()), hits.data()));
    return hits;
  }
  // Model floods (dust_hip_model_flood / flood_at / flood_paths / flood_apply): step distances from the seeds through the query's medium
  // (empty voxels, solid voxels, or one material), kept on the device until the next edit; the distances at coordinates
  // (DUST_HIP_FLOOD_UNREACHED where the flood did not get); per start, the first `capacity` voxels of its way down to a seed as
  // x << 16 | y << 8 | z keys (empty for an unreached start; capacity 2: the next step); and every reached voxel within max_steps
  // given a palette index (nullopt: None), after which scenes that instance this geometry must commit() again.
  DustHipFloodResult flood(DustHipFloodQuery query, const std::vector<UVec3>& seeds) {
    query.struct_size = sizeof(query);
    std::vector<uint32_t> xyz;
    for (const UVec3& c : seeds) xyz.insert(xyz.end(), c.begin(), c.end());
    DustHipFloodResult result{};
    check(dust_hip_model_flood(h_, &query, xyz.data(), uint32_t(seeds.size()), &result));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return result;
  }
  std::vector<uint16_t> flood_at(const std::vector<UVec3>& coords) {
    std::vector<uint32_t> xyz;
    std::vector<uint16_t> steps(coords.size());
    for (const UVec3& c : coords) xyz.insert(xyz.end(), c.begin(), c.end());
    check(dust_hip_model_flood_at(h_, xyz.data(), steps.data(), uint32_t(steps.size())));
    return steps;
  }
  std::vector<std::vector<uint32_t>> flood_paths(const std::vector<UVec3>& starts, uint32_t capacity) {
    std::vector<uint32_t> xyz, keys(starts.size() * size_t(capacity)), lengths(starts.size());
    for (const UVec3& c : starts) xyz.insert(xyz.end(), c.begin(), c.end());
    check(dust_hip_model_flood_paths(h_, xyz.data(), uint32_t(starts.size()), capacity, keys.data(), lengths.data()));
    std::vector<std::vector<uint32_t>> paths(starts.size());
    for (size_t i = 0; i < starts.size(); ++i)
      paths[i].assign(keys.begin() + i * capacity, keys.begin() + i * capacity + (lengths[i] < capacity ? lengths[i] : capacity));
    return paths;
  }
  uint32_t flood_apply(std::optional<uint8_t> palette_index, uint32_t max_steps = 0xFFFFFFFFu) {
    uint32_t changed = 0;
    check(dust_hip_model_flood_apply(h_, max_steps, palette_index ? int32_t(*palette_index) : -1, &changed));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  // Model distances (dust_hip_model_distance / distance_at / distance_apply): the exact distance from every voxel to the nearest
  // target of the query (solid voxels, empty voxels, or one material) -- squared under DUST_HIP_DISTANCE_EUCLIDEAN --, kept on the
  // device until the next edit; the values at coordinates (DUST_HIP_DISTANCE_FAR beyond the radius); and every voxel whose value lies
  // in lo..hi given a palette index (nullopt: None), after which scenes that instance this geometry must commit() again.
  DustHipDistanceResult distance(DustHipDistanceQuery query) {
    query.struct_size = sizeof(query);
    DustHipDistanceResult result{};
    check(dust_hip_model_distance(h_, &query, &result));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return result;
  }
  std::vector<uint16_t> distance_at(const std::vector<UVec3>& coords) {
    std::vector<uint32_t> xyz;
    std::vector<uint16_t> values(coords.size());
    for (const UVec3& c : coords) xyz.insert(xyz.end(), c.begin(), c.end());
    check(dust_hip_model_distance_at(h_, xyz.data(), values.data(), uint32_t(values.size())));
    return values;
  }
  uint32_t distance_apply(std::optional<uint8_t> palette_index, uint32_t lo = 1, uint32_t hi = 0xFFFFFFFFu) {
    uint32_t changed = 0;
    check(dust_hip_model_distance_apply(h_, lo, hi, palette_index ? int32_t(*palette_index) : -1, &changed));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  // Model reductions (dust_hip_model_reduce): a coarser copy of this geometry as it stands on the device, halved `levels` times, a
  // coarse voxel solid when at least min_solid of its eight children are and carrying the palette index most of them carry. The copy
  // is a geometry of its own in [0, 256 >> levels)^3 (spawn it with lod_transform); this one is only read. `result`, if given,
  // receives the voxel counts and the extent.
  std::unique_ptr<VoxGeometry> reduce(uint32_t levels = 1, uint32_t min_solid = 1, DustHipReduceResult* result = nullptr) const {
    DustHipReduce query{};
    query.struct_size = sizeof(query);
    query.levels = levels;
    query.min_solid = min_solid;
    DustHipModel* coarse = nullptr;
    check(dust_hip_model_reduce(h_, &query, &coarse, result));
    return std::unique_ptr<VoxGeometry>(new VoxGeometry(coarse));
  }
  // Model censuses (dust_hip_model_census): what the voxels inside edit_shapes' shapes hold, each shape counted on its own against
  // the geometry as it stands on the device; nothing changes (op and palette are ignored: ask first, carve after). Returns one record
  // per shape; `counts`, if given, receives DUST_HIP_CENSUS_BINS counters per shape: [0] the covered voxels that hold None, [1 + p] those
  // that hold palette index p (at most DUST_HIP_MAX_CENSUS_TABLES shapes then).
  std::vector<DustHipCensus> census(const std::vector<DustHipEditShape>& shapes, std::vector<uint32_t>* counts = nullptr) const {
    std::vector<DustHipCensus> records(shapes.size());
    if (counts) counts->assign(shapes.size() * size_t(DUST_HIP_CENSUS_BINS), 0u);
    check(dust_hip_model_census(h_, shapes.data(), uint32_t(shapes.size()), records.data(), counts ? counts->data() : nullptr));
    return records;
  }
  // Model surfaces (dust_hip_model_surface / surface_apply): the solid voxels with an exposed face among query.faces inside the
  // query's region -- counted into the result, listed (every one of them, in the order of the blocks: two calls, one to count), and per
  // direction and palette index into `counts` (6 * DUST_HIP_SURFACE_BINS), if given. Only reads. surface_apply gives every listed
  // voxel a palette index (nullopt: None -- exactly one layer is peeled); scenes that instance this geometry must commit() again.
  std::vector<DustHipSurfaceVoxel> surface(DustHipSurfaceQuery query, DustHipSurfaceResult* result = nullptr, std::vector<uint32_t>* counts = nullptr) const {
    query.struct_size = sizeof(query);
    DustHipSurfaceResult r{};
    check(dust_hip_model_surface(h_, &query, &r, nullptr, 0, nullptr));
    std::vector<DustHipSurfaceVoxel> voxels(r.voxels);
    if (counts) counts->assign(6 * size_t(DUST_HIP_SURFACE_BINS), 0u);
    check(dust_hip_model_surface(h_, &query, &r, voxels.data(), uint32_t(voxels.size()), counts ? counts->data() : nullptr));
    if (result) *result = r;
    return voxels;
  }
  uint32_t surface_apply(DustHipSurfaceQuery query, std::optional<uint8_t> palette_index) {
    query.struct_size = sizeof(query);
    uint32_t changed = 0;
    check(dust_hip_model_surface_apply(h_, &query, palette_index ? int32_t(*palette_index) : -1, &changed));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  // Model meshes (dust_hip_model_mesh): the exposed faces among query.faces inside the query's region merged into axis-aligned
  // rectangles under the header's canonical rule (not the minimum-count greedy mesh) -- every quad, in ascending (face, slice, v0, u0):
  // two calls, one to count. Only reads.
  std::vector<DustHipMeshQuad> mesh(DustHipMeshQuery query, DustHipMeshResult* result = nullptr) const {
    query.struct_size = sizeof(query);
    DustHipMeshResult r{};
    check(dust_hip_model_mesh(h_, &query, &r, nullptr, 0));
    std::vector<DustHipMeshQuad> quads(r.quads);
    check(dust_hip_model_mesh(h_, &query, &r, quads.data(), uint32_t(quads.size())));
    if (result) *result = r;
    return quads;
  }
  // Model boxes (dust_hip_model_boxes): the solid voxels inside the query's region merged into axis-aligned boxes under the header's
  // canonical rule (not the minimum-count decomposition) -- every box, in ascending (slice, v0, u0) of query.axis: two calls, one to
  // count. Only reads.
  std::vector<DustHipBox> boxes(DustHipBoxesQuery query, DustHipBoxesResult* result = nullptr) const {
    query.struct_size = sizeof(query);
    DustHipBoxesResult r{};
    check(dust_hip_model_boxes(h_, &query, &r, nullptr, 0));
    std::vector<DustHipBox> boxes(r.boxes);
    check(dust_hip_model_boxes(h_, &query, &r, boxes.data(), uint32_t(boxes.size())));
    if (result) *result = r;
    return boxes;
  }
  // Model deltas (dust_hip_model_delta / delta_apply): the voxels in which `after` differs from this geometry, of the kinds among
  // query.kinds inside the query's region -- counted into the result, listed (every one of them, in the order of the blocks: two calls,
  // one to count), and per value before and after into `counts` (2 * DUST_HIP_DELTA_BINS), if given. Only reads both. delta_apply plays
  // such a list onto this geometry, backwards on request; `conflicts` receives the records whose voxel was not in the state the list
  // assumes. Scenes that instance this geometry must commit() again.
  std::vector<DustHipDeltaVoxel> delta(const VoxGeometry& after, DustHipDeltaQuery query, DustHipDeltaResult* result = nullptr,
                                       std::vector<uint32_t>* counts = nullptr) const {
    query.struct_size = sizeof(query);
    DustHipDeltaResult r{};
    check(dust_hip_model_delta(h_, after.h_, &query, &r, nullptr, 0, nullptr));
    std::vector<DustHipDeltaVoxel> voxels(r.voxels);
    if (counts) counts->assign(2 * size_t(DUST_HIP_DELTA_BINS), 0u);
    check(dust_hip_model_delta(h_, after.h_, &query, &r, voxels.data(), uint32_t(voxels.size()), counts ? counts->data() : nullptr));
    if (result) *result = r;
    return voxels;
  }
  uint32_t delta_apply(const std::vector<DustHipDeltaVoxel>& records, bool backward = false, uint32_t* conflicts = nullptr) {
    uint32_t changed = 0;
    check(dust_hip_model_delta_apply(h_, records.data(), uint32_t(records.size()), backward ? DUST_HIP_DELTA_BACKWARD : 0u, &changed, conflicts));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  // Model columns (dust_hip_model_columns / columns_apply): this geometry seen from the ONE side query.face, column by column inside
  // the query's region -- run query.layer of every column as a map, row-major [v][u] (result.columns cells; the result says how many
  // columns have the layer, how deep they lie, which is nearest and farthest), and the hit columns per palette index into `counts`
  // (DUST_HIP_COLUMNS_BINS), if given. Only reads. columns_apply writes `depth` voxels of every hit column's run
  // (DUST_HIP_COLUMNS_RUN) or of the gap in front of it (DUST_HIP_COLUMNS_GAP) with a palette index (nullopt: None); scenes that
  // instance this geometry must commit() again.
  std::vector<DustHipColumnCell> columns(DustHipColumnsQuery query, DustHipColumnsResult* result = nullptr, std::vector<uint32_t>* counts = nullptr) const {
    query.struct_size = sizeof(query);
    DustHipColumnsResult r{};
    check(dust_hip_model_columns(h_, &query, &r, nullptr, 0, nullptr));
    std::vector<DustHipColumnCell> cells(r.columns);
    if (counts) counts->assign(size_t(DUST_HIP_COLUMNS_BINS), 0u);
    check(dust_hip_model_columns(h_, &query, &r, cells.empty() ? nullptr : cells.data(), uint32_t(cells.size()), counts ? counts->data() : nullptr));
    if (result) *result = r;
    return cells;
  }
  uint32_t columns_apply(DustHipColumnsQuery query, uint32_t where, uint32_t depth, std::optional<uint8_t> palette_index) {
    query.struct_size = sizeof(query);
    uint32_t changed = 0;
    check(dust_hip_model_columns_apply(h_, &query, where, depth, palette_index ? int32_t(*palette_index) : -1, &changed));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  // Model neighbourhoods (dust_hip_model_neighbours / neighbours_apply): how many of the 6, 18 or 26 neighbours of the voxels inside
  // the query's region are solid -- the result says what ONE generation of the query's birth / survive masks would do, `counts`
  // (2 * DUST_HIP_NEIGHBOURS_BINS: the empty row, then the solid row), if given, is the histogram. Only reads, and needs no grid.
  // neighbours_apply runs `generations` synchronous generations of the rule and rebuilds once; per_generation, if given, receives the
  // born and the died of every generation; scenes that instance this geometry must commit() again.
  DustHipNeighboursResult neighbours(DustHipNeighboursQuery query, std::vector<uint32_t>* counts = nullptr) const {
    query.struct_size = sizeof(query);
    DustHipNeighboursResult r{};
    if (counts) counts->assign(size_t(2) * DUST_HIP_NEIGHBOURS_BINS, 0u);
    check(dust_hip_model_neighbours(h_, &query, &r, counts ? counts->data() : nullptr));
    return r;
  }
  DustHipNeighboursApplied neighbours_apply(DustHipNeighboursQuery query, uint32_t generations = 1, std::vector<uint32_t>* per_generation = nullptr) {
    query.struct_size = sizeof(query);
    DustHipNeighboursApplied applied{};
    if (per_generation) per_generation->assign(size_t(2) * generations, 0u);
    check(dust_hip_model_neighbours_apply(h_, &query, generations, &applied, per_generation && generations ? per_generation->data() : nullptr));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return applied;
  }
  // Model settling (dust_hip_model_settle / settle_apply): the loose voxels of the query's region -- those whose palette index has its
  // bit in query.loose -- fall toward query.toward. settle says what ONE fall would do and only reads; settle_apply lets them fall,
  // runs `generations` generations of a 45 degree slide and a fall, and rebuilds once; per_generation, if given, receives the slid and
  // the fell of every generation; scenes that instance this geometry must commit() again.
  DustHipSettleResult settle(DustHipSettleQuery query) const {
    query.struct_size = sizeof(query);
    DustHipSettleResult r{};
    check(dust_hip_model_settle(h_, &query, &r));
    return r;
  }
  DustHipSettleApplied settle_apply(DustHipSettleQuery query, uint32_t generations = 0, std::vector<uint32_t>* per_generation = nullptr) {
    query.struct_size = sizeof(query);
    DustHipSettleApplied applied{};
    if (per_generation) per_generation->assign(size_t(2) * generations, 0u);
    check(dust_hip_model_settle_apply(h_, &query, generations, &applied, per_generation && generations ? per_generation->data() : nullptr));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return applied;
  }
  // Model voxelisation (dust_hip_model_edit_triangles / fill_mesh): triangles with integer vertices in 1/256 voxel of tree coordinates.
  // edit_triangles carves, fills, paints or places the voxels each triangle touches, in array order, and returns per triangle the voxels
  // whose value it changed; fill_mesh applies query.op / query.palette to the voxels of the query's region whose centres lie inside the
  // mesh (the parity of the triangles crossed above the centre). Both are exact on integers; scenes that instance this geometry must
  // commit() again.
  std::vector<uint32_t> edit_triangles(const std::vector<DustHipTriangle>& triangles) {
    std::vector<uint32_t> changed(triangles.size());
    check(dust_hip_model_edit_triangles(h_, triangles.data(), uint32_t(triangles.size()), changed.data()));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  DustHipFillMeshResult fill_mesh(const std::vector<DustHipTriangle>& triangles, DustHipFillMeshQuery query) {
    query.struct_size = sizeof(query);
    DustHipFillMeshResult result{};
    check(dust_hip_model_fill_mesh(h_, triangles.data(), uint32_t(triangles.size()), &query, &result));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return result;
  }
  // Model fracture (dust_hip_model_fracture / fracture_at / fracture_detach / fracture_apply): every counted voxel of the query's
  // region labelled with the index of its nearest seed (ties to the lowest index), the labels kept on the device until the next edit;
  // the cell of each coordinate (DUST_HIP_NO_CELL where it has none); the union of the named cells moved into a geometry of its own --
  // copied under DUST_HIP_DETACH_KEEP_SOURCE, only removed with want_geometry = false; and the seams or all labelled voxels given a
  // palette index (nullopt: None). For chunks: one fracture, a KEEP_SOURCE detach per piece, then one deleting detach of all of them.
  struct Fractured { DustHipFractureResult result; std::vector<DustHipFractureCell> cells; };
  Fractured fracture(DustHipFractureQuery query, const std::vector<DustHipFractureSeed>& seeds) {
    query.struct_size = sizeof(query);
    Fractured out{};
    out.cells.resize(seeds.size());
    check(dust_hip_model_fracture(h_, &query, seeds.data(), uint32_t(seeds.size()), &out.result, out.cells.data()));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return out;
  }
  std::vector<uint16_t> fracture_at(const std::vector<UVec3>& coords) {
    std::vector<uint32_t> xyz;
    std::vector<uint16_t> cells(coords.size());
    for (const UVec3& c : coords) xyz.insert(xyz.end(), c.begin(), c.end());
    check(dust_hip_model_fracture_at(h_, xyz.data(), cells.data(), uint32_t(cells.size())));
    return cells;
  }
  std::unique_ptr<VoxGeometry> fracture_detach(const std::vector<uint32_t>& cells, uint32_t flags = 0, bool want_geometry = true) {
    DustHipModel* piece = nullptr;
    check(dust_hip_model_fracture_detach(h_, cells.data(), uint32_t(cells.size()), flags, want_geometry ? &piece : nullptr));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return piece ? std::unique_ptr<VoxGeometry>(new VoxGeometry(piece)) : nullptr;
  }
  uint32_t fracture_apply(uint32_t where, std::optional<uint8_t> palette_index) {
    uint32_t changed = 0;
    check(dust_hip_model_fracture_apply(h_, where, palette_index ? int32_t(*palette_index) : -1, &changed));
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
    return changed;
  }
  // Model bodies (dust_hip_model_bodies): mass, first and second moments per group of the query's kind -- the whole geometry, a palette
  // index, an island of the standing labelling, a cell of the standing fracture -- with a weight per palette index (255 entries;
  // nullptr: every voxel weighs 1). Every record, in key order: two calls, one to count. Only reads.
  std::vector<DustHipBody> bodies(DustHipBodyQuery query, const uint16_t* weights = nullptr) const {
    query.struct_size = sizeof(query);
    uint32_t n = 0;
    check(dust_hip_model_bodies(h_, &query, weights, &n, nullptr, 0));
    std::vector<DustHipBody> out(n);
    check(dust_hip_model_bodies(h_, &query, weights, &n, out.data(), uint32_t(out.size())));
    if (n < out.size()) out.resize(n);
    return out;
  }
  // Model joints (dust_hip_model_joints): one record per pair of groups -- palette indices, or the cells of the standing fracture with
  // DUST_HIP_JOINT_REST for the solid voxels beyond it -- that share a voxel face: the faces, their directions from a to b, the bounds
  // and sums of their centres in half voxels. Every record, in ascending (a, b): two calls, one to count. Only reads.
  std::vector<DustHipJoint> joints(DustHipJointQuery query) const {
    query.struct_size = sizeof(query);
    uint32_t n = 0;
    check(dust_hip_model_joints(h_, &query, &n, nullptr, 0));
    std::vector<DustHipJoint> out(n);
    check(dust_hip_model_joints(h_, &query, &n, out.data(), uint32_t(out.size())));
    if (n < out.size()) out.resize(n);
    return out;
  }
  // the obj_to_world of an instance of reduce(levels)'s geometry that stands where an instance of this one with `obj_to_world_3x4`
  // stands: columns 0..2 scaled by 2^levels, the translation unchanged
  static std::array<float, 12> lod_transform(const float obj_to_world_3x4[12], uint32_t levels) {
    std::array<float, 12> m{};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) m[size_t(r * 4 + c)] = obj_to_world_3x4[r * 4 + c] * float(1u << levels);
      m[size_t(r * 4 + 3)] = obj_to_world_3x4[r * 4 + 3];
    }
    return m;
  }
  std::optional<uint8_t> get(UVec3 c) {
    int32_t v = -1;
    check(dust_hip_model_get_voxels(h_, c.data(), &v, 1));
    return v < 0 ? std::nullopt : std::optional<uint8_t>(uint8_t(v));
  }
  uint32_t num_blocks;
 private:
  explicit VoxGeometry(DustHipModel* adopted) : num_blocks(0), h_(adopted) {  // (detach_islands, reduce: the handle is already ours)
    uint64_t nm = 0;
    check(dust_hip_model_info(h_, &num_blocks, &nm));
  }
  DustHipModel* h_ = nullptr;
};

// What VoxLoader::load returns: models (geometry + material) and the entities that instance them.
struct VoxScene {
  std::vector<std::unique_ptr<VoxGeometry>> geometries;   // indexed by model id; null for unused models
  std::vector<DustVoxInstance> instances;                 // VoxBundle transform + model id
  std::array<uint8_t, 1024> palette{};
};

// PngLoader (rhyolite_bevy/src/loaders/png.rs:70-200): a PNG / APNG as a sliced image array, one layer per frame
struct SlicedImageArray {
  DustPngInfo info{};
  std::vector<uint8_t> texels;  // layers x height x width x channels x bytes_per_channel
};
struct PngLoader {
  static SlicedImageArray load(const uint8_t* bytes, size_t n) {
    SlicedImageArray a;
    uint8_t* p = nullptr;
    check(dust_png_load_array(bytes, n, &a.info, &p));
    const size_t total = size_t(a.info.layers) * a.info.height * a.info.width * a.info.channels * a.info.bytes_per_channel;
    a.texels.assign(p, p + total);
    dust_vox_free(p);
    return a;
  }
};

class VoxLoader {
 public:
  explicit VoxLoader(RenderContext& ctx) : ctx_(ctx) {}
  static std::vector<std::string> extensions() { return {"vox"}; }  // loader.rs:417-419
  // throws dust::Error{DUST_ERR_PARSE | DUST_ERR_UNSUPPORTED} like VoxLoadingError / unimplemented!()
  // frame: the animation frame MagicaVoxel keyframes (multi-frame nTRN, multi-model nSHP) are instantiated at; the reference
  // stops at unimplemented!() for those files (loader.rs:103-105,149-151)
  VoxScene load(const uint8_t* bytes, size_t n, uint32_t frame = 0) {
    DustVoxScene* s = nullptr;
    check(dust_vox_load_frame(bytes, n, frame, &s));
    struct Guard { DustVoxScene* s; ~Guard() { dust_vox_scene_destroy(s); } } g{s};
    VoxScene out;
    uint32_t nm = 0, ni = 0;
    check(dust_vox_scene_counts(s, &nm, &ni));
    const uint8_t* pal = nullptr;
    check(dust_vox_scene_palette(s, &pal));
    std::memcpy(out.palette.data(), pal, 1024);
    out.geometries.resize(nm);
    for (uint32_t m = 0; m < nm; ++m) {
      DustVoxModelInfo info{};
      check(dust_vox_scene_model_info(s, m, &info));
      if (!info.used) continue;
      const DustHipBlock* blocks = nullptr;
      const uint8_t* mats = nullptr;
      check(dust_vox_scene_model_data(s, m, &blocks, &mats));
      out.geometries[m] = std::make_unique<VoxGeometry>(ctx_, blocks, info.n_blocks, mats, info.n_materials, pal);
    }
    out.instances.resize(ni);
    if (ni) check(dust_vox_scene_instances(s, out.instances.data(), ni));
    return out;
  }
 private:
  RenderContext& ctx_;
};

// ----------------------------------------------------------------------------- scene (TLAS)
class Scene {
 public:
  explicit Scene(RenderContext& ctx) { check(dust_hip_scene_create(ctx.raw(), &h_)); }
  ~Scene() { dust_hip_scene_destroy(h_); }
  Scene(const Scene&) = delete;
  // spawn(VoxBundle{transform, geometry, material}) -> gl_InstanceID
  uint32_t spawn(const VoxGeometry& g, const float obj_to_world_3x4[12], const float* prev_mat4 = nullptr) {
    uint32_t id = 0;
    check(dust_hip_scene_add_instance(h_, g.raw(), obj_to_world_3x4, prev_mat4, &id));
    return id;
  }
  void spawn_scene(const VoxScene& s) {
    for (const auto& i : s.instances) spawn(*s.geometries[i.model], i.obj_to_world);
  }
  void set_transform(uint32_t id, const float obj_to_world_3x4[12], const float* prev_mat4 = nullptr) {
    check(dust_hip_scene_set_transform(h_, id, obj_to_world_3x4, prev_mat4));
  }
  void commit() { check(dust_hip_scene_commit(h_)); }
  // a game's own rays against the committed scene (the reference's RayTracingPipeline over the TLAS, pipeline/mod.rs:64-98): host
  // arrays, returns with the hits (hit.instance == DUST_HIP_NO_HIT: a miss). any_hit: some hit in [tmin, tmax], not the closest
  void trace_rays(const DustHipRay* rays, DustHipRayHit* hits, uint32_t n, bool any_hit = false) {
    check(dust_hip_scene_trace_rays(h_, rays, hits, n, any_hit ? DUST_HIP_QUERY_ANY_HIT : 0u));
  }
  std::vector<DustHipRayHit> trace_rays(const std::vector<DustHipRay>& rays, bool any_hit = false) {
    std::vector<DustHipRayHit> hits(rays.size());
    trace_rays(rays.data(), hits.data(), uint32_t(rays.size()), any_hit);
    return hits;
  }
  // device arrays, enqueued on the context's stream: the hits are there after RenderContext::sync (or an event on the caller's stream)
  void trace_rays_async(const DustHipRay* d_rays, DustHipRayHit* d_hits, uint32_t n, bool any_hit = false) {
    check(dust_hip_scene_trace_rays_async(h_, d_rays, d_hits, n, any_hit ? DUST_HIP_QUERY_ANY_HIT : 0u));
  }
  // the solid voxels inside world-space boxes (collision, placement, area edits): host arrays, returns with counts[i] and query i's first
  // min(counts[i], capacity) records at records[first ..], ordered by instance, block, voxel bit. any_hit: is the box free (count 0 / 1)
  void overlap_boxes(const DustHipBoxQuery* boxes, uint32_t n, uint32_t* counts, DustHipVoxelRef* records, uint32_t n_records,
                     bool any_hit = false) {
    check(dust_hip_scene_overlap_boxes(h_, boxes, n, counts, records, n_records, any_hit ? DUST_HIP_QUERY_ANY_HIT : 0u));
  }
  // the same into `records` as it is sized (every box's slice [first, first + capacity) must lie inside it); returns the counts
  std::vector<uint32_t> overlap_boxes(const std::vector<DustHipBoxQuery>& boxes, std::vector<DustHipVoxelRef>& records, bool any_hit = false) {
    std::vector<uint32_t> counts(boxes.size());
    overlap_boxes(boxes.data(), uint32_t(boxes.size()), counts.data(), records.data(), uint32_t(records.size()), any_hit);
    return counts;
  }
  // device arrays, enqueued on the context's stream: valid after RenderContext::sync (or an event on the caller's stream)
  void overlap_boxes_async(const DustHipBoxQuery* d_boxes, uint32_t n, uint32_t* d_counts, DustHipVoxelRef* d_records, uint32_t n_records,
                           bool any_hit = false) {
    check(dust_hip_scene_overlap_boxes_async(h_, d_boxes, n, d_counts, d_records, n_records, any_hit ? DUST_HIP_QUERY_ANY_HIT : 0u));
  }
  // the first solid voxel each box touches as it moves by delta (a character controller's move, a thrown prop): host arrays, returns
  // with hits[i] written (t = 1 and instance DUST_HIP_NO_HIT on a miss). any_hit: some hit, not necessarily the first; ignore_start:
  // voxels a box is already inside at t = 0 do not stop it
  void sweep_boxes(const DustHipBoxSweep* sweeps, DustHipSweepHit* hits, uint32_t n, bool any_hit = false, bool ignore_start = false) {
    check(dust_hip_scene_sweep_boxes(h_, sweeps, hits, n, sweep_flags(any_hit, ignore_start)));
  }
  std::vector<DustHipSweepHit> sweep_boxes(const std::vector<DustHipBoxSweep>& sweeps, bool any_hit = false, bool ignore_start = false) {
    std::vector<DustHipSweepHit> hits(sweeps.size());
    sweep_boxes(sweeps.data(), hits.data(), uint32_t(sweeps.size()), any_hit, ignore_start);
    return hits;
  }
  // device arrays (16-byte aligned), enqueued on the context's stream: valid after RenderContext::sync (or an event on the caller's stream)
  void sweep_boxes_async(const DustHipBoxSweep* d_sweeps, DustHipSweepHit* d_hits, uint32_t n, bool any_hit = false, bool ignore_start = false) {
    check(dust_hip_scene_sweep_boxes_async(h_, d_sweeps, d_hits, n, sweep_flags(any_hit, ignore_start)));
  }
  DustHipScene* raw() const { return h_; }
 private:
  static uint32_t sweep_flags(bool any_hit, bool ignore_start) {
    return (any_hit ? DUST_HIP_QUERY_ANY_HIT : 0u) | (ignore_start ? DUST_HIP_SWEEP_IGNORE_START : 0u);
  }
  DustHipScene* h_ = nullptr;
};

// ----------------------------------------------------------------------------- camera
struct PinholeProjection {  // projection.rs:3-29
  float fov = 0.78539816339744830962f;
  float near = 0.1f;
  float far = 10000.0f;
};
// rotation columns of a camera at `eye` looking at `target` (Transform::looking_at, -z forward)
inline std::array<float, 9> look_at_rotation(const double eye[3], const double target[3], const double up_[3]) {
  auto norm = [](double v[3]) { double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); for (int i = 0; i < 3; ++i) v[i] /= l; };
  double back[3] = {eye[0] - target[0], eye[1] - target[1], eye[2] - target[2]};
  norm(back);
  double right[3] = {up_[1] * back[2] - up_[2] * back[1], up_[2] * back[0] - up_[0] * back[2], up_[0] * back[1] - up_[1] * back[0]};
  norm(right);
  double up[3] = {back[1] * right[2] - back[2] * right[1], back[2] * right[0] - back[0] * right[2], back[0] * right[1] - back[1] * right[0]};
  return {float(right[0]), float(right[1]), float(right[2]), float(up[0]), float(up[1]), float(up[2]),
          float(back[0]), float(back[1]), float(back[2])};
}
inline DustHipCamera make_camera(const float eye[3], const std::array<float, 9>& rot_cols, const PinholeProjection& p) {
  DustHipCamera c{};
  std::memcpy(c.view_col0, &rot_cols[0], 12);
  std::memcpy(c.view_col1, &rot_cols[3], 12);
  std::memcpy(c.view_col2, &rot_cols[6], 12);
  std::memcpy(c.position, eye, 12);
  c.tan_half_fov = std::tan(p.fov / 2.0f);  // standard.rs:298
  c.far_ = p.far;
  c.near_ = p.near;
  return c;
}

// ----------------------------------------------------------------------------- Sunlight
// The Hosek-Wilkie tables Sunlight::bake reads, as the bytes of the reference's dataset.bin / datasetSolar.bin (sky.rs:34-63)
class SkyDataset {
 public:
  SkyDataset(const uint8_t* dataset_bin, size_t n, const uint8_t* dataset_solar_bin, size_t m) { check(dust_sky_dataset_create(dataset_bin, n, dataset_solar_bin, m, &h_)); }
  ~SkyDataset() { dust_sky_dataset_destroy(h_); }
  SkyDataset(const SkyDataset&) = delete;
  const DustSkyDataset* raw() const { return h_; }
 private:
  DustSkyDataset* h_ = nullptr;
};
struct Sunlight {  // sky.rs:6-23
  float turbidity = 1.0f;
  std::array<float, 3> albedo{0.2f, 0.2f, 0.2f};
  std::array<float, 3> direction{0.0f, 0.80114365f, -0.5984721f};
  DustHipSky bake(const SkyDataset& d) const {  // sky.rs:90-132
    DustHipSky s{};
    check(dust_sky_bake(d.raw(), turbidity, albedo.data(), direction.data(), &s));
    return s;
  }
};
struct ReblurSettings {  // nrd.rs:768-785 + NRD defaults, as far as DUST_PASS_DENOISE has the knob
  uint32_t max_accumulated_frame_num = 30;
  float disocclusion_threshold = 0.01f;
  float luminance_sigma_scale = 2.0f, luminance_antilag_power = 0.8f;
  float blur_radius = 15.0f;
};

// ----------------------------------------------------------------------------- StandardPipeline
class StandardPipeline {
 public:
  static constexpr uint32_t PRIMARY_RAYTYPE = 0;            // standard.rs:223-226
  static constexpr uint32_t AMBIENT_OCCLUSION_RAYTYPE = 1;
  static constexpr uint32_t FINAL_GATHER_RAYTYPE = 2;
  static constexpr uint32_t SURFEL_RAYTYPE = 3;
  static constexpr uint32_t num_raytypes() { return 4; }

  StandardPipeline(RenderContext& ctx, uint32_t width, uint32_t height) : width_(width), height_(height) {
    check(dust_hip_pipeline_create(ctx.raw(), width, height, &h_));
  }
  ~StandardPipeline() { dust_hip_pipeline_destroy(h_); }
  StandardPipeline(const StandardPipeline&) = delete;

  void set_blue_noise(uint32_t texture, const uint8_t* texels, uint32_t layers) {
    check(dust_hip_pipeline_set_noise(h_, texture, texels, layers));
  }
  // StandardPipeline::render: returns false ("try next frame") where the reference returns None (standard.rs:254-266)
  bool render(const Scene& scene, const DustHipCamera& camera, const DustHipSky& sunlight_baked, uint32_t passes,
              uint32_t frame_index, uint32_t rand, uint32_t row_begin = 0, uint32_t row_end = 0) {
    DustHipFrameParams fp{};
    fp.struct_size = sizeof(fp);
    fp.passes = passes; fp.frame_index = frame_index; fp.rand = rand; fp.row_begin = row_begin; fp.row_end = row_end;
    const DustStatus s = dust_hip_render_frame(h_, scene.raw(), &camera, &sunlight_baked, &fp);
    if (s == DUST_ERR_NOT_READY) return false;
    check(s);
    return true;
  }
  // Frames in flight (rhyolite_bevy/src/lib.rs:58): n frames, frame i into pipelines[i], as n render() calls in that order; primary + AO frames of
  // distinct pipelines of one context share one persistent launch (dust_hip_render_frames). false where any of them is not ready.
  static bool render_frames(StandardPipeline* const* pipelines, uint32_t n, Scene& scene, const DustHipCamera* cameras, const DustHipSky* skies,
                            uint32_t passes, const uint32_t* frame_indices, const uint32_t* rands, uint32_t row_begin = 0, uint32_t row_end = 0,
                            const DustHipFrameMoves* moves = nullptr) {   // moves[i]: the entities that moved before frame i (tlas_system's per-frame push), or null
    std::vector<DustHipPipeline*> hs(n);
    std::vector<DustHipFrameParams> fps(n);
    for (uint32_t i = 0; i < n; ++i) {
      hs[i] = pipelines[i]->h_;
      fps[i] = DustHipFrameParams{};
      fps[i].struct_size = sizeof(DustHipFrameParams);
      fps[i].passes = passes; fps[i].frame_index = frame_indices[i]; fps[i].rand = rands[i]; fps[i].row_begin = row_begin; fps[i].row_end = row_end;
    }
    const DustStatus s = dust_hip_render_frames(n, hs.data(), scene.raw(), cameras, skies, fps.data(), moves);
    if (s == DUST_ERR_NOT_READY) return false;
    check(s);
    return true;
  }
  // NRDPipeline settings / DenoiserEvent::Restart for DUST_PASS_DENOISE
  void set_denoiser(const ReblurSettings& r) {
    DustHipDenoiseParams dp{sizeof(DustHipDenoiseParams), r.max_accumulated_frame_num, r.disocclusion_threshold, r.luminance_sigma_scale,
                            r.luminance_antilag_power, r.blur_radius};
    check(dust_hip_pipeline_set_denoiser(h_, &dp));
  }
  void restart_denoiser() { check(dust_hip_pipeline_restart_denoiser(h_)); }
  // the host's frames in flight (rhyolite_bevy/src/lib.rs:58): launches then share the device instead of queueing
  void set_frames_in_flight(uint32_t n) { check(dust_hip_pipeline_set_frames_in_flight(h_, n)); }
  // the plugin's settings for this pipeline (RenderPlugin, crates/render/src/lib.rs:35-56): read, change the fields of interest, write back
  DustHipPipelineConfig config() const {
    DustHipPipelineConfig c{};
    c.struct_size = sizeof c;
    check(dust_hip_pipeline_get_config(h_, &c));
    return c;
  }
  void configure(const DustHipPipelineConfig& c) { check(dust_hip_pipeline_configure(h_, &c)); }
  void bind_plane(DustHipPlane plane, void* device_ptr, size_t bytes) { check(dust_hip_pipeline_bind_plane(h_, plane, device_ptr, bytes)); }
  template <class T>
  std::vector<T> read_plane(DustHipPlane plane) {
    size_t bytes = 0;
    void* p = nullptr;
    check(dust_hip_pipeline_plane_device_ptr(h_, plane, &p, &bytes));
    std::vector<T> out(bytes / sizeof(T));
    check(dust_hip_pipeline_read_plane(h_, plane, out.data(), bytes));
    return out;
  }
  uint32_t width() const { return width_; }
  uint32_t height() const { return height_; }
  DustHipPipeline* raw() const { return h_; }
 private:
  DustHipPipeline* h_ = nullptr;
  uint32_t width_, height_;
};


// One rank's end of the multi-GPU partition: an RCCL communicator on the context's device -- or, on one device, the
// ranks of a loopback group. The reference's plugin selects ONE device (crates/render/src/lib.rs:58-134); a host that runs one
// process per GPU makes one of these next to its RenderContext.
class DeviceComm {
 public:
  static std::vector<uint8_t> unique_id() {  // on rank 0; carried to the other processes by the host
    std::vector<uint8_t> id(DUST_HIP_COMM_ID_BYTES);
    check(dust_hip_comm_unique_id(id.data()));
    return id;
  }
  DeviceComm(RenderContext& ctx, uint32_t rank, uint32_t world, const std::vector<uint8_t>& id) { check(dust_hip_comm_create(ctx.raw(), rank, world, id.data(), &h_)); }
  explicit DeviceComm(DustHipComm* adopted) : h_(adopted) {}
  // `world` ranks on one device: collectives complete when the group's last rank has made the call
  static std::vector<std::unique_ptr<DeviceComm>> loopback(RenderContext& ctx, uint32_t world) {
    std::vector<DustHipComm*> raw(world, nullptr);
    check(dust_hip_comm_create_local(ctx.raw(), world, raw.data()));
    std::vector<std::unique_ptr<DeviceComm>> out;
    for (DustHipComm* c : raw) out.emplace_back(new DeviceComm(c));
    return out;
  }
  ~DeviceComm() { dust_hip_comm_destroy(h_); }
  DeviceComm(const DeviceComm&) = delete;
  // rows [cuts[r], cuts[r+1]) of `plane` from every rank r to `root` (its own plane when dst is null)
  // (the library reads cuts[0..world]: a shorter vector would be an out-of-bounds host read)
  void check_cuts(const std::vector<uint32_t>& cuts) const {
    uint32_t world = 0;
    check(dust_hip_comm_info(h_, nullptr, &world, nullptr));
    if (cuts.size() != size_t(world) + 1) throw Error(DUST_ERR_INVALID_ARGUMENT, "band cuts: want world + 1 row indices");
  }
  uint64_t gather_bands(StandardPipeline& p, DustHipPlane plane, const std::vector<uint32_t>& cuts, uint32_t root, void* dst = nullptr, size_t dst_bytes = 0) {
    check_cuts(cuts);
    uint64_t ticket = 0;
    check(dust_hip_gather_bands(p.raw(), h_, plane, cuts.data(), root, dst, dst_bytes, &ticket));
    return ticket;
  }
  // several planes (bit i of the mask = DustHipPlane i) in one collective, each into the root pipeline's own plane
  uint64_t gather_planes(StandardPipeline& p, uint32_t plane_mask, const std::vector<uint32_t>& cuts, uint32_t root) {
    check_cuts(cuts);
    uint64_t ticket = 0;
    check(dust_hip_gather_planes(p.raw(), h_, plane_mask, cuts.data(), root, &ticket));
    return ticket;
  }
  void gi_exchange(StandardPipeline& p, uint32_t row_begin, uint32_t row_end, uint32_t band_rows, uint32_t frame_index) {
    check(dust_hip_gi_exchange_run(p.raw(), h_, row_begin, row_end, band_rows, frame_index));
  }
  void gi_surfel_exchange(StandardPipeline& p, uint32_t frame_index) { check(dust_hip_gi_surfel_exchange_run(p.raw(), h_, frame_index)); }
  void wait(uint64_t ticket = 0) { check(dust_hip_comm_wait(h_, ticket)); }
  void sync() { check(dust_hip_comm_sync(h_)); }
  DustHipComm* raw() const { return h_; }
 private:
  DustHipComm* h_ = nullptr;
};

}  // namespace dust
