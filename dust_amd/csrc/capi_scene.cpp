// capi_scene.cpp -- the scene handle of the C ABI (include/dust_hip.h): instances, the commit that lays the scene's device image out
// (instance records, the top-level grid, slot order), and the scene queries (query.hip, overlap.hip, sweep.hip).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "capi_internal.hpp"
#include "query.hpp"

namespace {

// inverse of a 3x4 affine transform, evaluated in double and rounded once
void invert_affine(const float m[12], float out[12]) {
  const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  const double id = 1.0 / det;
  const double r[9] = {A * id, -(b * i - c * h) * id, (b * f - c * e) * id,
                       B * id, (a * i - c * g) * id, -(a * f - c * d) * id,
                       C * id, -(a * h - b * g) * id, (a * e - b * d) * id};
  const double tx = m[3], ty = m[7], tz = m[11];
  for (int k = 0; k < 3; ++k) {
    out[k * 4 + 0] = float(r[k * 3 + 0]); out[k * 4 + 1] = float(r[k * 3 + 1]); out[k * 4 + 2] = float(r[k * 3 + 2]);
    out[k * 4 + 3] = float(-(r[k * 3 + 0] * tx + r[k * 3 + 1] * ty + r[k * 3 + 2] * tz));
  }
}

}  // namespace

void release(const DustHipScene* cs) {
  DustHipScene* s = const_cast<DustHipScene*>(cs);
  if (!s || s->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  DustHipContext* c = s->ctx;
  (void)hipSetDevice(c->device);
  (void)sync_stream(c);  // both streams: the surfel pass reads the scene image on the second one
  s->free_images();
  for (HostInstance& hi : s->instances) release(hi.model);
  delete s;
  release(c);
}

DustStatus check_scene_ready(const DustHipScene* s) {
  if (!s->committed) return fail(DUST_ERR_NOT_READY, "scene has uncommitted changes (call dust_hip_scene_commit)");
  for (size_t i = 0; i < s->models.size(); ++i)
    if (s->models[i]->generation != s->model_generation[i])
      return fail(DUST_ERR_NOT_READY, "a model of the scene was edited after the last dust_hip_scene_commit");
  return DUST_OK;
}

extern "C" {

DustStatus dust_hip_scene_create(DustHipContext* ctx, DustHipScene** out) {
  if (!ctx || !out) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    DustHipScene* s = new DustHipScene;
    s->ctx = retain(ctx);
    *out = s;
    return DUST_OK;
  });
}
void dust_hip_scene_destroy(DustHipScene* s) { release(s); }

static DustStatus check_affine(const float m[12]) {
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(m[i])) return fail(DUST_ERR_INVALID_ARGUMENT, "non-finite instance transform");
  const double det = double(m[0]) * (double(m[5]) * m[10] - double(m[6]) * m[9]) -
                     double(m[1]) * (double(m[4]) * m[10] - double(m[6]) * m[8]) +
                     double(m[2]) * (double(m[4]) * m[9] - double(m[5]) * m[8]);
  if (!(std::fabs(det) > 1e-20)) return fail(DUST_ERR_INVALID_ARGUMENT, "singular instance transform");
  return DUST_OK;
}

DustStatus dust_hip_scene_add_instance(DustHipScene* s, const DustHipModel* model, const float o2w[12],
                                       const float prev[16], uint32_t* instance_id) {
  if (!s || !model || !o2w) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (model->ctx != s->ctx) return fail(DUST_ERR_INVALID_ARGUMENT, "model belongs to another context");
  if (s->instances.size() >= 65535) return fail(DUST_ERR_INVALID_ARGUMENT, "too many instances (voxel_id holds 16 bits)");
  DustStatus st = check_affine(o2w);
  if (st != DUST_OK) return st;
  return guarded([&] {
    HostInstance hi;
    hi.model = model;
    std::memcpy(hi.o2w, o2w, sizeof(hi.o2w));
    if (prev) std::memcpy(hi.prev, prev, sizeof(hi.prev));
    else {  // first frame: previous transform == current (standard.rs:856-878), column-major mat4
      for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) hi.prev[c * 4 + r] = r < 3 ? o2w[r * 4 + c] : (c == 3 ? 1.0f : 0.0f);
    }
    s->instances.reserve(s->instances.size() + 1);
    s->dirty.reserve(s->dirty.size() + 1);
    if (instance_id) *instance_id = uint32_t(s->instances.size());
    s->instances.push_back(hi);
    s->dirty.push_back(1);
    retain(const_cast<DustHipModel*>(model));  // the scene keeps what it instances alive
    s->structure_dirty = true;
    s->committed = false;
    return DUST_OK;
  });
}
DustStatus dust_hip_scene_set_transform(DustHipScene* s, uint32_t id, const float o2w[12], const float prev[16]) {
  if (!s || !o2w || id >= s->instances.size()) return fail(DUST_ERR_INVALID_ARGUMENT, "bad instance id");
  DustStatus st = check_affine(o2w);
  if (st != DUST_OK) return st;
  HostInstance& hi = s->instances[id];
  std::memcpy(hi.o2w, o2w, sizeof(hi.o2w));
  if (prev) std::memcpy(hi.prev, prev, sizeof(hi.prev));
  s->dirty[id] = 1;
  s->committed = false;
  return DUST_OK;
}

namespace {
// conservative world box of instance i: the eight corners of its model's tight bounds, each padded by 1e-4 of its size
void world_box(const HostInstance& hi, float wmin[3], float wmax[3]) {
  const dust::DevModel& m = hi.model->dev;
  for (int a = 0; a < 3; ++a) { wmin[a] = 1e30f; wmax[a] = -1e30f; }
  for (int c = 0; c < 8; ++c) {
    const double p[3] = {(c & 1) ? m.bmax[0] : m.bmin[0], (c & 2) ? m.bmax[1] : m.bmin[1], (c & 4) ? m.bmax[2] : m.bmin[2]};
    for (int a = 0; a < 3; ++a) {
      const float* r = hi.o2w + a * 4;
      const double w = double(r[0]) * p[0] + double(r[1]) * p[1] + double(r[2]) * p[2] + double(r[3]);
      const double pad = 1e-4 * (std::fabs(w) + 1.0);
      wmin[a] = std::min(wmin[a], float(w - pad));
      wmax[a] = std::max(wmax[a], float(w + pad));
    }
  }
}
// the device records of instance i, re-derived in the host master image (instance, box, visit)
void derive_instance(DustHipScene* s, size_t i) {
  const HostInstance& hi = s->instances[i];
  uint8_t* img = s->master.data();
  dust::DevInstance& d = reinterpret_cast<dust::DevInstance*>(img + s->layout.instances)[i];
  std::memcpy(d.o2w, hi.o2w, sizeof(d.o2w));
  std::memcpy(d.prev, hi.prev, sizeof(d.prev));
  invert_affine(hi.o2w, d.w2o);
  d.model = s->instance_slot[i];
  d.pad = 0;
  world_box(hi, d.wmin, d.wmax);
  // the world box again, packed 32 bytes apiece: what the packet culling streams through (coalesced) and the candidate
  // loop reads with one scalar load; and the flattened visit record (box, world -> object, model)
  dust::DevBox& bx = reinterpret_cast<dust::DevBox*>(img + s->layout.boxes)[i];
  dust::DevVisit& v = reinterpret_cast<dust::DevVisit*>(img + s->layout.visits)[i];
  for (int a = 0; a < 3; ++a) { bx.lo[a] = v.lo[a] = d.wmin[a]; bx.hi[a] = v.hi[a] = d.wmax[a]; }
  bx.pad0 = bx.pad1 = v.pad0 = v.pad1 = 0.0f;
  std::memcpy(v.w2o, d.w2o, sizeof(v.w2o));
  v.m = reinterpret_cast<const dust::DevModel*>(img + s->layout.models)[d.model];
  // and what the ray streams' instance set-up reads, in 80 bytes (the model's bounds are multiples of 4 up to 4096: exact in 16 bits)
  dust::DevEnter& e = reinterpret_cast<dust::DevEnter*>(img + s->layout.enters)[i];
  std::memcpy(e.w2o, d.w2o, sizeof(e.w2o));
  for (int a = 0; a < 3; ++a) { e.bmin[a] = uint16_t(v.m.bmin[a]); e.bmax[a] = uint16_t(v.m.bmax[a]); }
  e.model = uint16_t(d.model);
  e.lds_slot = v.m.lds_slot >= 0 && v.m.lds_slot < 255 ? uint8_t(v.m.lds_slot) : uint8_t(255);
  e.extent_log2 = v.m.extent > 256u ? 12 : 8;
  e.root = v.m.root;
  e.dense_mask = v.m.dense_mask;
}

// The top-level grid over the instances' world boxes (DevGrid; tlas.rs:37-65 rebuilds the TLAS every frame the same way).
// About `density` cells per instance (DUST_HIP_GRID_DENSITY, default 12; at most 256 per axis, 2^18 in all), cubes as nearly
// as the scene's proportions allow. An instance is listed in every cell its box, grown by kGridMargin of the scene's size,
// overlaps: the margin is what lets the per-ray walk (gi.hip, top_next) trust its single-precision cell steps.
// boxes: n x {lo[3], hi[3]}. ranges: per instance the block of cells it is listed in, {lo, hi} as x | y << 9 | z << 18.
constexpr double kGridMargin = 2e-5;
void build_grid(DustHipScene* s, const std::vector<float>& boxes, std::vector<uint32_t>& ranges) {
  const size_t n = boxes.size() / 6;
  dust::DevGrid& g = s->grid;
  double ext[3], big = 0.0;
  for (int a = 0; a < 3; ++a) big = std::max(big, double(s->world_max[a]) - double(s->world_min[a]));
  const double margin = kGridMargin * big + 0.01;
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = float(double(s->world_min[a]) - 2.0 * margin);
    ext[a] = std::max(double(s->world_max[a]) + 2.0 * margin - double(g.lo[a]), 1e-3 * big + 1.0);
  }
  const char* density_env = diag_env("GRID_DENSITY");  // (per commit: ~100 ns, and tests vary it)
  const double density0 = density_env ? std::max(0.001, std::atof(density_env)) : 12.0;
  ranges.resize(n * 2);
  std::vector<uint32_t> count;
  uint32_t last_dim[3] = {0, 0, 0}, halvings = 0;
  bool force_one = false;
  for (double density = density0;; density *= 0.5) {
    const double target = std::min(262144.0, std::max(1.0, density * double(std::max<size_t>(n, 1))));
    const double edge = std::cbrt(ext[0] * ext[1] * ext[2] / target);
    for (int a = 0; a < 3; ++a) {
      g.dim[a] = force_one ? 1u : uint32_t(std::min(256.0, std::max(1.0, std::floor(ext[a] / edge + 0.5))));
      g.cell[a] = float(ext[a] / double(g.dim[a]));
      g.inv_cell[a] = float(double(g.dim[a]) / ext[a]);
      g.hi[a] = float(double(g.lo[a]) + ext[a]);
    }
    const size_t n_cells = size_t(g.dim[0]) * g.dim[1] * g.dim[2];
    count.assign(n_cells, 0u);
    auto cell_of = [&](double w, int a) {
      const double c = std::floor((w - double(g.lo[a])) / ext[a] * double(g.dim[a]));
      return uint32_t(std::min(double(g.dim[a] - 1), std::max(0.0, c)));
    };
    size_t total = 0;
    uint32_t most = 0;
    for (size_t i = 0; i < n; ++i) {
      uint32_t lo[3], hi[3];
      for (int a = 0; a < 3; ++a) { lo[a] = cell_of(double(boxes[i * 6 + a]) - margin, a); hi[a] = cell_of(double(boxes[i * 6 + 3 + a]) + margin, a); }
      ranges[i * 2] = lo[0] | (lo[1] << 9) | (lo[2] << 18);
      ranges[i * 2 + 1] = hi[0] | (hi[1] << 9) | (hi[2] << 18);
      for (uint32_t z = lo[2]; z <= hi[2]; ++z)
        for (uint32_t y = lo[1]; y <= hi[1]; ++y)
          for (uint32_t x = lo[0]; x <= hi[0]; ++x) most = std::max(most, ++count[(size_t(z) * g.dim[1] + y) * g.dim[0] + x]);
      total += size_t(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
    }
    // (coarser until the item array fits the packed cell word's 20 index bits: never, for scenes of any sane shape. More than 4095 boxes over
    //  ONE cell cannot be listed at any resolution that helps: the grid is then marked unusable and the single-ray paths are not taken)
    s->grid_valid = most <= dust::kGridMaxCellItems;
    if (total < (size_t(1) << dust::kGridItemBits) || n_cells == 1) break;
    // (a fuse: an elongated scene whose rounded dims stop shrinking -- density x n <= 1 clamps the target to one cell, which ext / cbrt(V)
    //  never reaches for aspects above ~2 -- or 40 halvings: ONE cell then; should even that list 2^20 items or more -- 2^20 boxes do not
    //  exist, 65 535 instances at most --, the grid is marked unusable like a cell of more than 4095)
    const bool stuck = g.dim[0] == last_dim[0] && g.dim[1] == last_dim[1] && g.dim[2] == last_dim[2];
    for (int a = 0; a < 3; ++a) last_dim[a] = g.dim[a];
    if (force_one) { s->grid_valid = false; break; }
    if (stuck || ++halvings >= 40) force_one = true;
  }
  const size_t n_cells = count.size();
  s->grid_cells.assign(n_cells, 0u);
  std::vector<uint32_t> at(n_cells);
  uint32_t run = 0;
  for (size_t c = 0; c < n_cells; ++c) {
    at[c] = run;
    s->grid_cells[c] = run | (std::min(count[c], dust::kGridMaxCellItems) << dust::kGridItemBits);
    run += count[c];
  }
  g.n_items = run;
  s->grid_items.assign(run, 0);
  for (size_t i = 0; i < n; ++i) {  // ascending instance order inside every cell
    const uint32_t rl = ranges[i * 2], rh = ranges[i * 2 + 1];
    for (uint32_t z = rl >> 18; z <= (rh >> 18); ++z)
      for (uint32_t y = (rl >> 9) & 255u; y <= ((rh >> 9) & 255u); ++y)
        for (uint32_t x = rl & 255u; x <= (rh & 255u); ++x) s->grid_items[at[(size_t(z) * g.dim[1] + y) * g.dim[0] + x]++] = uint16_t(i);
  }
}
// the instances in the order of a Hilbert curve through their boxes' centres (10 bits per axis over the scene's bounds; Skilling's
// transform): the packet cull's groups are runs of 64 consecutive slots, and consecutive cells of this curve are always neighbours
// (along a Z-order a run that crosses a block boundary jumps across the scene, and the group's box with it)
void order_slots(DustHipScene* s) {
  const size_t n = s->world_boxes.size() / 6;
  std::vector<std::pair<uint32_t, uint32_t>> keyed(n);
  auto spread = [](uint32_t v) { v &= 1023u; v = (v | (v << 16)) & 0x030000FFu; v = (v | (v << 8)) & 0x0300F00Fu; v = (v | (v << 4)) & 0x030C30C3u; return (v | (v << 2)) & 0x09249249u; };
  for (size_t i = 0; i < n; ++i) {
    uint32_t c[3];
    for (int a = 0; a < 3; ++a) {
      const double span = std::max(1e-6, double(s->world_max[a]) - double(s->world_min[a]));
      const double mid = 0.5 * (double(s->world_boxes[i * 6 + a]) + double(s->world_boxes[i * 6 + 3 + a]));
      c[a] = uint32_t(std::min(1023.0, std::max(0.0, (mid - double(s->world_min[a])) / span * 1024.0)));
    }
    uint32_t X[3] = {c[0], c[1], c[2]};
    for (uint32_t Q = 512u; Q > 1u; Q >>= 1) {
      const uint32_t P = Q - 1u;
      for (int a = 0; a < 3; ++a) {
        if (X[a] & Q) X[0] ^= P;
        else { const uint32_t t = (X[0] ^ X[a]) & P; X[0] ^= t; X[a] ^= t; }
      }
    }
    X[1] ^= X[0]; X[2] ^= X[1];
    uint32_t t = 0;
    for (uint32_t Q = 512u; Q > 1u; Q >>= 1) if (X[2] & Q) t ^= Q - 1u;
    for (uint32_t& x : X) x ^= t;
    keyed[i] = {(spread(X[0]) << 2) | (spread(X[1]) << 1) | spread(X[2]), uint32_t(i)};
  }
  std::sort(keyed.begin(), keyed.end());
  s->slot_order.resize(n);
  for (size_t k = 0; k < n; ++k) s->slot_order[k] = keyed[k].second;
}
}  // namespace

DustStatus dust_hip_scene_commit(DustHipScene* s) {
  if (!s) return fail(DUST_ERR_INVALID_ARGUMENT, "null scene");
  return guarded([&]() -> DustStatus {
    HIP_TRY(hipSetDevice(s->ctx->device));
    const size_t n = s->instances.size();
    // a model edited since the last commit changes its record (bounds, sizes, maybe addresses): everything is derived again
    for (size_t i = 0; i < s->models.size() && !s->structure_dirty; ++i)
      if (s->models[i]->generation != s->model_generation[i]) s->structure_dirty = true;
    bool full = s->structure_dirty;
    if (full) {
      s->committed = false;  // (until the new image is up: what follows replaces the layout the current one was made with)
      s->models.clear();
      s->instance_slot.resize(n);
      for (size_t i = 0; i < n; ++i) {
        const DustHipModel* m = s->instances[i].model;
        auto it = std::find(s->models.begin(), s->models.end(), m);
        s->instance_slot[i] = uint32_t(it - s->models.begin());
        if (it == s->models.end()) s->models.push_back(m);
      }
      // roots of the first models go to LDS, as many as the budget holds
      s->n_lds_models = std::min<uint32_t>(uint32_t(s->models.size()), s->ctx->lds_root_bytes / dust::kN16LdsBytes);
    }
    // the instances' world boxes (those that moved, or all), the scene's bounds, and the top-level grid over them: the grid's
    // size decides the image's layout
    s->world_boxes.resize(n * 6);
    for (size_t i = 0; i < n; ++i)
      if (full || s->dirty[i]) world_box(s->instances[i], &s->world_boxes[i * 6], &s->world_boxes[i * 6 + 3]);
    for (int a = 0; a < 3; ++a) { s->world_min[a] = 1e30f; s->world_max[a] = -1e30f; }
    for (size_t i = 0; i < n; ++i)
      for (int a = 0; a < 3; ++a) { s->world_min[a] = std::min(s->world_min[a], s->world_boxes[i * 6 + a]); s->world_max[a] = std::max(s->world_max[a], s->world_boxes[i * 6 + 3 + a]); }
    if (n == 0) for (int a = 0; a < 3; ++a) s->world_min[a] = s->world_max[a] = 0.0f;
    std::vector<uint32_t> ranges;
    build_grid(s, s->world_boxes, ranges);
    const size_t n_cells = s->grid_cells.size(), n_items = s->grid_items.size();
    if (!full && (n_cells > s->layout.cap_cells || n_items > s->layout.cap_items)) full = true;  // the grid outgrew its sections
    if (full) {
      s->committed = false;
      s->structure_dirty = true;
      s->layout = SceneLayout::make(n, s->models.size(), s->n_lds_models, n_cells, n_items);
      if (s->layout.total > s->image_capacity || s->current < 0) {
        // grow (rare: instances were added). Launches that read the old images are done before they go; the new ones are
        // allocated into locals first, so a failed allocation leaves the scene as it was (and the next commit tries again).
        HIP_TRY(sync_stream(s->ctx));
        const size_t cap = s->layout.total + s->layout.total / 2 + 4096;
        DustHipScene::Slot fresh[DustHipScene::kImages];
        hipError_t ge = hipSuccess;
        for (DustHipScene::Slot& sl : fresh) {
          if (ge == hipSuccess) ge = sl.dev.alloc(cap);
          if (ge == hipSuccess) ge = hipHostMalloc(&sl.host, cap, hipHostMallocDefault);
        }
        if (ge != hipSuccess) {
          for (DustHipScene::Slot& sl : fresh) { if (sl.host) (void)hipHostFree(sl.host); sl.dev.release(); }
          s->structure_dirty = true;  // (the layout above is not the images': the next commit starts over)
          s->committed = false;
          return hip_fail(ge, "scene image allocation");
        }
        s->committed = false;  // no current image until the upload below has succeeded (a frame must not index slot -1)
        s->structure_dirty = true;
        s->free_images();
        for (int i = 0; i < DustHipScene::kImages; ++i) {
          s->slots[i].dev.p = fresh[i].dev.p; s->slots[i].dev.bytes = fresh[i].dev.bytes;
          fresh[i].dev.p = nullptr; fresh[i].dev.bytes = 0;  // (ownership moved: the local's destructor frees nothing)
          s->slots[i].host = fresh[i].host; s->slots[i].epoch = 0;
        }
        s->image_capacity = cap;
        s->next_slot = 0;
      }
      s->master.assign(s->layout.total, 0);
      uint8_t* img = s->master.data();
      dust::DevModel* dm = reinterpret_cast<dust::DevModel*>(img + s->layout.models);
      for (size_t i = 0; i < s->models.size(); ++i) {
        dm[i] = s->models[i]->dev;
        dm[i].lds_slot = i < s->n_lds_models ? int32_t(i) : -1;
      }
      for (uint32_t i = 0; i < s->n_lds_models; ++i)
        std::memcpy(img + s->layout.root_table + size_t(i) * dust::kN16LdsBytes, s->models[i]->host_root.data(), dust::kN16LdsBytes);
      s->model_generation.clear();
      for (const DustHipModel* m : s->models) s->model_generation.push_back(m->generation);
    }
    uint8_t* img = s->master.data();
    for (size_t i = 0; i < n; ++i)
      if (full || s->dirty[i]) { derive_instance(s, i); s->dirty[i] = 0; }
    // (the record behind the last instance stays zero: the cull reads boxes 64 at a time)
    // every instance's block of grid cells into the spare words of its box record (the grid is new: so are the blocks), the grid behind the records
    {
      dust::DevBox* bx = reinterpret_cast<dust::DevBox*>(img + s->layout.boxes);
      dust::DevVisit* vs = reinterpret_cast<dust::DevVisit*>(img + s->layout.visits);
      for (size_t i = 0; i < n; ++i) {
        std::memcpy(&bx[i].pad0, &ranges[i * 2], 4); std::memcpy(&bx[i].pad1, &ranges[i * 2 + 1], 4);
        vs[i].pad0 = bx[i].pad0; vs[i].pad1 = bx[i].pad1;
      }
      std::memcpy(img + s->layout.grid_cells, s->grid_cells.data(), s->grid_cells.size() * sizeof(uint32_t));
      // the packet cull's 64-wide hierarchy (kernels: cull_instances): slots along a Morton curve through the boxes' centres -- ordered
      // by structural commits, refitted by every commit --, a box per 64 consecutive slots
      s->n_groups = n > dust::kFlatCullMax && !diag_env("FLAT_CULL") ? uint32_t((n + 63) / 64) : 0u;  // (DUST_HIP_FLAT_CULL: every box for every packet, for A/B runs)
      if (s->n_groups) {
        if (full || s->slot_order.size() != n) {
          order_slots(s);
        }
        dust::DevBox* sb = reinterpret_cast<dust::DevBox*>(img + s->layout.sboxes);
        dust::DevBox* gb = reinterpret_cast<dust::DevBox*>(img + s->layout.gboxes);
        for (uint32_t g = 0; g < s->n_groups; ++g) {
          dust::DevBox u;
          for (int a = 0; a < 3; ++a) { u.lo[a] = 1e30f; u.hi[a] = -1e30f; }
          u.pad0 = u.pad1 = 0.0f;
          for (size_t k = size_t(g) * 64; k < std::min(n, size_t(g + 1) * 64); ++k) {
            const uint32_t i = s->slot_order[k];
            sb[k] = bx[i];
            std::memcpy(&sb[k].pad0, &i, 4);
            for (int a = 0; a < 3; ++a) { u.lo[a] = std::min(u.lo[a], bx[i].lo[a]); u.hi[a] = std::max(u.hi[a], bx[i].hi[a]); }
          }
          gb[g] = u;
        }
      } else {
        s->slot_order.clear();
      }
      if (n_items) std::memcpy(img + s->layout.grid_items, s->grid_items.data(), n_items * sizeof(uint16_t));
    }
    // upload: the whole image into the next slot of the ring, on the copy stream, and wait for it here (a ~100 KB copy: ~20 us of host
    // time, none of the launch stream's); frames in flight keep reading the slot they were enqueued with
    if (!s->ctx->copy) HIP_TRY(hipStreamCreateWithFlags(&s->ctx->copy, hipStreamNonBlocking));
    const int slot = int(s->next_slot++ % DustHipScene::kImages);
    DustHipScene::Slot& sl = s->slots[slot];
    if (sl.epoch == s->ctx->sync_epoch) {  // nobody has waited since a frame last read this slot: the host is a ring ahead
      // The frame AFTER that one has started => that one is done (one stream, launches in order; only the plain case: nothing outstanding on the
      // side stream or on communicators' streams). The GPU keeps the rest of the ring to work on meanwhile:
      // waiting for the whole stream instead left it idle for the ~50 us the host needs to enqueue again, every 8th frame (2 % of a moving view).
      DustHipContext* c = s->ctx;
      bool waited = false;
      const uint32_t need = sl.last_seq + (c->side ? 2u : 1u);  // (a surfel pass on the side stream is joined in the course of the NEXT frame: one more)
      if (c->started && sl.last_seq != 0 && !c->side_busy && c->extra_streams.empty() && int32_t(c->frame_seq - need) >= 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0;; ++spin) {
          if (int32_t(*c->started - need) >= 0) { waited = true; break; }
          if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;  // (something else holds the queue: wait for all of it)
        }
      }
      if (!waited) HIP_TRY(sync_stream(c));
    }
    const size_t used = s->layout.grid_items + n_items * sizeof(uint16_t);  // (the sections' spare room is not sent)
    std::memcpy(sl.host, img, used);
    HIP_TRY(hipMemcpyAsync(sl.dev.p, sl.host, used, hipMemcpyHostToDevice, s->ctx->copy));
    HIP_TRY(hipStreamSynchronize(s->ctx->copy));
    s->current = slot;
    ++s->revision;
    s->structure_dirty = false;
    s->committed = true;
    return DUST_OK;
  });
}

DustStatus dust_hip_top_level_build(const float* boxes, uint32_t n, DustTopLevelInfo* info, uint32_t* cells, size_t cells_capacity, uint16_t* items,
                                size_t items_capacity, uint32_t* ranges, uint32_t* slot_order) {
  if (!boxes || !info || n == 0 || n > 65535) return fail(DUST_ERR_INVALID_ARGUMENT, "bad top-level build arguments");
  STRUCT_TRY(info, "DustTopLevelInfo");
  return guarded([&]() -> DustStatus {
    DustHipScene s;   // (a bare scene record: no context, no device: only what build_grid / order_slots read and write)
    s.world_boxes.assign(boxes, boxes + size_t(n) * 6);
    for (int a = 0; a < 3; ++a) { s.world_min[a] = 1e30f; s.world_max[a] = -1e30f; }
    for (uint32_t i = 0; i < n; ++i)
      for (int a = 0; a < 3; ++a) {
        if (!(boxes[i * 6 + a] <= boxes[i * 6 + 3 + a])) return fail(DUST_ERR_INVALID_ARGUMENT, "a box with lo > hi (or NaN)");
        s.world_min[a] = std::min(s.world_min[a], boxes[i * 6 + a]); s.world_max[a] = std::max(s.world_max[a], boxes[i * 6 + 3 + a]);
      }
    std::vector<uint32_t> rg;
    build_grid(&s, s.world_boxes, rg);
    if (!s.grid_valid) return fail(DUST_ERR_UNSUPPORTED, "more than 4095 boxes over one grid cell: no grid lists them (a scene renders by the packet kernels then)");
    order_slots(&s);
    for (int a = 0; a < 3; ++a) { info->dim[a] = s.grid.dim[a]; info->lo[a] = s.grid.lo[a]; info->cell[a] = s.grid.cell[a]; }
    info->n_cells = uint32_t(s.grid_cells.size());
    info->n_items = uint32_t(s.grid_items.size());
    info->n_groups = n > dust::kFlatCullMax ? (n + 63) / 64 : 0;
    if (cells) { if (cells_capacity < s.grid_cells.size()) return fail(DUST_ERR_INVALID_ARGUMENT, "cells buffer too small"); std::memcpy(cells, s.grid_cells.data(), s.grid_cells.size() * 4); }
    if (items) { if (items_capacity < s.grid_items.size()) return fail(DUST_ERR_INVALID_ARGUMENT, "items buffer too small"); std::memcpy(items, s.grid_items.data(), s.grid_items.size() * 2); }
    if (ranges) std::memcpy(ranges, rg.data(), size_t(n) * 8);
    if (slot_order) std::memcpy(slot_order, s.slot_order.data(), size_t(n) * 4);
    return DUST_OK;
  });
}

}  // extern "C"

// Scene queries (query.hip, overlap.hip, sweep.hip). Enqueued on the context's stream as a frame is: the launch reads the scene image's current
// slot, which touch() marks, so that a commit DustHipScene::kImages commits later does not overwrite it while the query may still read it.
namespace {

// The checks every entry point shares. A null scene is refused; n == 0 is DUST_OK whatever the arrays (the caller returns there); then the
// arrays, the flags the kind allows, and the scene as committed.
DustStatus check_query(const DustHipScene* s, uint32_t n, std::initializer_list<const void*> arrays, uint32_t flags, uint32_t allowed) {
  if (!s) return fail(DUST_ERR_INVALID_ARGUMENT, "null scene");
  if (n == 0) return DUST_OK;
  for (const void* p : arrays)
    if (!p) return fail(DUST_ERR_INVALID_ARGUMENT, "null argument");
  if (flags & ~allowed) return fail(DUST_ERR_INVALID_ARGUMENT, "unknown query flags");
  return check_scene_ready(s);
}
constexpr uint32_t kSweepFlags = DUST_HIP_QUERY_ANY_HIT | DUST_HIP_SWEEP_IGNORE_START;

// The launch protocol every kind shares: the pair of device counters (allocated once; a launch takes queries from one and zeroes the other for
// the next), the scene half of the descriptor, the scene image slot marked. enqueue(a, counter, next_counter) fills the kind's own arguments,
// chooses its launch shape and launches.
template <class Enqueue>
DustStatus launch_query(DustHipScene* s, Enqueue&& enqueue) {
  DustHipContext* ctx = s->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->query_counters.p) {
    HIP_TRY(ctx->query_counters.alloc(2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(ctx->query_counters.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
  }
  s->touch();
  dust::FrameArgs a{};
  scene_args(s, a);
  for (const DustHipModel* m : s->models) a.deep |= m->dev.n_levels == 3 ? 1u : 0u;
  unsigned long long* counters = static_cast<unsigned long long*>(ctx->query_counters.p);
  HIP_TRY(enqueue(a, counters + ctx->query_parity, counters + (ctx->query_parity ^ 1u)));
  ctx->query_parity ^= 1u;
  return DUST_OK;
}
// a wave per query, `chunk` queries per trip to the counter; persistent workgroups of `waves_per_group` waves, up to 8 per CU; a single query is one wave
struct LaunchShape { uint32_t grid, block; };
LaunchShape wave_per_query(uint32_t n, uint32_t chunk, uint32_t waves_per_group, int cus) {
  const uint32_t waves = (n + chunk - 1u) / chunk;
  return {std::max<uint32_t>(1u, std::min<uint32_t>(uint32_t(cus) * 8u, (waves + waves_per_group - 1u) / waves_per_group)),
          std::min(waves, waves_per_group) * 64u};
}

// The synchronous calls: each host array through the context's staging slot of the same index {stage_in, stage_out, stage_aux} -- the slots
// grown, the inputs uploaded, the device path run on the slots (run(dev[])), the outputs downloaded, the stream waited for.
struct Staged { const void* up; void* down; size_t bytes; };  // what goes up before the launch (or null), what comes down after it (or null)
template <class Run>
DustStatus run_staged(DustHipScene* s, std::initializer_list<Staged> arrays, Run&& run) {
  return guarded([&]() -> DustStatus {
    DustHipContext* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DeviceBuffer* const slot[3] = {&c->stage_in, &c->stage_out, &c->stage_aux};
    void* dev[3] = {};
    DustStatus st = DUST_OK;
    for (size_t i = 0; i < arrays.size(); ++i) {
      const Staged& h = arrays.begin()[i];
      if ((st = grow(c, *slot[i], h.bytes)) != DUST_OK) return st;
      dev[i] = slot[i]->p;
      if (h.up && h.bytes) HIP_TRY(hipMemcpyAsync(dev[i], h.up, h.bytes, hipMemcpyHostToDevice, c->stream));
    }
    if ((st = run(dev)) != DUST_OK) return st;
    for (size_t i = 0; i < arrays.size(); ++i) {
      const Staged& h = arrays.begin()[i];
      if (h.down && h.bytes) HIP_TRY(hipMemcpyAsync(h.down, dev[i], h.bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DUST_OK;
  });
}

// ---- ray queries (query.hip)
DustStatus trace_rays_impl(DustHipScene* s, const DustHipRay* d_rays, DustHipRayHit* d_hits, uint32_t n, uint32_t flags) {
  return launch_query(s, [&](const dust::FrameArgs& a, unsigned long long* counter, unsigned long long* next_counter) {
    const dust::QueryArgs q{reinterpret_cast<const float*>(d_rays), reinterpret_cast<uint32_t*>(d_hits), n, (flags & DUST_HIP_QUERY_ANY_HIT) ? 1u : 0u,
                            counter, next_counter};
    // persistent 1024-thread workgroups, at most one per CU (each stages the roots once); a picking query is one small workgroup
    const uint32_t block = n >= 1024u ? 1024u : (n + 63u) / 64u * 64u;
    const uint32_t grid = std::min<uint32_t>(uint32_t(s->ctx->num_cus), (n + 1023u) / 1024u);
    return dust::launch_ray_query(a, q, grid, block, s->ctx->stream);
  });
}

// ---- box queries (overlap.hip)
DustStatus overlap_boxes_impl(DustHipScene* s, const DustHipBoxQuery* d_boxes, uint32_t n, uint32_t* d_counts, DustHipVoxelRef* d_records,
                              uint32_t n_records, uint32_t flags) {
  return launch_query(s, [&](const dust::FrameArgs& a, unsigned long long* counter, unsigned long long* next_counter) {
    const dust::OverlapArgs o{reinterpret_cast<const float*>(d_boxes), d_counts, reinterpret_cast<uint32_t*>(d_records), n, n_records,
                              (flags & DUST_HIP_QUERY_ANY_HIT) ? 1u : 0u, /*pad*/ 0u, counter, next_counter};
    const LaunchShape sh = wave_per_query(n, dust::kOverlapChunk, dust::kOverlapWaves, s->ctx->num_cus);
    return dust::launch_overlap_boxes(a, o, sh.grid, sh.block, s->ctx->stream);
  });
}

// ---- box sweeps (sweep.hip)
DustStatus sweep_boxes_impl(DustHipScene* s, const DustHipBoxSweep* d_sweeps, DustHipSweepHit* d_hits, uint32_t n, uint32_t flags) {
  return launch_query(s, [&](const dust::FrameArgs& a, unsigned long long* counter, unsigned long long* next_counter) {
    const dust::SweepArgs o{reinterpret_cast<const float*>(d_sweeps), reinterpret_cast<uint32_t*>(d_hits), n, (flags & DUST_HIP_QUERY_ANY_HIT) ? 1u : 0u,
                            (flags & DUST_HIP_SWEEP_IGNORE_START) ? 1u : 0u, /*pad*/ 0u, counter, next_counter};
    const LaunchShape sh = wave_per_query(n, dust::kSweepChunk, dust::kSweepWaves, s->ctx->num_cus);
    return dust::launch_sweep_boxes(a, o, sh.grid, sh.block, s->ctx->stream);
  });
}

}  // namespace

extern "C" {

DustStatus dust_hip_scene_trace_rays(DustHipScene* s, const DustHipRay* rays, DustHipRayHit* hits, uint32_t n, uint32_t flags) {
  const DustStatus cs = check_query(s, n, {rays, hits}, flags, DUST_HIP_QUERY_ANY_HIT);
  if (cs != DUST_OK || n == 0) return cs;
  return run_staged(s, {{rays, nullptr, size_t(n) * sizeof(DustHipRay)}, {nullptr, hits, size_t(n) * sizeof(DustHipRayHit)}}, [&](void* const* dev) {
    return trace_rays_impl(s, static_cast<const DustHipRay*>(dev[0]), static_cast<DustHipRayHit*>(dev[1]), n, flags);
  });
}
DustStatus dust_hip_scene_trace_rays_async(DustHipScene* s, const DustHipRay* d_rays, DustHipRayHit* d_hits, uint32_t n, uint32_t flags) {
  const DustStatus cs = check_query(s, n, {d_rays, d_hits}, flags, DUST_HIP_QUERY_ANY_HIT);
  if (cs != DUST_OK || n == 0) return cs;
  if ((reinterpret_cast<uintptr_t>(d_rays) | reinterpret_cast<uintptr_t>(d_hits)) & 15u)
    return fail(DUST_ERR_INVALID_ARGUMENT, "the ray and hit arrays must be 16-byte aligned (the kernel moves records as 16-byte vectors)");
  return guarded([&]() -> DustStatus { return trace_rays_impl(s, d_rays, d_hits, n, flags); });
}

DustStatus dust_hip_scene_overlap_boxes(DustHipScene* s, const DustHipBoxQuery* boxes, uint32_t n, uint32_t* counts, DustHipVoxelRef* records,
                                        uint32_t n_records, uint32_t flags) {
  const DustStatus cs = check_query(s, n, {boxes, counts, n_records ? static_cast<const void*>(records) : counts}, flags, DUST_HIP_QUERY_ANY_HIT);
  if (cs != DUST_OK || n == 0) return cs;
  for (uint32_t i = 0; i < n; ++i)  // every slice inside the records, before anything is launched
    if (boxes[i].capacity && uint64_t(boxes[i].first) + boxes[i].capacity > n_records)
      return fail(DUST_ERR_INVALID_ARGUMENT, "a box query's slice [first, first + capacity) runs past n_records");
  // slots past a query's count are left as the caller has them: the records go up, and come back, whole
  return run_staged(s, {{boxes, nullptr, size_t(n) * sizeof(DustHipBoxQuery)}, {nullptr, counts, size_t(n) * sizeof(uint32_t)},
                        {records, records, size_t(n_records) * sizeof(DustHipVoxelRef)}}, [&](void* const* dev) {
    return overlap_boxes_impl(s, static_cast<const DustHipBoxQuery*>(dev[0]), n, static_cast<uint32_t*>(dev[1]), static_cast<DustHipVoxelRef*>(dev[2]),
                              n_records, flags);
  });
}
DustStatus dust_hip_scene_overlap_boxes_async(DustHipScene* s, const DustHipBoxQuery* d_boxes, uint32_t n, uint32_t* d_counts, DustHipVoxelRef* d_records,
                                              uint32_t n_records, uint32_t flags) {
  const DustStatus cs = check_query(s, n, {d_boxes, d_counts, n_records ? static_cast<const void*>(d_records) : d_counts}, flags, DUST_HIP_QUERY_ANY_HIT);
  if (cs != DUST_OK || n == 0) return cs;
  if ((reinterpret_cast<uintptr_t>(d_boxes) | reinterpret_cast<uintptr_t>(d_records)) & 15u)
    return fail(DUST_ERR_INVALID_ARGUMENT, "the box and record arrays must be 16-byte aligned (the kernel moves records as 16-byte vectors)");
  return guarded([&]() -> DustStatus { return overlap_boxes_impl(s, d_boxes, n, d_counts, d_records, n_records, flags); });
}

DustStatus dust_hip_scene_sweep_boxes(DustHipScene* s, const DustHipBoxSweep* sweeps, DustHipSweepHit* hits, uint32_t n, uint32_t flags) {
  const DustStatus cs = check_query(s, n, {sweeps, hits}, flags, kSweepFlags);
  if (cs != DUST_OK || n == 0) return cs;
  return run_staged(s, {{sweeps, nullptr, size_t(n) * sizeof(DustHipBoxSweep)}, {nullptr, hits, size_t(n) * sizeof(DustHipSweepHit)}}, [&](void* const* dev) {
    return sweep_boxes_impl(s, static_cast<const DustHipBoxSweep*>(dev[0]), static_cast<DustHipSweepHit*>(dev[1]), n, flags);
  });
}
DustStatus dust_hip_scene_sweep_boxes_async(DustHipScene* s, const DustHipBoxSweep* d_sweeps, DustHipSweepHit* d_hits, uint32_t n, uint32_t flags) {
  const DustStatus cs = check_query(s, n, {d_sweeps, d_hits}, flags, kSweepFlags);
  if (cs != DUST_OK || n == 0) return cs;
  if ((reinterpret_cast<uintptr_t>(d_sweeps) | reinterpret_cast<uintptr_t>(d_hits)) & 15u)
    return fail(DUST_ERR_INVALID_ARGUMENT, "the sweep and hit arrays must be 16-byte aligned (the kernel moves them as 16-byte vectors)");
  return guarded([&]() -> DustStatus { return sweep_boxes_impl(s, d_sweeps, d_hits, n, flags); });
}

}  // extern "C"
