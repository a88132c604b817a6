// A host's "flat colliders for the physics engine, one set per edit" through the C++ mirror (include/dust_hip.hpp): the model's
// exposed faces come back merged into rectangles, materials ignored, and are turned into boxes one voxel thick. Compiled (not run) by
// tests/test_mesh_abi.py.
#include "dust_hip.hpp"

struct Collider { uint32_t lo[3], hi[3]; };  // inclusive voxel bounds of the slab of voxels behind a quad

std::vector<Collider> colliders(const dust::VoxGeometry& terrain, uint32_t* area) {
  DustHipMeshQuery all{};
  all.faces = DUST_HIP_FACES_ALL;
  all.flags = DUST_HIP_MESH_ANY_PALETTE;
  all.palette = -1;
  for (int r = 0; r < 3; ++r) all.hi[r] = 255;
  DustHipMeshResult result{};
  const std::vector<DustHipMeshQuad> quads = terrain.mesh(all, &result);
  std::vector<Collider> out;
  out.reserve(quads.size());
  for (const DustHipMeshQuad& q : quads) {
    const uint32_t n = q.face >> 1, u = n == 2u ? 1u : 2u, v = n == 0u ? 1u : 0u;  // u: the higher-numbered remaining axis
    Collider c{};
    c.lo[0] = q.key >> 16; c.lo[1] = (q.key >> 8) & 255u; c.lo[2] = q.key & 255u;
    for (int r = 0; r < 3; ++r) c.hi[r] = c.lo[r];
    c.hi[u] += q.du;
    c.hi[v] += q.dv;
    out.push_back(c);
  }
  static_assert(sizeof(DustHipMeshQuery) == 48 && sizeof(DustHipMeshResult) == 64 && sizeof(DustHipMeshQuad) == 8, "mesh records");
  if (area) *area = result.faces;
  return out;
}
