// A host's "one rigid body per loose piece" through the C++ mirror (include/dust_hip.hpp): mass and centre of mass of every island
// of the standing labelling under a density table. Compiled (not run) by tests/test_body_abi.py.
#include "dust_hip.hpp"

struct RigidBody { uint32_t key; double mass, com[3]; };

std::vector<RigidBody> rigid_bodies(const dust::VoxGeometry& model, const uint16_t (&density)[DUST_HIP_BODY_WEIGHTS]) {
  DustHipBodyQuery q{};
  q.group = DUST_HIP_BODIES_ISLANDS;
  q.palette = -1;
  for (int r = 0; r < 3; ++r) q.hi[r] = 255;
  std::vector<RigidBody> out;
  for (const DustHipBody& b : model.bodies(q, density)) {
    RigidBody body{b.key, double(b.mass), {0, 0, 0}};
    if (b.mass)
      for (int r = 0; r < 3; ++r) body.com[r] = double(b.m1[r]) / double(b.mass) + 0.5;
    out.push_back(body);
  }
  static_assert(sizeof(DustHipBodyQuery) == 48 && sizeof(DustHipBody) == 96, "body records");
  return out;
}
