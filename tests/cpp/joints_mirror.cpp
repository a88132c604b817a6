// A host's "one breakable joint per pair of touching pieces" through the C++ mirror (include/dust_hip.hpp): area, anchor and normal of
// every contact between the cells of the standing fracture, and which cells still touch the unbroken rest. Compiled (not run) by
// tests/test_joints_abi.py.
#include "dust_hip.hpp"

struct Joint { uint32_t a, b; double area, anchor[3], normal[3]; bool to_rest; };

std::vector<Joint> breakable_joints(const dust::VoxGeometry& model) {
  DustHipJointQuery q{};
  q.group = DUST_HIP_JOINTS_CELLS;
  q.palette = -1;
  for (int r = 0; r < 3; ++r) q.hi[r] = 255;
  std::vector<Joint> out;
  for (const DustHipJoint& j : model.joints(q)) {
    Joint joint{j.a, j.b, double(j.faces), {0, 0, 0}, {0, 0, 0}, j.b == DUST_HIP_JOINT_REST};
    for (int r = 0; r < 3; ++r) {
      joint.anchor[r] = double(j.sum2[r]) / (2.0 * double(j.faces));
      joint.normal[r] = double(j.by_face[2 * r + 1]) - double(j.by_face[2 * r]);
    }
    out.push_back(joint);
  }
  static_assert(sizeof(DustHipJointQuery) == 48 && sizeof(DustHipJoint) == 80, "joint records");
  return out;
}
