// A host's per-axis move-and-slide through the C++ mirror (include/dust_hip.hpp): sweep the player's box along y, then x, then z, each
// with one moving axis, and stop a small skin short of what it touches. Compiled (not run) by tests/test_sweep_abi.py.
#include <algorithm>

#include "dust_hip.hpp"

void move_and_slide(dust::Scene& scene, float lo[3], float hi[3], const float velocity[3], float dt) {
  const float skin = 1e-3f;
  const int order[3] = {1, 0, 2};
  for (int k : order) {
    DustHipBoxSweep s = {{lo[0], lo[1], lo[2]}, 0u, {hi[0], hi[1], hi[2]}, 0u, {0.0f, 0.0f, 0.0f}, 0u};
    s.delta[k] = velocity[k] * dt;
    if (s.delta[k] == 0.0f) continue;
    const std::vector<DustHipSweepHit> hit = scene.sweep_boxes(std::vector<DustHipBoxSweep>{s}, false, /*ignore_start=*/true);
    float move = s.delta[k] * hit[0].t;
    if (hit[0].instance != DUST_HIP_NO_HIT) move = move > 0.0f ? std::max(0.0f, move - skin) : std::min(0.0f, move + skin);
    lo[k] += move;
    hi[k] += move;
  }
}

void sweep_on_device(dust::Scene& scene, const DustHipBoxSweep* d_sweeps, DustHipSweepHit* d_hits, uint32_t n) {
  scene.sweep_boxes_async(d_sweeps, d_hits, n, /*any_hit=*/true);
}
