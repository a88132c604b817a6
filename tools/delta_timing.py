"""Model deltas (dust_hip_model_delta, dust_hip_model_delta_apply) on two pairs of editable 256^3 models: the solid terrain block of
tools/shape_edit_timing.py (y < 128, three layers of material, 8.4 M voxels) before and after a radius-24 CARVE at its surface, and a
half-density random fill of the whole tree (8.4 M voxels) against a re-seeded one of other materials (about a quarter of the tree
added, a quarter removed, a quarter repainted). Per pair, on the same run:
  (a) counts only for ADDED | REMOVED (brick masks alone: no grid byte is read);
  (b) counts for ALL (the grid bytes of the bricks solid in both);
  (c) ALL with the before / after tables;
  (d) the full list (a count call, then a call with room for every voxel: what Model.delta(capacity=None) does);
  (e) a delta_apply of that list, forward and backward in turn on a third model, so that every repetition changes every listed voxel
      -- the kernel, then the full rebuild;
beside them a single-voxel set_voxels on that third model -- the rebuild's floor --, a Model.surface full list of `before`, and once the
host route: Model.read() of both, the two grids rebuilt with numpy, the witness of tests/delta_witness.py. The device's result, list and
tables are checked against that witness, byte for byte, before anything is timed.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 900 python tools/delta_timing.py).

    python tools/delta_timing.py [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from island_timing import blocks_to_grid  # noqa: E402
import delta_witness  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    one = api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal)
    results = {}

    def timed(name, call, extra=None):
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                ts.append(dt * 1e3)
        results[name] = {"ms_median": round(float(np.median(ts)), 4), "ms_p10": round(float(np.percentile(ts, 10)), 4),
                         "ms_p90": round(float(np.percentile(ts, 90)), 4), "reps": len(ts)}
        results[name].update(extra or {})
        print(name, results[name], flush=True)

    def terrain():
        m = api.Model(ctx, *one, pal)
        boxes = ([[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]])
        m.edit_shapes(api.edit_shapes(L.SHAPE_BOX, *boxes, op=L.EDIT_FILL, palette=[1, 2, 3]))
        return m

    def fill(seed, first_material):
        rng = np.random.default_rng(seed)
        m = api.Model(ctx, *one, pal)
        for x0 in range(0, 256, 32):          # 32 slabs' worth of coordinates per call
            xyz = np.argwhere(rng.random((32, 256, 256)) < 0.5).astype(np.uint32)
            xyz[:, 0] += x0
            m.set_voxels(xyz, np.full(len(xyz), first_material + x0 // 32, np.int32))
        return m

    def carved():
        m = terrain()
        print("carve:", int(m.edit_shapes(api.edit_shapes(L.SHAPE_SPHERE, [[128.0, 120.0, 128.0]], radius=24.0, op=L.EDIT_CARVE))[0]), "voxels", flush=True)
        return m

    pairs = (("terrain_carve", terrain, carved), ("half_density_reseeded", lambda: fill(7, 1), lambda: fill(8, 2)))
    for name, make_before, make_after in pairs:
        before, after, third = make_before(), make_after(), make_before()
        # the host route, stage by stage, once -- and the answer the device is held to
        host = {}

        def stage(what, call):
            t0 = time.perf_counter()
            out = call()
            host[what + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            return out
        read = stage("read_both", lambda: (before.read(), after.read()))
        grids = stage("blocks_to_grid_numpy_both", lambda: [blocks_to_grid(blocks, mats) for blocks, mats in read])
        want_result, want_voxels, want_counts = stage("delta_witness_numpy", lambda: delta_witness.delta(*grids))
        results[name + "_host_route_once"] = host
        print(name + "_host_route_once", host, flush=True)
        result, voxels, counts = before.delta(after, tables=True)
        assert result.tobytes() == want_result.tobytes() and voxels.tobytes() == want_voxels.tobytes() and np.array_equal(counts, want_counts), name
        n = len(voxels)
        extra = {key: int(result[key]) for key in ("voxels", "added", "removed", "repainted", "solid_before", "solid_after")}
        timed(name + "_a_counts_added_removed", lambda: before.delta(after, kinds=L.DELTA_ADDED | L.DELTA_REMOVED, capacity=0), extra)
        timed(name + "_b_counts_all", lambda: before.delta(after, capacity=0))
        timed(name + "_c_counts_all_with_tables", lambda: before.delta(after, capacity=0, tables=True))
        timed(name + "_d_full_list", lambda: before.delta(after), {"list_bytes": 8 * n})
        assert third.delta_apply(voxels) == (n, 0) and int(third.delta(after, capacity=0)[0]["voxels"]) == 0, name
        assert third.delta_apply(voxels, backward=True) == (n, 0) and int(third.delta(before, capacity=0)[0]["voxels"]) == 0, name
        turn = [False]

        def apply():
            assert third.delta_apply(voxels, backward=turn[0]) == (n, 0)
            turn[0] = not turn[0]
        timed(name + "_e_delta_apply_full_list", apply, {"records": n})
        timed(name + "_single_voxel_set_voxels", lambda: third.set_voxels([(10, 200, 10)], [1]))
        timed(name + "_surface_full_list", lambda: before.surface(), {"surface_voxels": int(before.surface(capacity=0)[0]["voxels"])})
        del before, after, third
    print(json.dumps(results))


if __name__ == "__main__":
    main()
