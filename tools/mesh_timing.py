"""Model meshes (dust_hip_model_mesh) on four editable 256^3 models: the solid terrain block of tools/shape_edit_timing.py (y < 128,
three layers of material, 8.4 M voxels), a half-density random fill of the whole tree (8.4 M voxels, nearly all of them on the
surface), the empty tree and the full tree. Per model, on the same run:
  (a) counts only (capacity 0), with and without ANY_PALETTE (with it no grid byte is read);
  (b) the full list (a count call, then a call with room for every quad: what Model.mesh(capacity=None) does), with and without
      ANY_PALETTE;
  (c) Model.surface's full list -- the yardstick: the device work the host route needs before it can start merging;
beside the timings the number of quads next to the number of surface voxels and faces (the compression the call buys), and once the
host route: Model.read(), the grid rebuilt with numpy, the witness of tests/mesh_witness.py. The device's result and list are checked
against that witness, byte for byte, before anything is timed.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 900 python tools/mesh_timing.py).

    python tools/mesh_timing.py [--reps 20] [--warmup 3]
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
import mesh_witness  # noqa: E402
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

    terrain = api.Model(ctx, *one, pal)
    boxes = ([[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]])
    print("terrain:", int(terrain.edit_shapes(api.edit_shapes(L.SHAPE_BOX, *boxes, op=L.EDIT_FILL, palette=[1, 2, 3])).sum()), "voxels", flush=True)
    rng = np.random.default_rng(7)
    half = api.Model(ctx, *one, pal)
    for x0 in range(0, 256, 32):          # 32 slabs' worth of coordinates per call
        xyz = np.argwhere(rng.random((32, 256, 256)) < 0.5).astype(np.uint32)
        xyz[:, 0] += x0
        half.set_voxels(xyz, np.full(len(xyz), 1 + x0 // 32, np.int32))
    empty = api.Model(ctx, *one, pal)
    empty.set_voxels([(0, 0, 0)], [-1])
    full = api.Model(ctx, *one, pal)
    full.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0]], [[256, 256, 256]], op=L.EDIT_FILL, palette=[5]))

    for name, model in (("terrain", terrain), ("half_density", half), ("empty", empty), ("full", full)):
        # the host route, stage by stage, once -- and the bytes the device is held to
        host = {}

        def stage(what, call):
            t0 = time.perf_counter()
            out = call()
            host[what + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            return out
        blocks, mats = stage("read", model.read)
        grid = stage("blocks_to_grid_numpy", lambda: blocks_to_grid(blocks, mats))
        want_result, want_quads = stage("mesh_witness_numpy", lambda: mesh_witness.mesh(grid))
        results[name + "_host_route_once"] = host
        print(name + "_host_route_once", host, flush=True)
        result, quads = model.mesh()
        assert result.tobytes() == want_result.tobytes() and quads.tobytes() == want_quads.tobytes(), name
        merged, merged_quads = model.mesh(any_palette=True)
        want_merged, want_merged_quads = mesh_witness.mesh(grid, any_palette=True)
        assert merged.tobytes() == want_merged.tobytes() and merged_quads.tobytes() == want_merged_quads.tobytes(), name
        surface, voxels, _ = model.surface()
        assert result["faces_by_face"].tolist() == surface["by_face"].tolist() == merged["faces_by_face"].tolist(), name
        extra = {"surface_voxels": int(surface["voxels"]), "faces": int(result["faces"]), "quads": int(result["quads"]),
                 "quads_any_palette": int(merged["quads"]), "largest": int(result["largest"]), "largest_any_palette": int(merged["largest"])}
        timed(name + "_a_counts_only", lambda: model.mesh(capacity=0), extra)
        timed(name + "_a_counts_only_any_palette", lambda: model.mesh(capacity=0, any_palette=True))
        timed(name + "_b_full_list", lambda: model.mesh(), {"list_bytes": 8 * int(result["quads"])})
        timed(name + "_b_full_list_any_palette", lambda: model.mesh(any_palette=True), {"list_bytes": 8 * int(merged["quads"])})
        timed(name + "_c_surface_full_list", lambda: model.surface(), {"list_bytes": 8 * len(voxels)})
    print(json.dumps(results))


if __name__ == "__main__":
    main()
