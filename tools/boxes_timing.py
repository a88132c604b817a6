"""Model boxes (dust_hip_model_boxes) on five editable 256^3 models: the solid terrain block of tools/mesh_timing.py (y < 128, three
layers of material, 8.4 M voxels), the same block with a radius-24 crater carved into its top, a half-density random fill of the whole
tree (8.4 M voxels), the full tree and the empty tree. Per model, on the same run:
  (a) counts only (capacity 0), with and without ANY_PALETTE (with it no grid byte is read);
  (b) the full list (a count call, then a call with room for every box: what Model.boxes(capacity=None) does), with and without
      ANY_PALETTE and for each stacking axis;
  (c) the yardsticks: Model.mesh's full list and a count-only Model.surface;
beside the timings the number of boxes and rects next to the number of voxels (the compression the call buys), and once the host
route: Model.read(), the grid rebuilt with numpy, the witness of tests/boxes_witness.py. The device's result and list are checked
against that witness, byte for byte, for every axis and both flag values, before anything is timed.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 900 python tools/boxes_timing.py).

    python tools/boxes_timing.py [--reps 20] [--warmup 3]
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
import boxes_witness  # noqa: E402
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

    layers = ([[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]])
    terrain = api.Model(ctx, *one, pal)
    print("terrain:", int(terrain.edit_shapes(api.edit_shapes(L.SHAPE_BOX, *layers, op=L.EDIT_FILL, palette=[1, 2, 3])).sum()), "voxels", flush=True)
    crater = api.Model(ctx, *one, pal)
    crater.edit_shapes(api.edit_shapes(L.SHAPE_BOX, *layers, op=L.EDIT_FILL, palette=[1, 2, 3]))
    print("crater:", int(crater.edit_shapes(api.edit_shapes(L.SHAPE_SPHERE, [[128.5, 127.5, 128.5]], radius=24.0, op=L.EDIT_CARVE)).sum()), "voxels carved", flush=True)
    rng = np.random.default_rng(7)
    half = api.Model(ctx, *one, pal)
    for x0 in range(0, 256, 32):          # 32 slabs' worth of coordinates per call
        xyz = np.argwhere(rng.random((32, 256, 256)) < 0.5).astype(np.uint32)
        xyz[:, 0] += x0
        half.set_voxels(xyz, np.full(len(xyz), 1 + x0 // 32, np.int32))
    full = api.Model(ctx, *one, pal)
    full.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0]], [[256, 256, 256]], op=L.EDIT_FILL, palette=[5]))
    empty = api.Model(ctx, *one, pal)
    empty.set_voxels([(0, 0, 0)], [-1])

    for name, model in (("terrain", terrain), ("crater", crater), ("half_density", half), ("full", full), ("empty", empty)):
        # the host route, stage by stage, once -- and the bytes the device is held to
        host = {}

        def stage(what, call):
            t0 = time.perf_counter()
            out = call()
            host[what + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            return out
        blocks, mats = stage("read", model.read)
        grid = stage("blocks_to_grid_numpy", lambda: blocks_to_grid(blocks, mats))
        stage("boxes_witness_numpy", lambda: boxes_witness.boxes(grid))
        results[name + "_host_route_once"] = host
        print(name + "_host_route_once", host, flush=True)
        counts = {}
        for axis in range(3):
            for any_palette in (False, True):
                result, boxes = model.boxes(axis=axis, any_palette=any_palette)
                want_result, want_boxes = boxes_witness.boxes(grid, axis=axis, any_palette=any_palette)
                assert result.tobytes() == want_result.tobytes() and boxes.tobytes() == want_boxes.tobytes(), (name, axis, any_palette)
                counts[f"boxes_axis{axis}" + ("_any_palette" if any_palette else "")] = int(result["boxes"])
                counts[f"rects_axis{axis}" + ("_any_palette" if any_palette else "")] = int(result["rects"])
        surface = model.surface(capacity=0)[0]
        assert int(surface["solid"]) == int(result["voxels"]), name
        counts["voxels"] = int(result["voxels"])
        timed(name + "_a_counts_only", lambda: model.boxes(capacity=0), counts)
        timed(name + "_a_counts_only_any_palette", lambda: model.boxes(capacity=0, any_palette=True))
        for axis in range(3):
            timed(f"{name}_b_full_list_axis{axis}", lambda: model.boxes(axis=axis), {"list_bytes": 8 * counts[f"boxes_axis{axis}"]})
            timed(f"{name}_b_full_list_axis{axis}_any_palette", lambda: model.boxes(axis=axis, any_palette=True),
                  {"list_bytes": 8 * counts[f"boxes_axis{axis}_any_palette"]})
        timed(name + "_c_mesh_full_list", lambda: model.mesh())
        timed(name + "_c_surface_counts_only", lambda: model.surface(capacity=0))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
