"""Model surfaces (dust_hip_model_surface, dust_hip_model_surface_apply) on three editable 256^3 models: the solid terrain block of
tools/shape_edit_timing.py (y < 128, three layers of material, 8.4 M voxels), a half-density random fill of the whole tree (8.4 M
voxels, nearly all of them on the surface) and the empty tree. Per model, on the same run:
  (a) counts only (no grid byte is read);
  (b) counts with the per-direction, per-material tables;
  (c) the full list (a count call, then a call with room for every voxel: what Model.surface(capacity=None) does);
  (d) a +y paint through surface_apply (the tops take a palette index; repainting painted tops changes nothing, so every repetition
      does the same work -- the kernel, then the full rebuild);
beside them a single-voxel set_voxels on the same model -- the rebuild's floor --, and once the host route: Model.read(), the grid
rebuilt with numpy, six shifted compares. The device's counts are checked against that route before anything is timed.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 600 python tools/surface_timing.py).

    python tools/surface_timing.py [--reps 20] [--warmup 3]
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
from island_timing import blocks_to_grid  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402


def host_faces(grid):
    """exposed faces per direction (-x, +x, -y, +y, -z, +z) and the voxels with at least one, with numpy"""
    solid = np.pad(grid != 0, 1)
    core = solid[1:-1, 1:-1, 1:-1]
    shown = [core & ~solid[:-2, 1:-1, 1:-1], core & ~solid[2:, 1:-1, 1:-1], core & ~solid[1:-1, :-2, 1:-1], core & ~solid[1:-1, 2:, 1:-1],
             core & ~solid[1:-1, 1:-1, :-2], core & ~solid[1:-1, 1:-1, 2:]]
    some = shown[0] | shown[1] | shown[2] | shown[3] | shown[4] | shown[5]
    return [int(np.count_nonzero(s)) for s in shown], int(np.count_nonzero(some))


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

    for name, model in (("terrain", terrain), ("half_density", half), ("empty", empty)):
        # the host route, stage by stage, once -- and the counts the device is held to
        host = {}

        def stage(what, call):
            t0 = time.perf_counter()
            out = call()
            host[what + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            return out
        blocks, mats = stage("read", model.read)
        grid = stage("blocks_to_grid_numpy", lambda: blocks_to_grid(blocks, mats))
        by_face, listed = stage("six_shifted_compares_numpy", lambda: host_faces(grid))
        results[name + "_host_route_once"] = host
        print(name + "_host_route_once", host, flush=True)
        result, voxels, counts = model.surface(tables=True)
        assert result["by_face"].tolist() == by_face and int(result["voxels"]) == listed == len(voxels), name
        assert int(counts.sum()) == int(result["faces"]) == sum(by_face) and int(result["solid"]) == np.count_nonzero(grid), name
        extra = {"solid": int(result["solid"]), "voxels": listed, "faces": sum(by_face)}
        timed(name + "_a_counts_only", lambda: model.surface(capacity=0), extra)
        timed(name + "_b_counts_with_tables", lambda: model.surface(capacity=0, tables=True))
        timed(name + "_c_full_list", lambda: model.surface(), {"list_bytes": 8 * listed})
        tops = model.surface(faces=L.FACE_POS_Y, capacity=0)[0]
        assert model.surface_apply(9, faces=L.FACE_POS_Y) == int(tops["voxels"]) == by_face[3], name
        timed(name + "_d_paint_tops_surface_apply", lambda: model.surface_apply(9, faces=L.FACE_POS_Y), {"tops": by_face[3]})
        timed(name + "_single_voxel_set_voxels", lambda: model.set_voxels([(10, 200, 10)], [1] if name != "empty" else [-1]))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
