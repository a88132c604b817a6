"""Model reductions (dust_hip_model_reduce) on the solid terrain block of tools/island_timing.py (y < 128, three layers of material,
8.4 M voxels, a pillar on it), an editable 256^3 model:
  (a) reduce at levels 1, 2 and 3 with min_solid 1 (the new model is destroyed, untimed, after every call);
  (b) the same at level 1 from a copy of the terrain that is NOT editable (the source is expanded into the context's scratch first);
beside, on the same run, a single-voxel set_voxels (the rebuild's floor), a KEEP_SOURCE detach_islands of the whole terrain (another
call that makes a model and rebuilds it) and the host route for level 1, each stage once: Model.read(), the grid rebuilt with numpy,
the vote with numpy, flatten_model and Model(...).
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 600 python tools/reduce_timing.py).

    python tools/reduce_timing.py [--reps 20] [--warmup 3]
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


def vote(grid, min_solid=1):
    """one level on the host: the coarse voxel takes the byte most of its solid children carry, the lowest among equals"""
    n = grid.shape[0] // 2
    kids = grid.reshape(n, 2, n, 2, n, 2).transpose(0, 2, 4, 1, 3, 5).reshape(n, n, n, 8).astype(np.int16)
    same = np.zeros(kids.shape, np.int16)
    for j in range(8):
        same += kids == kids[..., j:j + 1]
    key = np.where(kids != 0, same * 256 + (255 - kids), 0).max(axis=-1)
    return np.where(np.count_nonzero(kids, axis=-1) >= min_solid, 255 - (key & 255), 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    one = api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal)
    model = api.Model(ctx, *one, pal)
    build = api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 96, 0], [0, 120, 0], [100, 128, 90]],
                            [[256, 96, 256], [256, 120, 256], [256, 128, 256], [120, 200, 110]], op=L.EDIT_FILL, palette=[1, 2, 3, 4])
    print("terrain:", int(model.edit_shapes(build).sum()), "voxels", flush=True)
    results = {}

    def timed(name, call, extra=None):
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            made = call(k)
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                ts.append(dt * 1e3)
            del made      # (a new model goes here, outside the clock)
        results[name] = {"ms_median": round(float(np.median(ts)), 4), "ms_p10": round(float(np.percentile(ts, 10)), 4),
                         "ms_p90": round(float(np.percentile(ts, 90)), 4), "reps": len(ts)}
        results[name].update(extra or {})
        print(name, results[name], flush=True)

    def record(r):
        return {k: int(r[k]) for k in ("src_voxels", "voxels", "extent")}

    timed("single_voxel_set_voxels", lambda k: model.set_voxels([(10, 100, 10)], [k % 2]))
    model.set_voxels([(10, 100, 10)], [2])      # as it was
    n, islands = model.find_islands(L.ISLANDS_FACES)
    timed("detach_islands_keep_source_whole_terrain", lambda k: model.detach_islands(islands["key"], keep_source=True), extra={"islands": n})
    for levels in (1, 2, 3):
        timed(f"a_reduce_levels_{levels}_min_solid_1", lambda k: model.reduce(levels, 1), extra=record(model.reduce(levels, 1)[1]))

    blocks, mats = model.read()
    fixed = api.Model(ctx, blocks, mats, pal)
    timed("b_reduce_levels_1_source_not_editable", lambda k: fixed.reduce(1, 1), extra=record(fixed.reduce(1, 1)[1]))

    # the host route for level 1, stage by stage
    host = {}

    def stage(name, call):
        t0 = time.perf_counter()
        out = call()
        host[name + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        return out

    blocks, mats = stage("read", model.read)
    grid = stage("blocks_to_grid_numpy", lambda: blocks_to_grid(blocks, mats))
    coarse = stage("vote_numpy", lambda: vote(grid))
    xyz = np.argwhere(coarse != 0)
    xyzi = np.stack([xyz[:, 0], 255 - xyz[:, 2], xyz[:, 1], coarse[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int64) - 1], axis=1).astype(np.uint8)
    flat = stage("flatten_model", lambda: api.flatten_model(xyzi, (256, 256, 256), pal))
    built = stage("model_create", lambda: api.Model(ctx, *flat, pal))
    host["total_ms"] = round(sum(host.values()), 2)
    same = all(x.tobytes() == y.tobytes() for x, y in zip(built.read(), model.reduce(1, 1)[0].read()))
    host["same_bytes_as_reduce"] = bool(same)
    results["host_route_once"] = host
    print("host_route_once", host, flush=True)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
