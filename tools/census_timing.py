"""Model censuses (dust_hip_model_census) on the solid terrain block of tools/shape_edit_timing.py (y < 128, three layers of material,
8.4 M voxels), an editable 256^3 model:
  (a) one radius-24 sphere, records and tables;
  (b) 4 096 radius-2 spheres in one call, records and tables;
  (c) 65 536 radius-2 spheres in one call, records only;
  (d) the whole-tree box, records and tables;
  (e) (a) on a copy of the terrain that is NOT editable (the model is expanded into the context's scratch grid first);
beside each, on the same run, edit_shapes CARVE of the same shapes (the terrain put back, untimed, after every call) -- the call a census
precedes, which ends with the full rebuild --, and once the host route: Model.read(), the grid rebuilt with numpy, and the counts with
numpy for (a) and (d). Every device answer is checked against that grid before anything is timed.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 600 python tools/census_timing.py).

    python tools/census_timing.py [--reps 20] [--warmup 3]
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


def sphere_counts(grid, centre, radius):
    """covered, solid and the row of one sphere with numpy (float64: the tool's spheres have no voxel centre near their surface)"""
    lo = np.maximum(np.floor(np.asarray(centre) - radius - 1).astype(int), 0)
    hi = np.minimum(np.ceil(np.asarray(centre) + radius + 1).astype(int), 256)
    ax = [np.arange(l, h) + 0.5 - c for l, h, c in zip(lo, hi, centre)]
    m = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2 <= radius * radius
    row = np.bincount(grid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][m], minlength=256)
    return int(m.sum()), int(m.sum() - row[0]), row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    model = api.Model(ctx, *api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal), pal)
    boxes = ([[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]])
    layers = api.edit_shapes(L.SHAPE_BOX, *boxes, op=L.EDIT_FILL, palette=[1, 2, 3])
    restore = api.edit_shapes(L.SHAPE_BOX, *boxes, op=L.EDIT_PLACE, palette=[1, 2, 3])
    print("terrain:", int(model.edit_shapes(layers).sum()), "voxels", flush=True)
    results = {}

    def timed(name, call, undo=None, extra=None):
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                ts.append(dt * 1e3)
            if undo is not None:
                undo()
        results[name] = {"ms_median": round(float(np.median(ts)), 4), "ms_p10": round(float(np.percentile(ts, 10)), 4),
                         "ms_p90": round(float(np.percentile(ts, 90)), 4), "reps": len(ts)}
        results[name].update(extra or {})
        print(name, results[name], flush=True)

    put_back = lambda: model.edit_shapes(restore)  # noqa: E731
    rng = np.random.default_rng(9)

    def small(n):
        return api.edit_shapes(L.SHAPE_SPHERE, np.stack([rng.uniform(4, 252, n), rng.uniform(4, 124, n), rng.uniform(4, 252, n)], axis=1), radius=2.03)
    cases = [("a_sphere24", api.edit_shapes(L.SHAPE_SPHERE, [128.3, 110.4, 128.6], radius=24.02), True),
             ("b_4096_spheres2", small(4096), True),
             ("c_65536_spheres2", small(65536), False),
             ("d_whole_tree_box", api.edit_shapes(L.SHAPE_BOX, [0, 0, 0], [256, 256, 256]), True)]

    # the host route, stage by stage, once -- and the grid every device answer is held to
    host = {}

    def stage(name, call):
        t0 = time.perf_counter()
        out = call()
        host[name + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        return out
    blocks, mats = stage("read", model.read)
    grid = stage("blocks_to_grid_numpy", lambda: blocks_to_grid(blocks, mats))
    crater = cases[0][1][0]
    want_crater = stage("sphere24_counts_numpy", lambda: sphere_counts(grid, crater["a"].astype(np.float64), float(crater["radius"])))
    want_whole = stage("whole_tree_counts_numpy", lambda: np.bincount(grid.reshape(-1), minlength=256))
    results["host_route_once"] = host
    print("host_route_once", host, flush=True)

    for name, shapes, tables in cases:
        records, counts = model.census(shapes, tables=tables)
        changed = model.edit_shapes(shapes)      # CARVE: overlapping spheres remove a voxel once, so the sum is at most the census's
        put_back()
        assert int(changed[0]) == int(records["solid"][0]) and int(changed.sum()) <= int(records["solid"].sum()), name
        if name == "a_sphere24":
            assert (int(records["covered"][0]), int(records["solid"][0])) == want_crater[:2] and np.array_equal(counts[0], want_crater[2]), name
        if name == "d_whole_tree_box":
            assert np.array_equal(counts[0], want_whole) and int(records["covered"][0]) == 1 << 24, name
        extra = {"shapes": len(shapes), "tables": tables, "covered": int(records["covered"].sum()), "solid": int(records["solid"].sum())}
        timed(name + "_census", lambda: model.census(shapes, tables=tables), None, extra)
        if tables and len(shapes) > 1:
            timed(name + "_census_records_only", lambda: model.census(shapes, tables=False))
        timed(name + "_edit_shapes_carve", lambda: model.edit_shapes(shapes), put_back, {"voxels_changed": int(changed.sum())})

    fixed = api.Model(ctx, blocks, mats, pal)
    records, counts = fixed.census(cases[0][1])
    assert int(records["solid"][0]) == want_crater[1] and np.array_equal(counts[0], want_crater[2])
    timed("e_sphere24_census_model_not_editable", lambda: fixed.census(cases[0][1]))
    timed("single_voxel_set_voxels", lambda: model.set_voxels([(10, 200, 10)], [1]))      # the rebuild's floor, for scale
    print(json.dumps(results))


if __name__ == "__main__":
    main()
