"""Model distances (dust_hip_model_distance / distance_apply) on editable 256^3 models:
on the solid terrain block of tools/island_timing.py (y < 128, three layers of material, 8.4 M voxels, a pillar on it)
  (a) TO_EMPTY + WALLS at R = 255: thickness, how deep inside the solid every voxel is;
  (b) TO_SOLID at R = 4;
  (c) distance_apply of a TO_SOLID field at R = 2, range 1..4: grow by 2 (the field is computed untimed before every call; undone,
      untimed, by carving everything above the ground and filling the pillar again);
on an empty tree
  (d) TO_SOLID at R = 255, without and with WALLS: no target anywhere, every line is skipped by its wave vote;
  (f) the same with one voxel in a corner, and (g) with one line of voxels along y: the long scans;
on a half-density random fill of the whole tree
  (e) TO_SOLID at R = 255;
beside, on the same run, a single-voxel set_voxels (the rebuild's floor) and the host route for (c): Model.read(), the grid rebuilt
with numpy, scipy.ndimage.distance_transform_edt over 256^3 (where scipy is installed) and the set_voxels call that writes the grown
voxels. An untimed edit that covers nothing invalidates the field before every timed distance call.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 600 python tools/distance_timing.py).

    python tools/distance_timing.py [--reps 20] [--warmup 3]
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

    def timed(name, call, undo=None, extra=None, before=None):
        ts = []
        for k in range(args.warmup + args.reps):
            if before is not None:
                before()
            t0 = time.perf_counter()
            call(k)
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                ts.append(dt * 1e3)
            if undo is not None:
                undo()
        results[name] = {"ms_median": round(float(np.median(ts)), 4), "ms_p10": round(float(np.percentile(ts, 10)), 4),
                         "ms_p90": round(float(np.percentile(ts, 90)), 4), "reps": len(ts)}
        results[name].update(extra or {})
        print(name, results[name], flush=True)

    def record(r):
        return {k: int(r[k]) for k in ("targets", "near", "far", "largest", "largest_key")}

    nothing = api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0])

    def invalidate(m):
        return lambda: m.edit_shapes(nothing)

    timed("single_voxel_set_voxels", lambda k: model.set_voxels([(10, 100, 10)], [k % 2]))
    model.set_voxels([(10, 100, 10)], [2])      # as it was
    timed("noop_edit_shapes", lambda k: model.edit_shapes(nothing))

    thickness = dict(target=L.DISTANCE_TO_EMPTY, max_radius=255, walls=True)
    timed("a_terrain_to_empty_walls_r255", lambda k: model.distance(**thickness), before=invalidate(model), extra=record(model.distance(**thickness)))
    near = dict(target=L.DISTANCE_TO_SOLID, max_radius=4)
    timed("b_terrain_to_solid_r4", lambda k: model.distance(**near), before=invalidate(model), extra=record(model.distance(**near)))
    grow = dict(target=L.DISTANCE_TO_SOLID, max_radius=2)
    r = model.distance(**grow)
    restore = api.edit_shapes(L.SHAPE_BOX, [[0, 128, 0], [100, 128, 90]], [[256, 256, 256], [120, 200, 110]], op=[L.EDIT_CARVE, L.EDIT_FILL], palette=[0, 4])
    changed = []
    timed("c_terrain_grow_by_2_apply", lambda k: changed.append(model.distance_apply(5, 1, 4)), undo=lambda: model.edit_shapes(restore),
          before=lambda: model.distance(**grow), extra=record(r))
    assert set(changed) == {int(r["near"])}, (set(changed), r)

    # the host route for (c)
    t0 = time.perf_counter()
    blocks, mats = model.read()
    host = {"read_ms": round((time.perf_counter() - t0) * 1e3, 2)}
    t0 = time.perf_counter()
    grid = blocks_to_grid(blocks, mats)
    host["blocks_to_grid_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    try:
        from scipy import ndimage
        t0 = time.perf_counter()
        squared = np.rint(ndimage.distance_transform_edt(grid == 0) ** 2).astype(np.int64)
        host["scipy_edt_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        xyz = np.argwhere((squared >= 1) & (squared <= 4)).astype(np.uint32)
        assert len(xyz) == int(r["near"]), (len(xyz), r)
    except ImportError:
        host["scipy_edt_ms"] = None
        model.distance(**grow)
        every = np.stack(np.meshgrid(np.arange(256), np.arange(126, 204), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 3)
        values = model.distance_at(every)
        xyz = every[(values >= 1) & (values <= 4)].astype(np.uint32)
    fill, clear = np.full(len(xyz), 5, np.int32), np.full(len(xyz), -1, np.int32)
    timed("host_route_set_voxels_grow_by_2", lambda k: model.set_voxels(xyz, fill), undo=lambda: model.set_voxels(xyz, clear), extra={"entries": len(xyz)})
    results["host_route_once"] = host
    print("host_route_once", host, flush=True)

    empty = api.Model(ctx, *one, pal)
    empty.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [0, 0, 0], [256, 256, 256]))
    whole = dict(target=L.DISTANCE_TO_SOLID, max_radius=255)
    timed("d_empty_tree_to_solid_r255", lambda k: empty.distance(**whole), before=invalidate(empty), extra=record(empty.distance(**whole)))
    timed("d_empty_tree_to_solid_r255_walls", lambda k: empty.distance(walls=True, **whole), before=invalidate(empty),
          extra=record(empty.distance(walls=True, **whole)))
    empty.set_voxels([(0, 0, 0)], [1])
    timed("f_one_voxel_to_solid_r255", lambda k: empty.distance(**whole), before=invalidate(empty), extra=record(empty.distance(**whole)))
    # one line of targets along y at x = z = 0: long scans (a line of pass y holds x^2 throughout and walks x steps, pass z looks for z = 0)
    empty.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [0, 0, 0], [1, 256, 1], op=L.EDIT_FILL, palette=1))
    timed("g_one_line_of_voxels_to_solid_r255", lambda k: empty.distance(**whole), before=invalidate(empty), extra=record(empty.distance(**whole)))

    rng = np.random.default_rng(7)
    half = api.Model(ctx, *one, pal)
    for x0 in range(0, 256, 32):          # 32 slabs' worth of coordinates per call
        xyz = np.argwhere(rng.random((32, 256, 256)) < 0.5).astype(np.uint32)
        xyz[:, 0] += x0
        half.set_voxels(xyz, np.full(len(xyz), 1 + x0 // 32, np.int32))
    timed("e_half_density_to_solid_r255", lambda k: half.distance(**whole), before=invalidate(half), extra=record(half.distance(**whole)))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
