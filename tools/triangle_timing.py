"""Model voxelisation (dust_hip_model_edit_triangles, dust_hip_model_fill_mesh) on the solid terrain block of tools/shape_edit_timing.py
(y < 128, three layers of material, 8.4 M voxels), its top roughened by 1 500 small craters so that its own mesh is large. On the same run:
  (a) one triangle (a few voxels wide, across a root-cell edge);
  (b) 4 096 small triangles scattered over the block's top;
  (c) one triangle whose bounds are the whole tree (the plane x = z where y <= x);
  (d) fill_mesh of the block's own mesh (Model.mesh -> api.quads_to_triangles: a closed mesh of about 100 k triangles) into an empty
      model;
beside a single-voxel set_voxels on the same block -- the rebuild's floor --, and once each the host route: the witness
(tests/triangle_witness.py) and set_voxels of the voxels it changed. Every timed call starts from the same voxels: between two of them a
pristine twin is stamped back over the whole tree (untimed). The device's counts, records and models are checked against the witness
before anything is timed ((d) against the block's own voxels and the witness's inside test).
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 900 python tools/triangle_timing.py).

    python tools/triangle_timing.py [--reps 20] [--warmup 3]
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
import triangle_witness as W  # noqa: E402
from island_timing import blocks_to_grid  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402

U = L.TRIANGLE_UNIT


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    one = api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal)
    rng = np.random.default_rng(7)
    results = {}

    def timed(name, call, extra=None, between=None):
        ts = []
        for k in range(args.warmup + args.reps):
            if between:
                between()
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                ts.append(dt * 1e3)
        results[name] = {"ms_median": round(float(np.median(ts)), 4), "ms_p10": round(float(np.percentile(ts, 10)), 4),
                         "ms_p90": round(float(np.percentile(ts, 90)), 4), "reps": len(ts)}
        results[name].update(extra or {})
        print(name, results[name], flush=True)

    craters = api.edit_shapes(L.SHAPE_SPHERE, np.stack([rng.uniform(4, 252, 1500), rng.uniform(126, 129, 1500), rng.uniform(4, 252, 1500)], axis=1),
                              radius=rng.uniform(2.0, 5.0, 1500), op=L.EDIT_CARVE)

    def terrain():
        m = api.Model(ctx, *one, pal)
        boxes = ([[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]])
        m.edit_shapes(api.edit_shapes(L.SHAPE_BOX, *boxes, op=L.EDIT_FILL, palette=[1, 2, 3]))
        m.edit_shapes(craters)
        return m

    model, pristine = terrain(), terrain()
    empty = api.Model(ctx, *one, pal)
    empty.set_voxels([(0, 0, 0)], [-1])
    blank = api.Model(ctx, *one, pal)
    blank.set_voxels([(0, 0, 0)], [-1])

    def restore():
        model.stamp(pristine, api.stamps((0, 0, 0), op=L.STAMP_REPLACE))

    def clear():
        empty.stamp(blank, api.stamps((0, 0, 0), op=L.STAMP_REPLACE))

    grid = blocks_to_grid(*model.read())
    single = W.triangles([[(60 * U + 40, 126 * U, 62 * U), (67 * U, 131 * U + 9, 63 * U + 100), (63 * U, 127 * U, 69 * U + 200)]], W.FILL, 9)
    at = np.stack([rng.uniform(2, 250, 4096), rng.uniform(124, 130, 4096), rng.uniform(2, 250, 4096)], axis=1)
    small = api.triangles(at[:, None, :] + rng.uniform(-1.5, 1.5, (4096, 3, 3)), rng.integers(0, 4, 4096), rng.integers(0, 255, 4096))
    whole = W.triangles([[(0, 0, 0), (256 * U, 256 * U, 256 * U), (256 * U, 0, 256 * U)]], W.PAINT, 11)
    _, quads = model.mesh(any_palette=True)
    mesh = api.quads_to_triangles(quads)
    results["mesh"] = {"quads": len(quads), "triangles": len(mesh), "voxels": int(np.count_nonzero(grid))}
    print("mesh", results["mesh"], flush=True)

    # the host route, once each -- and the grids the device is held to
    host = {}

    def stage(what, call):
        t0 = time.perf_counter()
        out = call()
        host[what + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        return out
    for name, tris in (("one_triangle", single), ("small_4096", small), ("whole_tree", whole)):
        after = grid.copy()
        want = stage(name + "_witness", lambda: W.edit_triangles(after, tris))
        changed = np.argwhere(after != grid).astype(np.uint32)
        twin = terrain()
        stage(name + "_set_voxels_of_the_changed", lambda: twin.set_voxels(changed, after[tuple(changed.T)].astype(np.int32) - 1))
        host[name + "_changed_voxels"] = len(changed)
        got = model.edit_triangles(tris)
        assert got.tolist() == want.tolist(), name
        assert np.array_equal(blocks_to_grid(*model.read()), after) and np.array_equal(blocks_to_grid(*twin.read()), after), name
        restore()
    assert np.array_equal(blocks_to_grid(*model.read()), grid)                        # the restore between two timed edits works
    inside = stage("mesh_witness_inside", lambda: W.inside(mesh))
    assert np.array_equal(inside, grid != 0)                                          # the round trip, in the witness
    solid = np.argwhere(inside).astype(np.uint32)
    stage("mesh_set_voxels_of_the_inside", lambda: empty.set_voxels(solid, np.full(len(solid), 5, np.int32)))
    clear()
    r = empty.fill_mesh(mesh, L.EDIT_FILL, 5)
    assert int(r["covered"]) == int(r["changed"]) == len(solid) and int(r["live"]) == len(mesh)
    assert np.array_equal(blocks_to_grid(*empty.read()), np.where(grid != 0, 6, 0).astype(np.uint8))
    results["fill_mesh_record"] = {k: int(r[k]) for k in ("covered", "changed", "live", "crossing")}
    results["host_route_once"] = host
    print("host_route_once", host, flush=True)

    timed("a_one_triangle", lambda: model.edit_triangles(single), between=restore)
    timed("b_4096_small_triangles", lambda: model.edit_triangles(small), between=restore)
    timed("c_whole_tree_triangle", lambda: model.edit_triangles(whole), between=restore)
    timed("d_fill_mesh_of_the_blocks_own_mesh", lambda: empty.fill_mesh(mesh, L.EDIT_FILL, 5), extra={"triangles": len(mesh)}, between=clear)
    timed("d_fill_mesh_over_itself_nothing_changes", lambda: model.fill_mesh(mesh, L.EDIT_PLACE, 5), extra={"triangles": len(mesh)})
    restore()
    timed("single_voxel_set_voxels", lambda: model.set_voxels([(10, 200, 10)], [1]))
    timed("single_voxel_set_voxels_empty_model", lambda: empty.set_voxels([(10, 200, 10)], [1]))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
