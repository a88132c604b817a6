"""Model columns (dust_hip_model_columns, dust_hip_model_columns_apply) on three editable 256^3 models: the solid terrain block of
tools/shape_edit_timing.py (y < 128, three layers of material, 8.4 M voxels), a half-density random fill of the whole tree (8.4 M
voxels, about 64 runs in every column) and the empty tree. Per model, on the same run:
  (a) counts only from +y (no grid byte is read);
  (b) the full 256 x 256 map from +y, with the table;
  (c) the full map from +x, whose mask words lie a whole root-cell row apart;
  (d) a single-column query (one workgroup);
  (e) RUN 1 from +y: the top voxel of every column takes a palette index (repainting painted tops changes nothing, so every
      repetition does the same work -- the kernel, then the full rebuild);
  (f) GAP 1 from +y: a voxel of snow on every column under open sky; an untimed RUN 1 None takes it off again before the next one;
beside (a) a count-only Model.surface call, beside (e) and (f) a single-voxel set_voxels on the same model -- the rebuild's floor --,
and once the host route: Model.read(), the grid rebuilt with numpy, argmax along y. The device's map is checked against the witness
(tests/column_witness.py) and against that route before anything is timed.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 600 python tools/column_timing.py).

    python tools/column_timing.py [--reps 20] [--warmup 3]
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
import column_witness as W  # noqa: E402
from island_timing import blocks_to_grid  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402


def host_heights(grid):
    """per (x, z) the y of the topmost solid voxel and whether there is one, with numpy"""
    solid = grid != 0
    top = 255 - np.argmax(solid[:, ::-1, :], axis=1)
    return top, solid.any(axis=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    one = api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal)
    results = {}

    def timed(name, call, extra=None, between=None):
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if between:
                between()
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
        # the host route, stage by stage, once -- and the map the device is held to
        host = {}

        def stage(what, call):
            t0 = time.perf_counter()
            out = call()
            host[what + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            return out
        blocks, mats = stage("read", model.read)
        grid = stage("blocks_to_grid_numpy", lambda: blocks_to_grid(blocks, mats))
        top, any_solid = stage("argmax_numpy", lambda: host_heights(grid))
        results[name + "_host_route_once"] = host
        print(name + "_host_route_once", host, flush=True)
        for face in (L.FACE_POS_Y, L.FACE_POS_X):
            result, cells, counts = model.columns(face, tables=True)
            want = W.columns(grid, face)
            assert result.tobytes() == want[0].tobytes() and cells.tobytes() == want[1].tobytes() and np.array_equal(counts, want[2]), (name, face)
        result, cells, counts = model.columns(L.FACE_POS_Y, tables=True)
        assert np.array_equal(cells["palette"] != 255, any_solid) and np.array_equal(cells["at"][any_solid], top[any_solid]), name
        extra = {"hit": int(result["hit"]), "runs": int(result["runs"]), "voxels": int(result["voxels"])}
        timed(name + "_a_counts_only_pos_y", lambda: model.columns(L.FACE_POS_Y, cells=False), extra)
        timed(name + "_surface_counts_only", lambda: model.surface(capacity=0))
        timed(name + "_b_full_map_pos_y", lambda: model.columns(L.FACE_POS_Y, tables=True), {"map_bytes": 4 * cells.size})
        timed(name + "_c_full_map_pos_x", lambda: model.columns(L.FACE_POS_X, tables=True))
        timed(name + "_d_single_column", lambda: model.columns(L.FACE_POS_Y, region=((100, 0, 100), (100, 255, 100))))
        tops = int(result["hit"])
        assert model.columns_apply(9, L.FACE_POS_Y) == tops, name
        timed(name + "_e_run_1_columns_apply", lambda: model.columns_apply(9, L.FACE_POS_Y), {"tops": tops})
        open_sky = int(np.count_nonzero(any_solid & (top < 255)))      # (a column that reaches y = 255 has no gap in front of its first run)
        assert model.columns_apply(10, L.FACE_POS_Y, where=L.COLUMNS_GAP) == open_sky, name
        assert model.columns_apply(-1, L.FACE_POS_Y, palette=10) == open_sky, name
        timed(name + "_f_gap_1_columns_apply", lambda: model.columns_apply(10, L.FACE_POS_Y, where=L.COLUMNS_GAP), {"open_sky": open_sky},
              between=lambda: model.columns_apply(-1, L.FACE_POS_Y, palette=10))
        timed(name + "_single_voxel_set_voxels", lambda: model.set_voxels([(10, 200, 10)], [1] if name != "empty" else [-1]))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
