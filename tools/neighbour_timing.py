"""Model neighbourhoods (dust_hip_model_neighbours, dust_hip_model_neighbours_apply) on three editable 256^3 models: the solid terrain
block of tools/shape_edit_timing.py (y < 128, three layers of material, 8.4 M voxels), a half-density random fill of the whole tree
(8.4 M voxels) and the empty tree (one voxel). Per model, on the same run:
  (a) the read-only call without and with the table, for each of the three neighbourhoods (the masks are all it reads);
  (b) one generation and eight generations of the cave rule (26 neighbours, birth 14..26, survive 13..26) with a fixed palette;
  (c) one generation of the same rule under MAJORITY;
beside (a) a count-only Model.surface call, beside (b) and (c) a single-voxel set_voxels on the same model -- the rebuild's floor --, and
once the host route: Model.read(), the grid rebuilt with numpy and the 26 shifted sums. Every timed apply starts from the same voxels:
between two of them a pristine twin is stamped back over the whole tree (untimed). The device's histogram, its result
and the model one generation leaves are checked against the witness (tests/neighbour_witness.py) before anything is timed.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 900 python tools/neighbour_timing.py).

    python tools/neighbour_timing.py [--reps 20] [--warmup 3]
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
import neighbour_witness as W  # noqa: E402
from island_timing import blocks_to_grid  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402

CAVE = (api.count_mask((14, 26)), api.count_mask((13, 26)))


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

    def terrain_model():
        m = api.Model(ctx, *one, pal)
        boxes = ([[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]])
        m.edit_shapes(api.edit_shapes(L.SHAPE_BOX, *boxes, op=L.EDIT_FILL, palette=[1, 2, 3]))
        return m

    def half_model():
        rng = np.random.default_rng(7)
        m = api.Model(ctx, *one, pal)
        for x0 in range(0, 256, 32):          # 32 slabs' worth of coordinates per call
            xyz = np.argwhere(rng.random((32, 256, 256)) < 0.5).astype(np.uint32)
            xyz[:, 0] += x0
            m.set_voxels(xyz, np.full(len(xyz), 1 + x0 // 32, np.int32))
        return m

    def empty_model():
        m = api.Model(ctx, *one, pal)
        m.set_voxels([(0, 0, 0)], [-1])
        return m

    for name, build in (("terrain", terrain_model), ("half_density", half_model), ("empty", empty_model)):
        model, pristine = build(), build()

        def restore():
            model.stamp(pristine, api.stamps((0, 0, 0), op=L.STAMP_REPLACE))

        # the host route, stage by stage, once -- and the grid the device is held to
        host = {}

        def stage(what, call):
            t0 = time.perf_counter()
            out = call()
            host[what + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            return out
        blocks, mats = stage("read", model.read)
        grid = stage("blocks_to_grid_numpy", lambda: blocks_to_grid(blocks, mats))
        stage("shifted_sums_26_numpy", lambda: W.counts_in(grid, W.CORNERS, (0, 0, 0), (255, 255, 255)))
        results[name + "_host_route_once"] = host
        print(name + "_host_route_once", host, flush=True)
        for nb in W.NEIGHBOURHOODS:
            result, counts = model.neighbours(nb, birth=CAVE[0] & ((2 << nb) - 1), survive=CAVE[1] & ((2 << nb) - 1))
            want = W.neighbours(grid, nb, CAVE[0] & ((2 << nb) - 1), CAVE[1] & ((2 << nb) - 1))
            assert result.tobytes() == want[0].tobytes() and np.array_equal(counts, want[1]), (name, nb)
        for majority in (False, True):
            applied = model.neighbours_apply(W.CORNERS, *CAVE, 1, palette=9, majority=majority)
            after, want, _, _ = W.apply(grid, W.CORNERS, *CAVE, 1, palette=9, majority=majority)
            assert applied.tobytes() == want.tobytes(), (name, majority)
            assert np.array_equal(blocks_to_grid(*model.read()), after), (name, majority)
            restore()
        assert np.array_equal(blocks_to_grid(*model.read()), grid), name                 # the restore between two timed applies works
        extra = {"born": int(want["born"]), "died": int(want["died"])}
        for nb in W.NEIGHBOURHOODS:
            timed(f"{name}_a_read_only_{nb}", lambda: model.neighbours(nb, birth=CAVE[0] & ((2 << nb) - 1), survive=CAVE[1] & ((2 << nb) - 1), tables=False))
            timed(f"{name}_a_read_only_{nb}_table", lambda: model.neighbours(nb, birth=CAVE[0] & ((2 << nb) - 1), survive=CAVE[1] & ((2 << nb) - 1)))
        timed(name + "_surface_counts_only", lambda: model.surface(capacity=0))
        timed(name + "_b_cave_1_generation", lambda: model.neighbours_apply(W.CORNERS, *CAVE, 1, palette=9), extra, between=restore)
        restore()
        eight = model.neighbours_apply(W.CORNERS, *CAVE, 8, palette=9)
        timed(name + "_b_cave_8_generations", lambda: model.neighbours_apply(W.CORNERS, *CAVE, 8, palette=9),
              {"generations": int(eight["generations"]), "born": int(eight["born"]), "died": int(eight["died"])}, between=restore)
        timed(name + "_c_cave_1_generation_majority", lambda: model.neighbours_apply(W.CORNERS, *CAVE, 1, palette=9, majority=True), extra, between=restore)
        restore()
        timed(name + "_single_voxel_set_voxels", lambda: model.set_voxels([(10, 200, 10)], [1] if name != "empty" else [-1]))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
