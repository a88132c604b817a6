"""Model settling (dust_hip_model_settle, dust_hip_model_settle_apply) on the solid terrain block of tools/shape_edit_timing.py (y < 128,
three layers of material, 8.4 M voxels; the two upper layers, palette indices 2 and 3, are loose) with a radius-24 crater carved under
the loose layers at (128, 100, 128). On the same run:
  (a) the count-only call, with the two loose indices named and with every index loose (the masks are all that one reads);
  (b) settle_apply with 0 generations: the crater's roof and rim fall in;
  (c) settle_apply with 1 and with 8 generations: (c8 - b) / 8 is the cost of one further generation (a slide, a fall, the masks);
beside a single-voxel set_voxels on the same model -- the rebuild's floor --, a count-only Model.columns call, one generation of
Model.neighbours_apply, and once the host route: Model.read(), the grid rebuilt with numpy, the witness's fall and set_voxels of the
voxels it changed. Every timed apply starts from the same voxels: between two of them a pristine twin is stamped back over the whole
tree (untimed). The device's result, its applied records and the models they leave are checked against the witness
(tests/settle_witness.py) before anything is timed.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 900 python tools/settle_timing.py).

    python tools/settle_timing.py [--reps 20] [--warmup 3]
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
import settle_witness as W  # noqa: E402
from island_timing import blocks_to_grid  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402

LOOSE = api.loose_mask([2, 3])
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

    def cratered():
        m = api.Model(ctx, *one, pal)
        boxes = ([[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]])
        m.edit_shapes(api.edit_shapes(L.SHAPE_BOX, *boxes, op=L.EDIT_FILL, palette=[1, 2, 3]))
        m.edit_shapes(api.edit_shapes(L.SHAPE_SPHERE, [128.0, 100.0, 128.0], radius=24.0, op=L.EDIT_CARVE))
        return m

    model, pristine = cratered(), cratered()

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
    after, want, _ = stage("witness_fall_numpy", lambda: W.apply(grid, W.NEG_Y, LOOSE, 0))
    changed = np.argwhere(after != grid).astype(np.uint32)
    twin = cratered()
    stage("set_voxels_of_the_changed", lambda: twin.set_voxels(changed, after[tuple(changed.T)].astype(np.int32) - 1))
    assert np.array_equal(blocks_to_grid(*twin.read()), after)
    host["changed_voxels"] = len(changed)
    results["host_route_once"] = host
    print("host_route_once", host, flush=True)
    for loose in (LOOSE, W.ALL_LOOSE):
        assert model.settle(L.FACE_NEG_Y, loose).tobytes() == W.settle(grid, W.NEG_Y, loose).tobytes()
    for generations in (0, 1, 8):
        applied, rows = model.settle_apply(L.FACE_NEG_Y, LOOSE, generations=generations, per_generation=True)
        after, want, want_rows = W.apply(grid, W.NEG_Y, LOOSE, generations)
        assert applied.tobytes() == want.tobytes() and np.array_equal(rows, want_rows), generations
        assert np.array_equal(blocks_to_grid(*model.read()), after), generations
        results[f"applied_{generations}"] = {k: int(want[k]) for k in ("generations", "first_moved", "loose", "slid", "fell", "fall_sum")}
        print(f"applied_{generations}", results[f"applied_{generations}"], flush=True)
        restore()
    assert np.array_equal(blocks_to_grid(*model.read()), grid)                        # the restore between two timed applies works
    timed("a_settle_counts_two_indices", lambda: model.settle(L.FACE_NEG_Y, LOOSE))
    timed("a_settle_counts_all_loose", lambda: model.settle(L.FACE_NEG_Y))
    timed("columns_counts_only", lambda: model.columns(L.FACE_POS_Y, cells=False, tables=False))
    for generations in (0, 1, 8):
        timed(f"{'b' if generations == 0 else 'c'}_settle_apply_{generations}_generations", lambda: model.settle_apply(L.FACE_NEG_Y, LOOSE, generations=generations),
              between=restore)
    g0, g1, g8 = (results[f"{'b' if g == 0 else 'c'}_settle_apply_{g}_generations"]["ms_median"] for g in (0, 1, 8))
    results["one_further_generation_ms"] = {"from_1": round(g1 - g0, 4), "from_8": round((g8 - g0) / 8, 4)}
    print("one_further_generation_ms", results["one_further_generation_ms"], flush=True)
    restore()
    timed("neighbours_apply_1_generation", lambda: model.neighbours_apply(L.NEIGHBOURS_CORNERS, *CAVE, 1, palette=9), between=restore)
    restore()
    timed("single_voxel_set_voxels", lambda: model.set_voxels([(10, 200, 10)], [1]))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
