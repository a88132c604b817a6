"""Model fracture (dust_hip_model_fracture, _fracture_detach, _fracture_apply) on the solid terrain block of tools/shape_edit_timing.py
(y < 128, three layers of material, 8.4 M voxels) and on a half-density random fill of the whole tree. On the same run, per model:
  (a) fracture with 16, 256 and 4096 seeds scattered through the block, with the records and without;
  (b) 64 seeds within a ball of radius 24 under max_distance2 = 24^2: the impact;
  (c) the 4096-seed case with the cull switched off (DUST_HIP_NO_FRACTURE_CULL: every seed a candidate of every cell);
  (d) the recipe: 16 KEEP_SOURCE detaches and one deleting detach of all 16 cells;
  (e) fracture_apply of the seams (256 seeds) to None;
beside a single-voxel set_voxels (one rebuild), find_islands and Model.distance at R = 255 on the same model, and once the host route:
Model.read() into a grid, the partition on the host (numpy, brute force, 16 seeds), set_voxels of the seams. The device's labels and
records are checked against the witness (tests/fracture_witness.py) on a cropped region before anything is timed. Every timed call that
changes voxels starts from the same voxels: a pristine twin is stamped back over the whole tree (untimed) and the labels are made again.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 900 python tools/fracture_timing.py).

    python tools/fracture_timing.py [--reps 20] [--warmup 3]
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
import fracture_witness as W  # noqa: E402
from island_timing import blocks_to_grid  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402

CROP = ((100, 104, 90), (131, 135, 121))   # 32^3 across root cells on every axis and across the terrain's layers


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

    def terrain():
        m = api.Model(ctx, *one, pal)
        boxes = ([[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]])
        m.edit_shapes(api.edit_shapes(L.SHAPE_BOX, *boxes, op=L.EDIT_FILL, palette=[1, 2, 3]))
        return m

    def noise():
        fill = (np.random.default_rng(7).random((256,) * 3) < 0.5).astype(np.uint8) * 5
        return api.Model(ctx, *api.flatten_model(W.to_xyzi(fill), (256, 256, 256), pal), pal)

    nothing = api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0])
    for tag, build, top in (("terrain", terrain, 128), ("random_half", noise, 256)):
        rng = np.random.default_rng(11)
        model, pristine = build(), build()
        model.set_voxels([(0, 0, 0)], [1])           # (both editable before anything is timed)
        pristine.set_voxels([(0, 0, 0)], [1])
        grid = blocks_to_grid(*model.read())
        voxels = int(np.count_nonzero(grid))
        scattered = {n: np.stack([rng.integers(0, 256, n), rng.integers(0, top, n), rng.integers(0, 256, n)], axis=1) for n in (16, 256, 4096)}
        centre = np.array([118, min(top, 140) - 12, 106])   # inside the crop, at the terrain's top
        ball = []
        while len(ball) < 64:
            p = rng.integers(-24, 25, 3)
            if int((p * p).sum()) <= 24 * 24:
                ball.append(centre + p)
        ball = np.array(ball)

        def restore():
            model.stamp(pristine, api.stamps((0, 0, 0), op=L.STAMP_REPLACE))

        # the device against the witness, on the crop: the labels of whole-tree calls, the records of calls on the crop itself
        xyz = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(*CROP)], indexing="ij"), axis=-1).reshape(-1, 3)
        for n, seeds in scattered.items():
            near = seeds[np.argsort(((seeds - np.array(CROP[0]) - 16) ** 2).sum(axis=1))[:256]] if n == 4096 else seeds   # (the witness is brute force)
            r, cells = model.fracture(near, scale=(1, 2, 1))
            lab, far = W.labels(grid, near, region=CROP, scale=(1, 2, 1))
            assert np.array_equal(model.fracture_at(xyz), W.at(lab, xyz)), (tag, n)
            assert int(cells["voxels"].sum()) == int(r["labelled"]) == voxels and int(cells["cut_faces"].sum()) == 2 * int(r["cut_faces"]), (tag, n)
            r, cells = model.fracture(near, region=CROP, scale=(1, 2, 1))
            assert r.tobytes() == W.result(grid, lab, far, CROP, None, len(near)).tobytes() and cells.tobytes() == W.cells(lab, len(near)).tobytes(), (tag, n)
        r, cells = model.fracture(ball, max_distance2=576)
        lab, far = W.labels(grid, ball, region=CROP, max_distance2=576)
        assert np.array_equal(model.fracture_at(xyz), W.at(lab, xyz)) and 0 < int(r["labelled"]) < voxels, tag
        results[tag] = {"voxels": voxels, "impact_labelled": int(r["labelled"]), "impact_cells": int(r["cells"])}
        print(tag, results[tag], flush=True)

        for n, seeds in scattered.items():
            recs = api.fracture_seeds(seeds)
            r, cells = model.fracture(recs)
            extra = {"cells": int(r["cells"]), "cut_faces": int(r["cut_faces"])}
            timed(f"{tag}_a_fracture_{n}_seeds_records", lambda: model.fracture(recs), extra=extra)
            timed(f"{tag}_a_fracture_{n}_seeds_labels_only", lambda: model.fracture(recs, records=False))
        recs = api.fracture_seeds(ball)
        timed(f"{tag}_b_impact_64_seeds_radius_24", lambda: model.fracture(recs, max_distance2=576))
        timed(f"{tag}_b_impact_64_seeds_radius_24_labels_only", lambda: model.fracture(recs, max_distance2=576, records=False))
        recs = api.fracture_seeds(scattered[4096])
        want = model.fracture(recs)
        os.environ["DUST_HIP_NO_FRACTURE_CULL"] = "1"
        got = model.fracture(recs)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), tag      # the cull changes no byte
        timed(f"{tag}_c_fracture_4096_seeds_no_cull_labels_only", lambda: model.fracture(recs, records=False))
        del os.environ["DUST_HIP_NO_FRACTURE_CULL"]

        recs = api.fracture_seeds(scattered[16])

        def relabel():
            restore()
            model.fracture(recs, records=False)

        def recipe():
            pieces = [model.fracture_detach([i], keep_source=True) for i in range(16)]
            model.fracture_detach(np.arange(16), receive=False)
            return pieces

        relabel()
        assert all(len(p.read()[0]) > 0 for p in recipe()) and len(model.read()[0]) == 0     # 16 pieces, and nothing is left of the source
        timed(f"{tag}_d_recipe_16_copies_and_one_deleting_detach", recipe, between=relabel)
        recs = api.fracture_seeds(scattered[256])
        relabel()
        seams = model.fracture_apply(-1, L.FRACTURE_SEAMS)
        timed(f"{tag}_e_seams_apply_256_seeds", lambda: model.fracture_apply(-1, L.FRACTURE_SEAMS), extra={"seam_voxels": seams}, between=relabel)
        restore()
        timed(f"{tag}_single_voxel_set_voxels", lambda: model.set_voxels([(10, 200, 10)], [1]))
        timed(f"{tag}_find_islands_count_only", lambda: model.find_islands(L.ISLANDS_FACES, capacity=0), between=lambda: model.edit_shapes(nothing))
        timed(f"{tag}_distance_r255", lambda: model.distance(max_radius=255))

        if tag == "terrain":   # the host route, once: read the model back, partition it on the host, push the seams in with set_voxels
            host = {}

            def stage(what, call):
                t0 = time.perf_counter()
                out = call()
                host[what + "_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                return out
            restore()
            back = stage("read_into_a_grid", lambda: blocks_to_grid(*model.read()))
            seeds = scattered[16]

            def partition():
                lab = np.full(back.shape, W.NO_CELL, np.uint16)
                pts = np.argwhere(back != 0).astype(np.int32)
                for c0 in range(0, len(pts), 1 << 18):
                    p = pts[c0:c0 + (1 << 18)]
                    d = p[:, None, :] - seeds[None, :, :].astype(np.int32)
                    lab[p[:, 0], p[:, 1], p[:, 2]] = (d * d).sum(axis=2).argmin(axis=1)
                return lab
            lab = stage("partition_16_seeds_numpy", partition)
            seam = stage("seams_numpy", lambda: np.argwhere(W.seams(lab)).astype(np.uint32))
            stage("set_voxels_of_the_seams", lambda: model.set_voxels(seam, np.full(len(seam), -1, np.int32)))
            host["seam_voxels"] = len(seam)
            twin = build()
            twin.fracture(api.fracture_seeds(seeds), records=False)
            assert twin.fracture_apply(-1, L.FRACTURE_SEAMS) == len(seam) and [a.tobytes() for a in twin.read()] == [a.tobytes() for a in model.read()]
            results["host_route_once"] = host
            print("host_route_once", host, flush=True)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
