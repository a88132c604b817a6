"""Model bodies (dust_hip_model_bodies) on three editable 256^3 models: the solid terrain block of tools/mesh_timing.py (y < 128, three
layers of material, 8.4 M voxels), a half-density random fill of the whole tree (8.4 M voxels, eight materials) and the empty tree.
Per model, on the same run:
  (a) ALL without weights (masks only: no grid byte is read) and with weights;
  (b) MATERIALS with weights;
  (c) ISLANDS with weights after a find_islands, every record;
  (d) CELLS with weights after a 16-seed and after a 4096-seed fracture;
  (e) the yardsticks: a count-only Model.surface, a find_islands with all records (the labelling standing) and a whole-tree census.
Before anything is timed the device's records are checked: ALL and MATERIALS, with and without weights, byte for byte against the witness
of tests/body_witness.py on the grid read back from the model; ISLANDS and CELLS, whose witnesses would need a host labelling of
millions of pieces, field for field against find_islands' and fracture's own records under unit weights, and their weighted records
summed against the weighted ALL record over the same voxels.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 900 python tools/body_timing.py).

    python tools/body_timing.py [--reps 20] [--warmup 3]
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
import body_witness  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402


def summed(records):
    """what the records of a partition add up to: voxels, mass, m1, m2 as Python ints"""
    return (int(records["voxels"].sum(dtype=np.uint64)), int(records["mass"].sum(dtype=np.uint64)),
            [int(v) for v in records["m1"].sum(axis=0, dtype=np.uint64)], [int(v) for v in records["m2"].sum(axis=0, dtype=np.uint64)])


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
    rng = np.random.default_rng(7)
    half = api.Model(ctx, *one, pal)
    for x0 in range(0, 256, 32):          # 32 slabs' worth of coordinates per call
        xyz = np.argwhere(rng.random((32, 256, 256)) < 0.5).astype(np.uint32)
        xyz[:, 0] += x0
        half.set_voxels(xyz, np.full(len(xyz), 1 + x0 // 32, np.int32))
    empty = api.Model(ctx, *one, pal)
    empty.set_voxels([(0, 0, 0)], [-1])
    weights = rng.integers(0, 65536, 255)
    weights[:4] = 2700, 700, 0, 65535
    whole_tree = api.edit_shapes(L.SHAPE_BOX, (0, 0, 0), (256, 256, 256))
    seeds16 = rng.integers(0, 256, (16, 3))
    seeds4096 = rng.integers(0, 256, (4096, 3))

    for name, model in (("terrain", terrain), ("half_density", half), ("empty", empty)):
        blocks, mats = model.read()
        voxels = body_witness.voxel_list(blocks_to_grid(blocks, mats))
        for group in (L.BODIES_ALL, L.BODIES_MATERIALS):
            for w in (None, weights):
                assert model.bodies(group, w).tobytes() == body_witness.bodies(voxels, group, w).tobytes(), (name, group)
        everything = summed(model.bodies(L.BODIES_ALL, weights))
        n, islands = model.find_islands(L.ISLANDS_FACES)
        plain = model.bodies(L.BODIES_ISLANDS)
        for field, theirs in (("key", "key"), ("voxels", "voxels"), ("lo", "lo"), ("hi", "hi"), ("m1", "sum")):
            assert plain[field].tobytes() == islands[theirs].tobytes(), (name, field)
        assert summed(model.bodies(L.BODIES_ISLANDS, weights)) == everything, name
        timed(name + "_a_all_unweighted", lambda: model.bodies(L.BODIES_ALL), {"voxels": everything[0]})
        timed(name + "_a_all_weighted", lambda: model.bodies(L.BODIES_ALL, weights))
        timed(name + "_b_materials_weighted", lambda: model.bodies(L.BODIES_MATERIALS, weights))
        timed(name + "_c_islands_weighted", lambda: model.bodies(L.BODIES_ISLANDS, weights), {"islands": n, "record_bytes": 96 * n})
        timed(name + "_e_find_islands_all_records", lambda: model.find_islands(L.ISLANDS_FACES), {"record_bytes": 40 * n})
        for seeds in (seeds16, seeds4096):
            _, cells = model.fracture(seeds)
            plain = model.bodies(L.BODIES_CELLS)
            for field, theirs in (("voxels", "voxels"), ("lo", "lo"), ("hi", "hi"), ("m1", "sum")):
                assert plain[field].tobytes() == cells[theirs].tobytes(), (name, len(seeds), field)
            assert summed(model.bodies(L.BODIES_CELLS, weights)) == everything, (name, len(seeds))   # (no limit: every solid voxel is labelled)
            timed(f"{name}_d_cells_{len(seeds)}_seeds_weighted", lambda: model.bodies(L.BODIES_CELLS, weights))
        timed(name + "_e_surface_counts_only", lambda: model.surface(capacity=0))
        timed(name + "_e_census_whole_tree", lambda: model.census(whole_tree, tables=False))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
