"""Model joints (dust_hip_model_joints) on three editable 256^3 models: the solid terrain block of tools/mesh_timing.py (y < 128, three
layers of material, 8.4 M voxels), a half-density random fill of the whole tree (8.4 M voxels, eight materials) and the empty tree.
On the same run:
  (a) CELLS on the terrain block after a 16-, a 256- and a 4096-seed fracture;
  (b) CELLS on the terrain block after a 64-seed impact under max_distance2 = 576 (24 voxels): the cells and the unbroken rest;
  (c) MATERIALS on the terrain block, on the half-density fill and on the empty tree;
  (d) the yardsticks: Model.fracture with records, Model.bodies(CELLS) and a count-only Model.surface.
Before anything is timed the device's records are checked byte for byte against the witness of tests/joints_witness.py on the grid read
back from the model, under CELLS with the cell of every solid voxel read back through Model.fracture_at, and their faces against the
cut_faces of the fracture's own records.
All calls are synchronous, so the times are host wall clock around the whole call (Model.joints with capacity=None: a count call and a
call with room for every record): after --warmup calls, the median of --reps calls with the 10th and 90th percentiles beside it. One
process; run it under a time limit (timeout 900 python tools/joints_timing.py).

    python tools/joints_timing.py [--reps 20] [--warmup 3]
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
import joints_witness  # noqa: E402
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
        half.set_voxels(xyz, np.full(len(xyz), 1 + x0 // 32, np.int32))          # (tools/body_timing.py's fill: a material per slab of 32)
    empty = api.Model(ctx, *one, pal)
    empty.set_voxels([(0, 0, 0)], [-1])

    def grid_of(model):
        return blocks_to_grid(*model.read())

    def check_cells(model, grid, result, cells):
        """the device's records against the witness on the labels read back, and against the fracture's own cut_faces"""
        labels = np.full(grid.shape, L.NO_CELL, np.uint16)
        xyz = np.argwhere(grid != 0).astype(np.uint32)
        for k in range(0, len(xyz), 1 << 21):
            part = xyz[k:k + (1 << 21)]
            labels[part[:, 0], part[:, 1], part[:, 2]] = model.fracture_at(part)
        got = model.joints(L.JOINTS_CELLS)
        assert got.tobytes() == joints_witness.joints(grid, joints_witness.CELLS, labels).tobytes()
        inner = got[got["b"] != L.JOINT_REST]
        assert int(inner["faces"].sum()) == int(result["cut_faces"])
        per_cell = np.bincount(inner["a"], inner["faces"], len(cells)) + np.bincount(inner["b"], inner["faces"], len(cells))
        assert per_cell.astype(np.int64).tolist() == cells["cut_faces"].astype(np.int64).tolist()
        return got

    # ---- the terrain block: CELLS
    grid = grid_of(terrain)
    cases = [(f"{n}_seeds", rng.integers((0, 0, 0), (256, 128, 256), (n, 3)), None) for n in (16, 256, 4096)]
    impact = np.array((128, 127, 128)) + rng.integers(-20, 21, (64, 3)) * np.array((1, 0, 1)) - np.array((0, 1, 0)) * rng.integers(0, 20, (64, 1))
    cases.append(("impact_64_seeds_limit_576", impact, 576))
    for name, seeds, limit in cases:
        result, cells = terrain.fracture(seeds, max_distance2=limit)
        got = check_cells(terrain, grid, result, cells)
        extra = {"pairs": len(got), "faces": int(got["faces"].sum(dtype=np.uint64)), "to_rest": int(np.count_nonzero(got["b"] == L.JOINT_REST)), "record_bytes": 80 * len(got)}
        timed(f"terrain_cells_{name}", lambda: terrain.joints(L.JOINTS_CELLS), extra)
        timed(f"terrain_cells_{name}_count_only", lambda: terrain.joints(L.JOINTS_CELLS, capacity=0))
        timed(f"terrain_yardstick_fracture_records_{name}", lambda: terrain.fracture(seeds, max_distance2=limit))
        timed(f"terrain_yardstick_fracture_labels_only_{name}", lambda: terrain.fracture(seeds, max_distance2=limit, records=False))
        terrain.fracture(seeds, max_distance2=limit)
        timed(f"terrain_yardstick_bodies_cells_{name}", lambda: terrain.bodies(L.BODIES_CELLS))
    timed("terrain_yardstick_surface_counts_only", lambda: terrain.surface(capacity=0))

    # ---- MATERIALS
    for name, model in (("terrain", terrain), ("half_density", half), ("empty", empty)):
        grid = grid_of(model)
        got = model.joints(L.JOINTS_MATERIALS)
        assert got.tobytes() == joints_witness.joints(grid, joints_witness.MATERIALS).tobytes(), name
        extra = {"voxels": int(np.count_nonzero(grid)), "pairs": len(got), "faces": int(got["faces"].sum(dtype=np.uint64))}
        timed(f"{name}_materials", lambda: model.joints(L.JOINTS_MATERIALS), extra)
        timed(f"{name}_yardstick_surface_counts_only", lambda: model.surface(capacity=0))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
