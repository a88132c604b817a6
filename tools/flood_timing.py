"""Model floods (dust_hip_model_flood / flood_paths / flood_apply) on one editable 256^3 model, the solid terrain block of
tools/island_timing.py (y < 128, three layers of material, 8.4 M voxels, a pillar on it) with a closed 16^3 room hollowed out of it:
  (a) an air flood from one seed over the whole tree (the 8.4 M empty voxels above the ground);
  (b) the same with max_steps = 32;
  (c) a flood confined to the 16^3 room (the region is the room and its walls);
  (d) flood_paths of 4 096 starts on (a)'s field, at capacity 2 (the next step) and 256;
  (e) flood_apply of (b): the air within 32 steps of the seed becomes a material (undone, untimed, by a carve of the same box region);
beside, on the same run, the parent's own calls: find_islands (faces), a single-voxel set_voxels, and the host route for (a):
Model.read(), the witness's search (tests/flood_witness.py) on the host, and the set_voxels call that writes (b)'s voxels.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. One process; run it under a time limit (timeout 600 python tools/flood_timing.py).

    python tools/flood_timing.py [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flood_witness as W  # noqa: E402
from island_timing import blocks_to_grid  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402

SEED = (180, 140, 180)                       # in the air, 12 voxels above the ground, clear of the pillar
ROOM = ((40, 60, 40), (57, 77, 57))          # the room's walls; the air inside is 41 .. 56


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    model = api.Model(ctx, *api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal), pal)
    build = api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 96, 0], [0, 120, 0], [100, 128, 90]],
                            [[256, 96, 256], [256, 120, 256], [256, 128, 256], [120, 200, 110]], op=L.EDIT_FILL, palette=[1, 2, 3, 4])
    print("terrain:", int(model.edit_shapes(build).sum()), "voxels", flush=True)
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [41, 61, 41], [57, 77, 57]))      # the room
    results = {}

    def timed(name, call, undo=None, extra=None, reps=None, before=None):
        ts = []
        reps = reps or args.reps
        for k in range(args.warmup + reps):
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
        return {k: int(r[k]) for k in ("reached", "farthest", "boundary")}

    nothing = api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0])
    timed("single_voxel_set_voxels", lambda k: model.set_voxels([(10, 100, 10)], [k % 2]))
    model.set_voxels([(10, 100, 10)], [2])      # as it was
    records = np.zeros(16, api.ISLAND_DTYPE)
    timed("find_islands_faces", lambda k: model.find_islands(L.ISLANDS_FACES, records=records), before=lambda: model.edit_shapes(nothing))

    r = model.flood([SEED])
    timed("a_air_flood_whole_tree", lambda k: model.flood([SEED]), extra=record(r))
    rng = np.random.default_rng(5)
    starts = np.stack([rng.integers(0, 256, 4096), rng.integers(128, 256, 4096), rng.integers(0, 256, 4096)], axis=1)
    lengths, _ = model.flood_paths(starts, 2)
    extra = {"starts": len(starts), "reached_starts": int(np.count_nonzero(lengths)), "mean_length": round(float(lengths.mean()), 1)}
    for capacity in (2, 256):
        keys = np.zeros((len(starts), capacity), np.uint32)
        timed(f"d_flood_paths_capacity_{capacity}", lambda k: model.flood_paths(starts, capacity, keys=keys), extra=extra)
    r = model.flood([SEED], max_steps=32)
    timed("b_air_flood_32_steps", lambda k: model.flood([SEED], max_steps=32), extra=record(r))
    inside = tuple(v + 8 for v in ROOM[0])
    r = model.flood([inside], region=ROOM)
    assert int(r["reached"]) == 16 ** 3 and int(r["boundary"]) == 0, r
    timed("c_flood_16_cubed_room", lambda k: model.flood([inside], region=ROOM), extra=record(r))
    # (e): the flood is part of the preparation, the timed call is the apply alone; the undo carves the voxels it filled
    r = model.flood([SEED], max_steps=32)
    lo, hi = r["lo"].astype(np.float64), r["hi"].astype(np.float64) + 1.0
    lo[1] = 128.0                                  # (the flood's lowest layer is the first one above the ground)
    undo = api.edit_shapes(L.SHAPE_BOX, lo, hi)
    changed = []
    timed("e_flood_apply_32_steps", lambda k: changed.append(model.flood_apply(5)), undo=lambda: model.edit_shapes(undo),
          before=lambda: model.flood([SEED], max_steps=32), extra=record(r))
    assert set(changed) == {int(r["reached"])}, (set(changed), r)

    # the host route for (a) and (e)
    t0 = time.perf_counter()
    blocks, mats = model.read()
    read_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    grid = blocks_to_grid(blocks, mats)
    grid_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    field = W.steps(grid, [SEED])
    witness_ms = (time.perf_counter() - t0) * 1e3
    host = {"read_ms": round(read_ms, 2), "blocks_to_grid_numpy_ms": round(grid_ms, 2), "steps_witness_numpy_ms": round(witness_ms, 2)}
    whole = model.flood([SEED])
    assert whole.tobytes() == W.result(field).tobytes(), (whole, W.result(field))
    xyz = np.argwhere(field <= 32).astype(np.uint32)
    fill, clear = np.full(len(xyz), 5, np.int32), np.full(len(xyz), -1, np.int32)
    timed("host_route_set_voxels_32_steps", lambda k: model.set_voxels(xyz, fill), undo=lambda: model.set_voxels(xyz, clear), extra={"entries": len(xyz)})
    results["host_route_once"] = host
    print("host_route_once", host, flush=True)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
