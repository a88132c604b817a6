"""Model islands (dust_hip_model_find_islands / dust_hip_model_detach_islands) on one editable 256^3 model, the solid terrain block of
tools/shape_edit_timing.py (y < 128, three layers of material, 8.4 M voxels) with a pillar standing on it:
  (1) find_islands on the intact block: one island;
  (2) find_islands after a slab has been carved out of the pillar: its top floats, two islands;
  (3) find_islands on a half-density random fill of the whole tree, the many-island case (both connectivities; count only, and with
      every record);
  (4) detach_islands of the floating top into a model of its own (put back, untimed, between two timed calls) -- and, for its parts,
      the same with KEEP_SOURCE (no source rebuild) and as a deletion (no new model);
  (5) the host route a caller has without these calls: Model.read(), labelling on the host (tests/island_witness.py, and
      scipy.ndimage.label where it is installed), and the two set_voxels calls that move the piece;
  (6) one single-voxel box edit: the floor of any edit, the full rebuild plus its readback.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it.

    python tools/island_timing.py [--reps 20] [--warmup 3]
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
import island_witness as W  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402

BOTTOM = ((0, 0, 0), (255, 0, 255))


def blocks_to_grid(blocks, materials):
    """what a caller does with Model.read(): the Block records and the material stream back into a voxel grid"""
    grid = np.zeros((256,) * 3, np.uint8)
    bits = ((blocks["mask"][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    b, bit = np.nonzero(bits)       # ascending bit inside a block: the material stream's order
    x = blocks["x"][b].astype(np.int64) + (bit >> 4)
    y = blocks["y"][b].astype(np.int64) + ((bit >> 2) & 3)
    z = blocks["z"][b].astype(np.int64) + (bit & 3)
    rank = np.arange(len(b)) - np.repeat(np.searchsorted(b, np.arange(len(blocks))), np.bincount(b, minlength=len(blocks)))
    grid[x, y, z] = materials[blocks["material_ptr"][b].astype(np.int64) + rank] + 1
    return grid


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
    cut = api.edit_shapes(L.SHAPE_BOX, [100, 150, 90], [120, 154, 110])
    top = api.edit_shapes(L.SHAPE_BOX, [100, 154, 90], [120, 200, 110], op=L.EDIT_FILL, palette=4)
    print("terrain:", int(model.edit_shapes(build).sum()), "voxels", flush=True)
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

    records = np.zeros(16, api.ISLAND_DTYPE)
    nothing = api.edit_shapes(L.SHAPE_BOX, [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0])
    # a labelling that stands is kept by the next find_islands; an edit with n > 0, here of a shape that covers nothing, invalidates it,
    # so the timed call labels from scratch ("again": the labelling stands and the islands are only counted and described again)
    stale = lambda: model.edit_shapes(nothing)  # noqa: E731
    # (repaints a voxel that is solid already, as tools/shape_edit_timing.py does: the occupancy, and so the islands, stay as they are)
    timed("6_single_voxel_box", lambda k: model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [10.2, 100.2, 10.2], [10.8, 100.8, 10.8],
                                                                             op=L.EDIT_FILL, palette=k % 2)))
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [10.2, 100.2, 10.2], [10.8, 100.8, 10.8], op=L.EDIT_FILL, palette=2))  # as it was
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    assert n == 1, n
    timed("1_find_intact_faces", lambda k: model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM, records=records), extra={"islands": n}, before=stale)
    timed("1_find_intact_corners", lambda k: model.find_islands(L.ISLANDS_CORNERS, anchor=BOTTOM, records=records), extra={"islands": n}, before=stale)
    timed("1_find_intact_corners_again", lambda k: model.find_islands(L.ISLANDS_CORNERS, anchor=BOTTOM, records=records), extra={"islands": n})
    model.edit_shapes(cut)
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    assert n == 2 and rec["flags"].tolist() == [L.ISLAND_ANCHORED, 0], rec
    floating = rec["key"][1:]
    timed("2_find_cut_faces", lambda k: model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM, records=records), extra={"islands": n, "floating_voxels": int(rec["voxels"][1])},
          before=stale)

    def put_back():
        model.edit_shapes(top)
        model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM, records=records)

    model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM, records=records)
    pieces = []
    timed("4_detach_floating_piece", lambda k: pieces.append(model.detach_islands(floating)), lambda: (pieces.clear(), put_back()))
    timed("4_detach_keep_source", lambda k: pieces.append(model.detach_islands(floating, keep_source=True)), pieces.clear)
    timed("4_detach_delete_only", lambda k: model.detach_islands(floating, want_model=False), put_back)

    # (5) the host route
    t0 = time.perf_counter()
    blocks, mats = model.read()
    read_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    grid = blocks_to_grid(blocks, mats)
    grid_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    labels = W.label(grid, W.FACES)
    witness_ms = (time.perf_counter() - t0) * 1e3
    host = {"read_ms": round(read_ms, 2), "blocks_to_grid_numpy_ms": round(grid_ms, 2), "label_witness_numpy_ms": round(witness_ms, 2)}
    try:
        from scipy import ndimage
        t0 = time.perf_counter()
        _, count = ndimage.label(grid != 0)
        host["label_scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        assert count == 2
    except ImportError:
        host["label_scipy_ms"] = None
    t0 = time.perf_counter()
    xyz = np.argwhere(labels == floating[0]).astype(np.uint32)
    values = grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]].astype(np.int32) - 1
    host["enumerate_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    other = api.Model(ctx, *api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal), pal)
    other.set_voxels([(0, 0, 255)], [-1])
    clear = np.full(len(xyz), -1, np.int32)
    timed("5_host_route_read", lambda k: model.read(), extra={"blocks": len(blocks), "materials": len(mats)})
    timed("5_host_route_two_set_voxels", lambda k: (model.set_voxels(xyz, clear), other.set_voxels(xyz, values)),
          lambda: (model.set_voxels(xyz, values), other.set_voxels(xyz, clear)), extra={"entries": len(xyz)})
    results["5_host_route_once"] = host
    print("5_host_route_once", host, flush=True)

    # (3) the many-island case
    rng = np.random.default_rng(7)
    fill = (rng.random((256,) * 3) < 0.5).astype(np.uint8) * 5
    noisy = api.Model(ctx, *api.flatten_model(W.to_xyzi(fill), (256, 256, 256), pal), pal)
    for name, connectivity in (("faces", L.ISLANDS_FACES), ("corners", L.ISLANDS_CORNERS)):
        n, rec = noisy.find_islands(connectivity, anchor=BOTTOM)
        big = np.zeros(n, api.ISLAND_DTYPE)
        extra = {"islands": n, "voxels": int(rec["voxels"].sum()), "largest": int(rec["voxels"].max())}
        stale = lambda: noisy.edit_shapes(nothing)  # noqa: E731
        timed(f"3_find_random_half_{name}_count_only", lambda k: noisy.find_islands(connectivity, capacity=0), extra=extra, before=stale)
        timed(f"3_find_random_half_{name}_all_records", lambda k: noisy.find_islands(connectivity, anchor=BOTTOM, records=big), extra=extra, before=stale)
        timed(f"3_find_random_half_{name}_all_records_again", lambda k: noisy.find_islands(connectivity, anchor=BOTTOM, records=big), extra=extra)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
