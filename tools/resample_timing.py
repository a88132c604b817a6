"""Model resampling (dust_hip_model_resample) on one editable 256^3 model, the solid terrain block of tools/shape_edit_timing.py (y < 128,
three layers of material, 8.4 M voxels), with two source models beside it: a copy of the terrain, and a prefab model that holds a 64^3
block and a 200 x 200 x 4 slab of random materials.
  (1) an identity resample of the whole tree (REPLACE from the copy), beside the identity stamp of the same box;
  (2) the 64^3 piece turned 30 degrees about z and placed above the terrain (PLACE; carved away again, untimed), beside the stamp of the
      same box unturned;
  (3) the 200 x 200 x 4 slab turned 45 degrees about y, its destination box the whole tree (PLACE; carved away again, untimed): the
      root cells the interval test lists beside those the box reaches; its dry run, and the dry run with the image's own bounding box;
  (4) the dry run of (2);
  (5) the host route for (2), once: Model.read(), the voxels expanded into a grid, the witness's numpy, set_voxels of what changed;
  (6) a single-voxel set_voxels: the floor of any edit, the full rebuild plus its readback.
Every case's four counts are compared with the witness's (tests/resample_witness.py) and the written voxels of (2) and (3) are read back
and compared with its grid before anything is timed. All calls are synchronous, so the times are host wall clock around the whole
call: after --warmup calls, the median of --reps calls with the 10th and 90th percentiles beside it, every case in the same process.

    python tools/resample_timing.py [--reps 20] [--warmup 3]
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
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402
import resample_witness as R  # noqa: E402
from island_timing import blocks_to_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    one = api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal)
    build = api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 256, 256], [256, 96, 256], [256, 120, 256], [256, 128, 256]],
                            op=[L.EDIT_CARVE] + [L.EDIT_FILL] * 3, palette=[0, 1, 2, 3])
    model, copy = api.Model(ctx, *one, pal), api.Model(ctx, *one, pal)
    print("terrain:", int(model.edit_shapes(build)[1:].sum()), "voxels", flush=True)
    copy.edit_shapes(build)
    terrain = np.zeros((256,) * 3, np.uint8)
    terrain[:, 0:96], terrain[:, 96:120], terrain[:, 120:128] = 2, 3, 4
    rng = np.random.default_rng(7)
    prefab_grid = np.zeros((256,) * 3, np.uint8)
    prefab_grid[0:64, 0:64, 0:64] = rng.integers(1, 200, (64, 64, 64))
    prefab_grid[20:220, 28:228, 100:104] = rng.integers(1, 200, (200, 200, 4))       # thin in z
    prefab = api.Model(ctx, *one, pal)
    px = np.argwhere(prefab_grid != 0).astype(np.uint32)
    prefab.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [0, 0, 0], [256, 256, 256]))
    prefab.set_voxels(px, prefab_grid[px[:, 0], px[:, 1], px[:, 2]].astype(np.int32) - 1)
    results = {}

    def timed(name, call, undo=None, extra=None):
        ts = []
        for k in range(args.warmup + args.reps):
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

    def verified(recs, src_model, src_grid, undo):
        """the call once against the witness: the four counts, and the image's bounding region read back voxel by voxel"""
        want, counts = R.resample(terrain, src_grid, recs)
        got = model.resample(src_model, recs)
        assert got.tolist() == counts.tolist(), (got, counts)
        where = np.argwhere(want != terrain)
        lo, hi = where.min(axis=0), where.max(axis=0) + 1
        xyz = (np.argwhere(np.ones(hi - lo, bool)) + lo).astype(np.uint32)
        assert (model.get_voxels(xyz).astype(np.int64) + 1 == want[xyz[:, 0], xyz[:, 1], xyz[:, 2]]).all()
        undo()
        assert (model.get_voxels(xyz).astype(np.int64) + 1 == terrain[xyz[:, 0], xyz[:, 1], xyz[:, 2]]).all()
        return want, counts

    # (6) the floor (repaints a voxel that is solid already)
    timed("6_single_voxel_set_voxels", lambda k: model.set_voxels([(10, 100, 10)], [k % 2]))
    model.set_voxels([(10, 100, 10)], [2])   # as it was

    # (1) the whole tree, identity
    identity = R.records([np.eye(3, dtype=np.int64) * R.ONE], [(0, 0, 0)], (0, 0, 0), (255, 255, 255), L.STAMP_REPLACE)
    want, counts = R.resample(terrain, terrain, identity)
    assert model.resample(copy, identity).tolist() == counts.tolist() == [(0, 1 << 24, 1 << 23, 1 << 23)]
    timed("1_resample_identity_whole_tree", lambda k: model.resample(copy, identity))
    whole = api.stamps([(0, 0, 0)], api.ORIENT_IDENTITY, L.STAMP_REPLACE)
    assert model.stamp(copy, whole).tolist() == [0]
    timed("1_stamp_identity_whole_tree", lambda k: model.stamp(copy, whole))

    # (2) the 64^3 piece, 30 degrees about z, standing on the terrain's top
    piece = api.resamples(api.rotation_about("z", 30.0, (32.0, 32.0, 32.0), (128.0, 176.0, 128.0)), L.STAMP_PLACE, (0, 0, 0), (63, 63, 63))
    clear = api.edit_shapes(L.SHAPE_BOX, [0, 128, 0], [256, 256, 256])
    want_piece, piece_counts = verified(piece, prefab, prefab_grid, lambda: model.edit_shapes(clear))
    timed("2_resample_64_cube_30_degrees", lambda k: model.resample(prefab, piece), lambda: model.edit_shapes(clear), extra={"voxels": int(piece_counts["changed"][0])})
    plain = api.stamps([(96, 144, 96)], api.ORIENT_IDENTITY, L.STAMP_PLACE, (0, 0, 0), (63, 63, 63))
    assert model.stamp(prefab, plain).tolist() == [64 ** 3]
    model.edit_shapes(clear)
    timed("2_stamp_64_cube", lambda k: model.stamp(prefab, plain), lambda: model.edit_shapes(clear), extra={"voxels": 64 ** 3})

    # (4) its dry run
    assert model.resample(prefab, piece, dry_run=True).tolist() == piece_counts.tolist()
    timed("4_dry_run_64_cube_30_degrees", lambda k: model.resample(prefab, piece, dry_run=True))

    # (3) the slab, 45 degrees about y, through the terrain and the air above it (PLACE: only the voxels above the terrain change)
    slab = api.resamples(api.rotation_about("y", 45.0, (120.0, 128.0, 102.0), (128.0, 128.0, 128.0)), L.STAMP_PLACE, (20, 28, 100), (219, 227, 103))
    slab["dst_lo"], slab["dst_hi"] = 0, 255
    listed, reached = R.cells_listed(slab[0])
    restore = lambda: model.edit_shapes(clear)  # noqa: E731
    _, slab_counts = verified(slab, prefab, prefab_grid, restore)
    extra = {"voxels": int(slab_counts["changed"][0]), "cells_listed": len(listed), "cells_reached": reached}
    timed("3_resample_slab_45_degrees", lambda k: model.resample(prefab, slab), restore, extra=extra)
    assert model.resample(prefab, slab, dry_run=True).tolist() == slab_counts.tolist()
    timed("3_dry_run_slab_45_degrees", lambda k: model.resample(prefab, slab, dry_run=True))      # (no rebuild: the kernel and the binning show)
    # the same slab in a record whose destination box is the image's own bounding box (what api.resamples sets)
    tight = api.resamples(api.rotation_about("y", 45.0, (120.0, 128.0, 102.0), (128.0, 128.0, 128.0)), L.STAMP_PLACE, (20, 28, 100), (219, 227, 103))
    assert model.resample(prefab, tight, dry_run=True).tolist() == slab_counts.tolist()
    timed("3_dry_run_slab_45_degrees_own_box", lambda k: model.resample(prefab, tight, dry_run=True))
    whole_dry = model.resample(copy, identity, dry_run=True)
    assert whole_dry.tolist() == [(0, 1 << 24, 1 << 23, 1 << 23)]
    timed("1_dry_run_identity_whole_tree", lambda k: model.resample(copy, identity, dry_run=True))

    # (5) the host route for (2), once
    t0 = time.perf_counter()
    grid = blocks_to_grid(*model.read())
    t_read = time.perf_counter() - t0
    assert np.array_equal(grid, terrain)
    t0 = time.perf_counter()
    after, _ = R.resample(grid, prefab_grid, piece)
    differs = np.argwhere(after != grid).astype(np.uint32)
    values = after[differs[:, 0], differs[:, 1], differs[:, 2]].astype(np.int32) - 1
    t_numpy = time.perf_counter() - t0
    t0 = time.perf_counter()
    model.set_voxels(differs, values)
    t_set = time.perf_counter() - t0
    assert np.array_equal(after, want_piece)
    model.edit_shapes(clear)
    results["5_host_route_64_cube_30_degrees"] = {"ms_read": round(t_read * 1e3, 1), "ms_numpy": round(t_numpy * 1e3, 1), "ms_set_voxels": round(t_set * 1e3, 1),
                                                  "ms_total": round((t_read + t_numpy + t_set) * 1e3, 1), "entries": len(differs)}
    print("5_host_route_64_cube_30_degrees", results["5_host_route_64_cube_30_degrees"], flush=True)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
