"""Model stamps (dust_hip_model_stamp) on one editable 256^3 model, the solid terrain block of tools/shape_edit_timing.py (y < 128, three
layers of material, 8.4 M voxels) with a pillar standing on it whose top a carved slab has cut loose and dust_hip_model_detach_islands
has lifted into a model of its own (tools/island_timing.py):
  (1) the detached 18 400-voxel top stamped back where it was (PLACE; carved out again, untimed, between two timed calls);
  (2) 4 096 PLACE stamps of one 8 x 16 x 8 prefab in one call, 32 x 32 of them side by side in four layers on the terrain (carved away
      again, untimed);
  (3) beside each, the same voxels through set_voxels with the list prebuilt: the only route without the call;
  (4) one single-voxel box edit: the floor of any edit, the full rebuild plus its readback.
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. Every case runs in the same process, one after the other.

    python tools/stamp_timing.py [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402

BOTTOM = ((0, 0, 0), (255, 0, 255))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    one = api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal)
    model = api.Model(ctx, *one, pal)
    build = api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 0, 0], [0, 96, 0], [0, 120, 0], [100, 128, 90]],
                            [[256, 256, 256], [256, 96, 256], [256, 120, 256], [256, 128, 256], [120, 200, 110]],
                            op=[L.EDIT_CARVE] + [L.EDIT_FILL] * 4, palette=[0, 1, 2, 3, 4])
    print("terrain:", int(model.edit_shapes(build)[1:].sum()), "voxels", flush=True)
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [100, 150, 90], [120, 154, 110]))
    n, rec = model.find_islands(L.ISLANDS_FACES, anchor=BOTTOM)
    assert n == 2 and rec["flags"].tolist() == [L.ISLAND_ANCHORED, 0], rec
    piece = model.detach_islands(rec["key"][1:])
    top_voxels = int(rec["voxels"][1])
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

    # (4) the floor (repaints a voxel that is solid already, as tools/shape_edit_timing.py does)
    timed("4_single_voxel_box", lambda k: model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [10.2, 100.2, 10.2], [10.8, 100.8, 10.8],
                                                                             op=L.EDIT_FILL, palette=k % 2)))
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [10.2, 100.2, 10.2], [10.8, 100.8, 10.8], op=L.EDIT_FILL, palette=2))  # as it was

    # (1) the detached top back where it was
    back = api.stamps([(100, 154, 90)], api.ORIENT_IDENTITY, L.STAMP_PLACE, (100, 154, 90), (119, 199, 109))
    carve_top = api.edit_shapes(L.SHAPE_BOX, [100, 154, 90], [120, 200, 110])
    counts = []
    timed("1_stamp_detached_top", lambda k: counts.append(int(model.stamp(piece, back)[0])), lambda: model.edit_shapes(carve_top),
          extra={"voxels": top_voxels})
    assert set(counts) == {top_voxels}, set(counts)
    xyz = np.argwhere(np.ones((20, 46, 20), bool)).astype(np.uint32) + np.uint32([100, 154, 90])
    values = piece.get_voxels(xyz)
    assert (values == 4).all() and len(values) == top_voxels
    timed("3_set_voxels_detached_top", lambda k: model.set_voxels(xyz, values), lambda: model.edit_shapes(carve_top), extra={"entries": len(xyz)})

    # (2) a field of prefabs: an 8 x 16 x 8 tower of two materials with a hollow core, 32 x 32 x 4 of them on the terrain
    prefab = api.Model(ctx, *one, pal)
    prefab.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 0, 0], [0, 12, 0], [2, 0, 2]], [[256, 256, 256], [8, 16, 8], [8, 16, 8], [6, 14, 6]],
                                       op=[L.EDIT_CARVE, L.EDIT_FILL, L.EDIT_FILL, L.EDIT_CARVE], palette=[0, 6, 7, 0]))
    gx, gy, gz = np.meshgrid(np.arange(32) * 8, 128 + np.arange(4) * 16, np.arange(32) * 8, indexing="ij")
    offsets = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)
    field = api.stamps(offsets, api.ORIENT_IDENTITY, L.STAMP_PLACE, (0, 0, 0), (7, 15, 7))
    clear_field = np.concatenate([api.edit_shapes(L.SHAPE_BOX, [0, 128, 0], [256, 192, 256]),
                                  api.edit_shapes(L.SHAPE_BOX, [100, 128, 90], [120, 150, 110], op=L.EDIT_FILL, palette=4)])
    placed = []
    timed("2_stamp_4096_prefabs", lambda k: placed.append(int(model.stamp(prefab, field).sum(dtype=np.int64))), lambda: model.edit_shapes(clear_field),
          extra={"stamps": len(field)})
    assert len(set(placed)) == 1, set(placed)
    results["2_stamp_4096_prefabs"]["voxels_placed"] = placed[0]
    # the same voxels through set_voxels: the region as the stamps leave it, enumerated once outside the timing
    model.stamp(prefab, field)
    region = np.argwhere(np.ones((256, 64, 256), bool)).astype(np.uint32) + np.uint32([0, 128, 0])
    after = model.get_voxels(region)
    model.edit_shapes(clear_field)
    differs = after != model.get_voxels(region)
    fxyz, fvalues = region[differs], after[differs]
    assert len(fxyz) == placed[0], (len(fxyz), placed[0])
    timed("3_set_voxels_4096_prefabs", lambda k: model.set_voxels(fxyz, fvalues), lambda: model.edit_shapes(clear_field), extra={"entries": len(fxyz)})
    print(json.dumps(results))


if __name__ == "__main__":
    main()
