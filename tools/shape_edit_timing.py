"""Shape edits (dust_hip_model_edit_shapes) against the per-voxel route (dust_hip_model_set_voxels) on one editable 256^3 model, a solid
terrain block (y < 128, three layers of material):
  (a)  one radius-24 sphere carve through edit_shapes;
  (a') the same voxels through set_voxels, the coordinate list prebuilt (tests/shape_edit_witness.py) -- and, separately, the numpy
       enumeration of that list;
  (b)  4 096 radius-2 sphere carves in one call, against the same voxels through set_voxels;
  (c)  a whole-tree box FILL (every voxel changes colour each time);
  (d)  one single-voxel box: the floor of any edit, the full-lattice rebuild plus its readback.
Both calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. Between two timed calls the carved voxels are put back (untimed). The baseline of every
comparison is the set_voxels figure of the same run.

    python tools/shape_edit_timing.py [--reps 30] [--warmup 5]
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
import shape_edit_witness as W  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402


def covered(shapes):
    """(xyz, count per shape): the voxels the shapes cover, each once, by the witness"""
    seen = np.zeros((256,) * 3, bool)
    for s in shapes:
        reg, m = W.coverage(s)
        seen[reg] |= m
    return np.argwhere(seen).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    ctx = api.Context(device=0, timing=False)
    pal = synth.make_palette(3)
    model = api.Model(ctx, *api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal), pal)
    layers = api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]],
                             op=L.EDIT_FILL, palette=[1, 2, 3])
    restore = api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 96, 0], [0, 120, 0]], [[256, 96, 256], [256, 120, 256], [256, 128, 256]],
                              op=L.EDIT_PLACE, palette=[1, 2, 3])
    print("terrain:", int(model.edit_shapes(layers).sum()), "voxels", flush=True)
    results = {}

    def timed(name, call, undo, extra=None):
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

    put_back = lambda: model.edit_shapes(restore)  # noqa: E731
    rng = np.random.default_rng(9)
    crater = api.edit_shapes(L.SHAPE_SPHERE, [128.5, 110.5, 128.5], radius=24.0)
    t0 = time.perf_counter()
    xyz = covered(crater)
    enum_ms = (time.perf_counter() - t0) * 1e3
    solid = xyz[xyz[:, 1] < 128]
    clear = np.full(len(xyz), -1, np.int32)
    changed = model.edit_shapes(crater)
    assert int(changed[0]) == len(solid), (changed, len(solid))
    put_back()
    timed("d_single_voxel_box", lambda k: model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [10.2, 200.2, 10.2], [10.8, 200.8, 10.8], op=L.EDIT_FILL,
                                                                             palette=k % 2)), None)
    timed("a_sphere24_edit_shapes", lambda k: model.edit_shapes(crater), put_back, {"voxels_changed": int(changed[0]), "voxels_covered": len(xyz)})
    timed("a_sphere24_set_voxels", lambda k: model.set_voxels(xyz, clear), put_back, {"entries": len(xyz), "numpy_enumeration_ms": round(enum_ms, 3)})
    n = 4096
    small = api.edit_shapes(L.SHAPE_SPHERE, np.stack([rng.uniform(4, 252, n), rng.uniform(4, 124, n), rng.uniform(4, 252, n)], axis=1), radius=2.0)
    t0 = time.perf_counter()
    xyz_small = covered(small)
    enum_small_ms = (time.perf_counter() - t0) * 1e3
    clear_small = np.full(len(xyz_small), -1, np.int32)
    total = int(model.edit_shapes(small).sum())
    assert total == len(xyz_small), (total, len(xyz_small))
    put_back()
    timed("b_4096_spheres2_edit_shapes", lambda k: model.edit_shapes(small), put_back, {"voxels_changed": total})
    timed("b_4096_spheres2_set_voxels", lambda k: model.set_voxels(xyz_small, clear_small), put_back,
          {"entries": len(xyz_small), "numpy_enumeration_ms": round(enum_small_ms, 3)})
    timed("restore_three_layer_boxes", lambda k: model.edit_shapes(restore), None)    # (what an undo above costs: three large PLACE boxes)
    timed("c_whole_tree_fill", lambda k: model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [-1e30] * 3, [1e30] * 3, op=L.EDIT_FILL, palette=4 + k % 2)), None)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
