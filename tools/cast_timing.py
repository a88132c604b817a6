"""Model casts (dust_hip_model_cast) on one editable 256^3 model, the solid terrain block of tools/shape_edit_timing.py (y < 128, three
layers of material, 8.4 M voxels) with a pillar standing on it whose top a carved slab has cut loose and dust_hip_model_detach_islands
has lifted into a model of its own (tools/island_timing.py):
  (1) the detached 18 400-voxel top cast straight down, with walls, until it rests on the pillar's stump;
  (2) a 64^3 prefab (a hollow box) fit-tested at 4 096 offsets on and above the terrain in one call (max_steps = 0);
  (3) 65 536 debris pieces of up to eight voxels each, cast down in one call;
  (4) beside each, the host route, the only one there is without the call: Model.read of both models, the two grids rebuilt from the
      blocks' masks, and the whole-array numpy of tests/cast_witness.py -- for (2) and (3) on a sample of the casts, scaled to the call;
  (5) one single-voxel box edit: the floor of any edit, for scale (a cast rebuilds nothing).
All calls are synchronous, so the times are host wall clock around the whole call: after --warmup calls, the median of --reps calls
with the 10th and 90th percentiles beside it. Every case runs in the same process, one after the other.

    python tools/cast_timing.py [--reps 20] [--warmup 3] [--host-sample 64]
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
import cast_witness  # noqa: E402
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, synth  # noqa: E402

BOTTOM = ((0, 0, 0), (255, 0, 255))


def solid_grid(model):
    """the host route's first half: the model read back and its blocks' masks expanded into a 256^3 boolean grid"""
    blocks, _ = model.read()
    grid = np.zeros((256,) * 3, bool)
    bits = np.unpackbits(blocks["mask"].astype("<u8").view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").astype(bool)
    which, bit = np.nonzero(bits)
    grid[blocks["x"][which] + (bit >> 4), blocks["y"][which] + ((bit >> 2) & 3), blocks["z"][which] + (bit & 3)] = True
    return grid


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=64, help="casts of cases (2) and (3) the host route runs (its time is scaled to the call)")
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

    def timed(name, call, extra=None):
        ts = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            call(k)
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                ts.append(dt * 1e3)
        results[name] = {"ms_median": round(float(np.median(ts)), 4), "ms_p10": round(float(np.percentile(ts, 10)), 4),
                         "ms_p90": round(float(np.percentile(ts, 90)), 4), "reps": len(ts)}
        results[name].update(extra or {})
        print(name, results[name], flush=True)

    def host_route(name, dst, src, casts, total):
        """read both models back, rebuild the grids, run the witness on `casts` (a sample when total > len(casts)); once, not --reps times"""
        t0 = time.perf_counter()
        dst_grid, src_grid = solid_grid(dst), solid_grid(src)
        t1 = time.perf_counter()
        hits = cast_witness.cast(dst_grid, src_grid, casts)
        t2 = time.perf_counter()
        read_ms, witness_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3 * total / len(casts)
        results[name] = {"ms": round(read_ms + witness_ms, 1), "ms_read_and_grids": round(read_ms, 1), "ms_witness_scaled": round(witness_ms, 1),
                         "casts_run": len(casts), "casts": total, "reps": 1}
        print(name, results[name], flush=True)
        return hits

    # (5) the floor of an edit (repaints a voxel that is solid already, as tools/shape_edit_timing.py does)
    timed("5_single_voxel_box", lambda k: model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [10.2, 100.2, 10.2], [10.8, 100.8, 10.8],
                                                                             op=L.EDIT_FILL, palette=k % 2)))
    model.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [10.2, 100.2, 10.2], [10.8, 100.8, 10.8], op=L.EDIT_FILL, palette=2))  # as it was

    # (1) the floating top, down to rest
    lo, hi = (100, 154, 90), (119, 199, 109)
    fall = api.casts([lo], (0, -1, 0), L.CAST_MAX_STEPS, flags=L.CAST_WALLS, src_lo=lo, src_hi=hi)
    got = []
    timed("1_cast_detached_top", lambda k: got.append(model.cast(piece, fall)), extra={"voxels": top_voxels})
    assert all(g.tobytes() == got[0].tobytes() for g in got) and got[0]["steps"][0] == 4 and got[0]["contacts"][0] == 400, got[0]
    want = host_route("4_host_detached_top", model, piece, fall, 1)
    assert want.tobytes() == got[0].tobytes(), (want, got[0])

    # (2) a 64^3 prefab, a hollow box with walls four thick, fit-tested at 16 x 16 x 16 offsets from inside the terrain to above the pillar
    prefab = api.Model(ctx, *one, pal)
    prefab.edit_shapes(api.edit_shapes(L.SHAPE_BOX, [[0, 0, 0], [0, 0, 0], [4, 4, 4]], [[256, 256, 256], [64, 64, 64], [60, 60, 60]],
                                       op=[L.EDIT_CARVE, L.EDIT_FILL, L.EDIT_CARVE], palette=[0, 6, 0]))
    gx, gy, gz = np.meshgrid(np.arange(16) * 12, 116 + np.arange(16) * 2, np.arange(16) * 12, indexing="ij")
    fits = api.casts(np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1), (0, 0, 0), 0, src_lo=(0, 0, 0), src_hi=(63, 63, 63))
    got = []
    timed("2_fit_4096_offsets", lambda k: got.append(model.cast(prefab, fits)), extra={"casts": len(fits)})
    assert all(g.tobytes() == got[0].tobytes() for g in got)
    results["2_fit_4096_offsets"]["fit"] = int(np.count_nonzero(got[0]["flags"] == 0))
    rng = np.random.default_rng(1)
    sample = np.sort(rng.choice(len(fits), min(args.host_sample, len(fits)), replace=False))
    want = host_route("4_host_fit_4096_offsets", model, prefab, fits[sample], len(fits))
    assert want.tobytes() == got[0][sample].tobytes()

    # (3) debris: 65 536 sub-boxes of 2^3 voxels of the piece, scattered above the terrain and cast down
    corner = np.stack([rng.integers(100, 119, L.MAX_CASTS), rng.integers(154, 199, L.MAX_CASTS), rng.integers(90, 109, L.MAX_CASTS)], axis=1)
    start = np.stack([rng.integers(0, 254, L.MAX_CASTS), rng.integers(130, 250, L.MAX_CASTS), rng.integers(0, 254, L.MAX_CASTS)], axis=1)
    debris = api.casts(start, (0, -1, 0), L.CAST_MAX_STEPS, flags=L.CAST_WALLS, src_lo=corner, src_hi=corner + 1)
    got = []
    timed("3_cast_65536_debris", lambda k: got.append(model.cast(piece, debris)), extra={"casts": len(debris)})
    assert all(g.tobytes() == got[0].tobytes() for g in got) and (got[0]["flags"] & L.CAST_HIT).all()
    sample = np.sort(rng.choice(len(debris), min(args.host_sample, len(debris)), replace=False))
    want = host_route("4_host_65536_debris", model, piece, debris[sample], len(debris))
    assert want.tobytes() == got[0][sample].tobytes()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
