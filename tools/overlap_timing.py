"""Scene box queries (dust_hip_scene_overlap_boxes / _async) on the castle stand-in (synth.castle_scene): the host round trip of one
synchronous player-sized box (1 x 2 x 1 voxels), 65 536 player-sized boxes on the device path and 256 boxes of 64^3 (blasts), each
counted and with up to 64 records apiece; then 16 384 boxes of 8^3 on a LARGE scene (4 096 scattered, rotated instances) and on a DEEP
one (a 4096^3 model), the other variants of the kernel. Device times are hipEvents (torch.cuda.Event) around the launch on the context's stream (a torch
stream handed to the context and made current) after a warm-up, median of the repetitions; the single query is host wall clock around the whole call, median of --single calls.

    python tools/overlap_timing.py [--reps 20] [--single 1000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dust_amd import _lib as L  # noqa: E402
from dust_amd import api, scenes, synth  # noqa: E402


def world_box(desc):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for mid, t in desc.instances:
        b = desc.models[mid][0]
        m = np.asarray(t, np.float64).reshape(3, 4)
        pts = np.array([[x, y, z] for x in (b["x"].min(), b["x"].max() + 4.0) for y in (b["y"].min(), b["y"].max() + 4.0)
                        for z in (b["z"].min(), b["z"].max() + 4.0)], np.float64) @ m[:, :3].T + m[:, 3]
        lo, hi = np.minimum(lo, pts.min(0)), np.maximum(hi, pts.max(0))
    return lo, hi


def extra_scenes(ctx):
    """[(name, scene, world lo, world hi)]: a LARGE scene (more than 256 instances: the kernels' MODE bit 2) and a DEEP one (a 4096^3
    model: bit 1), as the GPU tests build them"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import parity_util as P
    from test_gpu_many_instances import scattered_scene
    desc = scattered_scene(4096, seed=11)
    out = [("large_4096", scenes.hip_scene(ctx, desc)) + world_box(desc)]
    blocks, mats, pal = P.clustered_deep_model(n_cells=6000)
    deep = api.Scene(ctx)
    xf = np.eye(3, 4, dtype=np.float32)
    xf[:, 3] = -2048.0
    deep.add_instance(api.Model(ctx, blocks, mats, pal, tree_extent_log2=12), xf.reshape(12))
    deep.commit()
    out.append(("deep_4096cubed", deep, np.full(3, -512.0), np.full(3, 512.0)))   # (the occupied 16-cells: 96 .. 160, minus 2048)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--single", type=int, default=1000)
    args = ap.parse_args()
    import torch
    # the context on a torch stream of its own, made current: the events below bracket the query's launch and nothing else
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = api.Context(device=0, timing=False, stream=stream.cuda_stream)
    data, _ = synth.castle_scene()
    desc = scenes.SceneDesc.from_vox(data)
    scene = scenes.hip_scene(ctx, desc)
    lo, hi = world_box(desc)
    rng = np.random.default_rng(5)
    results = {"scene": {"instances": len(desc.instances), "models": len(desc.models), "bricks": desc.n_bricks()}}
    # the ground's top is y = 0 (y up): players stand on it, blasts are centred round it
    player = (1.0, 2.0, 1.0)

    def boxes_at(n, size, y0):
        c = lo + rng.random((n, 3)) * (hi - lo)
        c[:, 1] = y0 + rng.uniform(-4.0, 12.0, n)
        b_lo = np.round(c).astype(np.float32)
        return b_lo, (b_lo + np.asarray(size, np.float32)).astype(np.float32)

    cases = [("player_65536", scene, 65536) + boxes_at(65536, player, 0.0), ("blast64_256", scene, 256) + boxes_at(256, (64.0, 64.0, 64.0), -32.0)]
    for name, other, w_lo, w_hi in extra_scenes(ctx):
        b_lo = np.round(w_lo + rng.random((16384, 3)) * (w_hi - w_lo)).astype(np.float32)
        cases.append((name + "_box8_16384", other, 16384, b_lo, b_lo + np.float32(8.0)))
    for name, scene, n, b_lo, b_hi in cases:
        boxes = api.box_queries(b_lo, b_hi, 64)
        dev = torch.from_numpy(boxes.view(np.int32).reshape(-1, 8).copy()).to("cuda")
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        recs = torch.zeros((n * 64, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for any_hit in (False, True):
            for _ in range(3):
                scene.overlap_boxes(dev, counts=counts, records=recs, any_hit=any_hit)
            ctx.sync()
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ctx.sync()
                e0.record()
                scene.overlap_boxes(dev, counts=counts, records=recs, any_hit=any_hit)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            cnt = counts.cpu().numpy().view(np.uint32)
            key = f"{name}_{'any' if any_hit else 'all'}"
            results[key] = {"ms": round(float(np.median(ts)), 4), "boxes": n, "nonempty": round(float((cnt > 0).mean()), 4),
                            "voxels": int(cnt.astype(np.int64).sum())}
            print(key, results[key], flush=True)
    lib = L.load()
    scene = cases[0][1]
    b_lo, b_hi = boxes_at(64, player, 0.0)
    one = api.box_queries(b_lo[:1], b_hi[:1], 64)
    cnt = np.zeros(1, np.uint32)
    out = np.zeros(64, api.VOXEL_REF_DTYPE)
    bp, cp, rp = one.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for _ in range(20):
        L.check(lib.dust_hip_scene_overlap_boxes(scene._h, bp, 1, cp, rp, 64, 0))
    ts = []
    for _ in range(args.single):
        t0 = time.perf_counter()
        lib.dust_hip_scene_overlap_boxes(scene._h, bp, 1, cp, rp, 64, 0)
        ts.append(time.perf_counter() - t0)
    results["single_player_box_sync_us"] = {"median": round(float(np.median(ts)) * 1e6, 2), "p10": round(float(np.percentile(ts, 10)) * 1e6, 2),
                                            "p90": round(float(np.percentile(ts, 90)) * 1e6, 2), "count": int(cnt[0])}
    print("single_player_box_sync_us", results["single_player_box_sync_us"], flush=True)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
