"""Scene box sweeps (dust_hip_scene_sweep_boxes / _async) on the castle stand-in (synth.castle_scene): 65 536 player-box steps (1 x 2 x 1
voxels at ground level, |delta| <= 1), closest and any hit; 4 096 long sweeps (0.5^3 boxes over 64 to 256 voxels); the host round trip
of one synchronous sweep; 16 384 sweeps of a 2^3 box over 8 to 64 voxels on a LARGE and on a DEEP scene (overlap_timing.py's
extra_scenes: the other variants of the kernel); and the same 65 536 player boxes through dust_hip_scene_overlap_boxes (64 records each) in the same run, for
comparison. Device times are hipEvents (torch.cuda.Event) around the launch on the context's stream (a torch stream handed to the
context and made current) after a warm-up, median of the repetitions; the single sweep is host wall clock around the whole call, median
of --single calls.

    python tools/sweep_timing.py [--reps 20] [--single 1000]
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
from overlap_timing import extra_scenes, world_box  # noqa: E402


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

    def timed(fn):
        for _ in range(3):
            fn()
        ctx.sync()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.sync()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 4)

    def directions(n, lo_len, hi_len):
        d = rng.normal(size=(n, 3))
        return (d * rng.uniform(lo_len, hi_len, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    # the ground's top is y = 0 (y up): players stand on it and step by up to one voxel
    n = 65536
    c = lo + rng.random((n, 3)) * (hi - lo)
    c[:, 1] = rng.uniform(-4.0, 12.0, n)
    p_lo = np.round(c).astype(np.float32)
    p_hi = (p_lo + np.float32([1.0, 2.0, 1.0])).astype(np.float32)
    c = lo + rng.random((4096, 3)) * (hi - lo)
    c[:, 1] = rng.uniform(-4.0, 40.0, 4096)
    l_lo = c.astype(np.float32)
    l_hi = (l_lo + np.float32(0.5)).astype(np.float32)
    cases = [("player_65536", scene, p_lo, p_hi, directions(n, 0.0, 1.0)), ("long_4096", scene, l_lo, l_hi, directions(4096, 64.0, 256.0))]
    for name, other, w_lo, w_hi in extra_scenes(ctx):
        s_lo = np.round(w_lo + rng.random((16384, 3)) * (w_hi - w_lo)).astype(np.float32)
        cases.append((name + "_16384", other, s_lo, s_lo + np.float32(2.0), directions(16384, 8.0, 64.0)))
    for name, sc, s_lo, s_hi, d in cases:
        dev = torch.from_numpy(api.box_sweeps(s_lo, s_hi, d).view(np.int32).reshape(-1, 12).copy()).to("cuda")
        hits = torch.zeros((len(s_lo), 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for any_hit in (False, True):
            ms = timed(lambda: sc.sweep_boxes(dev, hits=hits, any_hit=any_hit))
            h = hits.cpu().numpy().reshape(-1).view(api.SWEEP_HIT_DTYPE)
            key = f"{name}_{'any' if any_hit else 'closest'}"
            results[key] = {"ms": ms, "sweeps": len(s_lo), "hit": round(float((h["instance"] != L.NO_HIT).mean()), 4),
                            "t0": round(float(((h["instance"] != L.NO_HIT) & (h["t"] == 0)).mean()), 4)}
            print(key, results[key], flush=True)
    boxes = api.box_queries(p_lo, p_hi, 64)
    devb = torch.from_numpy(boxes.view(np.int32).reshape(-1, 8).copy()).to("cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    recs = torch.zeros((n * 64, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    results["overlap_player_65536_all"] = {"ms": timed(lambda: scene.overlap_boxes(devb, counts=counts, records=recs)), "boxes": n,
                                           "nonempty": round(float((counts.cpu().numpy() > 0).mean()), 4)}
    print("overlap_player_65536_all", results["overlap_player_65536_all"], flush=True)
    lib = L.load()
    one = api.box_sweeps(p_lo[:1], p_hi[:1], directions(1, 0.5, 1.0))
    out = np.zeros(1, api.SWEEP_HIT_DTYPE)
    sp, hp = one.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for _ in range(20):
        L.check(lib.dust_hip_scene_sweep_boxes(scene._h, sp, hp, 1, 0))
    ts = []
    for _ in range(args.single):
        t0 = time.perf_counter()
        lib.dust_hip_scene_sweep_boxes(scene._h, sp, hp, 1, 0)
        ts.append(time.perf_counter() - t0)
    results["single_sweep_sync_us"] = {"median": round(float(np.median(ts)) * 1e6, 2), "p10": round(float(np.percentile(ts, 10)) * 1e6, 2),
                                       "p90": round(float(np.percentile(ts, 90)) * 1e6, 2)}
    print("single_sweep_sync_us", results["single_sweep_sync_us"], flush=True)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
