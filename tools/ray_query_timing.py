"""Scene ray queries (dust_hip_scene_trace_rays / _async) on the castle stand-in (synth.castle_scene): the 1920x1080 camera rays at pixel
centres through the device path, 2 073 600 incoherent rays (origins uniform in the world box, directions uniform on the sphere), each
closest-hit and any-hit, and the host round trip of one synchronous single-ray query. Times are host wall clock around enqueue + sync
of the context's stream (the query's launch and nothing else is on it), median of the repetitions.

    python tools/ray_query_timing.py [--reps 20] [--single 1000]
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


def camera_dirs(cam, w, h):
    """camera.glsl:4-16 in float32, every pixel centre"""
    f = np.float32
    px, py = np.meshgrid(np.arange(w, dtype=f), np.arange(h, dtype=f))
    cx = f(2.0) * ((px + f(0.5)) / f(w)) - f(1.0)
    cy = -(f(2.0) * ((py + f(0.5)) / f(h)) - f(1.0))
    cx = cx * (f(w) / f(h)) * f(cam.tan_half_fov)
    cy = cy * f(cam.tan_half_fov)
    c0, c1, c2 = (np.asarray(v[:], f) for v in (cam.view_col0, cam.view_col1, cam.view_col2))
    d = (c0 * cx[..., None] + c1 * cy[..., None]) + c2 * f(-1.0)
    return d.reshape(-1, 3)


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--single", type=int, default=1000)
    args = ap.parse_args()
    import torch
    ctx = api.Context(device=0, timing=False)
    data, _ = synth.castle_scene()
    desc = scenes.SceneDesc.from_vox(data)
    scene = scenes.hip_scene(ctx, desc)
    eye = (122.0, 300.61, 54.45)                       # bench.py's headline view (examples/castle.rs:120-129)
    cam = api.make_camera(eye, api.look_at_rotation(eye, (0.0, 0.0, 0.0)), api.PinholeProjection())
    w, h = 1920, 1080
    n = w * h
    cam_rays = api.ray_records(np.tile(np.asarray(cam.position[:], np.float32), (n, 1)), camera_dirs(cam, w, h), cam.near_, cam.far_)
    rng = np.random.default_rng(5)
    bounds = np.array([[np.inf] * 3, [-np.inf] * 3])
    for mid, t in desc.instances:   # the world box: every instance's brick bounds, transformed
        b = desc.models[mid][0]
        m = np.asarray(t, np.float64).reshape(3, 4)
        pts = np.array([[x, y, z] for x in (b["x"].min(), b["x"].max() + 4.0) for y in (b["y"].min(), b["y"].max() + 4.0)
                        for z in (b["z"].min(), b["z"].max() + 4.0)], np.float64) @ m[:, :3].T + m[:, 3]
        bounds = np.array([np.minimum(bounds[0], pts.min(0)), np.maximum(bounds[1], pts.max(0))])
    org = (bounds[0] + rng.random((n, 3)) * (bounds[1] - bounds[0])).astype(np.float32)
    v = rng.normal(size=(n, 3))
    rnd_rays = api.ray_records(org, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))
    hits = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    results = {"scene": {"instances": len(desc.instances), "models": len(desc.models), "bricks": desc.n_bricks()}}
    for name, rays in (("camera_1080p", cam_rays), ("random_2073600", rnd_rays)):
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda")
        torch.cuda.synchronize()
        for any_hit in (False, True):
            ms = timed(ctx, lambda: scene.trace_rays(dev, hits=hits, any_hit=any_hit), args.reps)
            got = hits.cpu().numpy().reshape(-1).view(api.HIT_DTYPE)
            key = f"{name}_{'any' if any_hit else 'closest'}"
            results[key] = {"ms": round(ms, 4), "grays_per_s": round(n / (ms * 1e-3) / 1e9, 3),
                            "hit_fraction": round(float((got["instance"] != L.NO_HIT).mean()), 4)}
            print(key, results[key], flush=True)
    lib = L.load()
    one = cam_rays[n // 2 + w // 2: n // 2 + w // 2 + 1].copy()
    out = np.zeros(1, api.HIT_DTYPE)
    rp, hp = one.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    L.check(lib.dust_hip_scene_trace_rays(scene._h, rp, hp, 1, 0))
    ts = []
    for _ in range(args.single):
        t0 = time.perf_counter()
        lib.dust_hip_scene_trace_rays(scene._h, rp, hp, 1, 0)
        ts.append(time.perf_counter() - t0)
    results["single_ray_sync_us"] = {"median": round(float(np.median(ts)) * 1e6, 2), "p10": round(float(np.percentile(ts, 10)) * 1e6, 2),
                                     "p90": round(float(np.percentile(ts, 90)) * 1e6, 2)}
    print("single_ray_sync_us", results["single_ray_sync_us"], flush=True)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
