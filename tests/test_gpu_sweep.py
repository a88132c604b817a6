"""Scene box sweeps on the device (dust_hip_scene_sweep_boxes / _async, sweep.hip): the first solid voxel a moving world-space box touches.
The numpy witness of tests/sweep_witness.py does the checking: whole records byte for byte on axis-aligned scenes (t bits and normal
included), the tolerance bracket of the header on rotated ones."""
import ctypes as C

import numpy as np
import pytest

import parity_util as P
from dust_amd import _lib as L
from dust_amd import api, scenes
from sweep_witness import SweepWitness, first_time, miss
from test_gpu_many_instances import scattered_scene
from test_gpu_overlap import castle_desc, world_bounds

pytestmark = pytest.mark.gpu

F = np.float32
NO_HIT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def castle():
    desc = castle_desc()
    ctx = api.Context(device=0)
    scene = scenes.hip_scene(ctx, desc)
    return ctx, scene, desc, SweepWitness(desc)


def check_exact(scene, wit, lo, hi, d, ignore_start=False):
    lo, hi, d = np.asarray(lo, F), np.asarray(hi, F), np.asarray(d, F)
    got = scene.sweep_boxes(lo, hi, d, ignore_start=ignore_start)
    for i in range(len(lo)):
        want = wit.exact(lo[i], hi[i], d[i], ignore_start=ignore_start)
        assert got[i].tobytes() == want.tobytes(), (i, lo[i], hi[i], d[i], got[i], want)
    return got


def castle_sweeps(rng, desc, n):
    """the castle families, about n sweeps: player steps, drops onto the ground, walks into walls, long sweeps across many instances,
    axis-only deltas, zero deltas, flat and point boxes on integer and half-integer planes, starts inside, negative-zero components"""
    wlo, whi = world_bounds(desc)
    k = n // 10
    out = []

    def at(m, y0=None, yspan=(-2.0, 10.0)):
        c = wlo + rng.random((m, 3)) * (whi - wlo)
        if y0 is not None:
            c[:, 1] = y0 + rng.uniform(*yspan, m)
        return c

    player = np.array([1.0, 2.0, 1.0])
    c = np.round(at(2 * k, 0.0))                                          # player steps on voxel faces, |delta| <= 1
    d = rng.normal(size=(2 * k, 3))
    d *= rng.uniform(0.0, 1.0, (2 * k, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    out.append((c, c + player, d))
    c = at(k, 0.0, (0.5, 10.0))                                            # drops onto the ground (its top is y = 0)
    out.append((c, c + player, np.tile([0.0, -20.0, 0.0], (k, 1))))
    c = np.round(at(k, 0.0, (0.0, 4.0)))                                  # walks into walls
    ang = rng.uniform(0.0, 2.0 * np.pi, k)
    out.append((c, c + player, np.stack([np.cos(ang), np.zeros(k), np.sin(ang)], 1) * rng.uniform(1.0, 8.0, (k, 1))))
    c = at(k, 0.0, (-4.0, 40.0))                                           # long sweeps, 64 to 300 voxels, across many instances
    d = rng.normal(size=(k, 3))
    d *= rng.uniform(64.0, 300.0, (k, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    out.append((c, c + 0.5, d))
    c = np.round(at(k, 0.0) * 2.0) / 2.0                                   # axis-only deltas
    d = np.zeros((k, 3))
    d[np.arange(k), rng.integers(0, 3, k)] = rng.uniform(-12.0, 12.0, k)
    out.append((c, c + player, d))
    c = np.round(at(k // 2, 0.0, (-3.0, 3.0)) * 2.0) / 2.0              # zero deltas
    out.append((c, c + rng.integers(0, 3, (k // 2, 3)), np.zeros((k // 2, 3))))
    c = np.round(at(k, 0.0) * 2.0) / 2.0                                   # flat and point boxes on integer and half-integer planes
    size = rng.integers(0, 4, (k, 3)).astype(np.float64)
    size[: k // 2] = 0.0
    size[k // 2:, 1] = 0.0
    d = rng.uniform(-6.0, 6.0, (k, 3))
    d[rng.random((k, 3)) < 0.3] = 0.0
    out.append((c, c + size, d))
    c = at(k, 0.0, (-6.0, 0.0))                                            # starts inside (most of these are in the ground)
    d = rng.uniform(-3.0, 3.0, (k, 3))
    out.append((c, c + rng.uniform(0.2, 2.0, (k, 3)), d))
    c = np.round(at(k - k // 2, 0.0, (0.0, 6.0)))                          # negative-zero components
    d = rng.uniform(-5.0, 5.0, (k - k // 2, 3))
    d[rng.random(d.shape) < 0.5] = -0.0
    out.append((c, c + player, d))
    lo = np.concatenate([o[0] for o in out]).astype(F)
    hi = np.concatenate([o[1] for o in out]).astype(F)
    dd = np.concatenate([o[2] for o in out]).astype(F)
    return lo, hi, dd


# ------------------------------------------------------------------ 1. the castle stand-in: exact, whole records
def test_castle_sweeps_match_the_witness_exactly(castle):
    ctx, scene, desc, wit = castle
    lo, hi, d = castle_sweeps(np.random.default_rng(1), desc, 4000)
    assert len(lo) == 3600 and np.any(np.signbit(d) & (d == 0))
    got = check_exact(scene, wit, lo, hi, d)
    hit = got["instance"] != NO_HIT
    assert hit.mean() > 0.3 and (got["t"][hit] > 0).sum() > 300 and (got["t"][hit] == 0).sum() > 100
    # the ground's top is y = 0: many drops land on it, with normal +y
    drops = slice(800, 1200)
    up = got["normal"][drops][:, 1] == 1.0
    assert up.mean() > 0.5
    landed = lo[drops][:, 1] + got["t"][drops] * d[drops][:, 1]
    assert np.mean(np.abs(landed[up]) < 1e-3) > 0.3


def test_ignore_start_exact(castle):
    ctx, scene, desc, wit = castle
    lo, hi, d = castle_sweeps(np.random.default_rng(2), desc, 1000)
    plain = scene.sweep_boxes(lo, hi, d)
    got = check_exact(scene, wit, lo, hi, d, ignore_start=True)
    started_inside = (plain["instance"] != NO_HIT) & (plain["t"] == 0) & np.all(plain["normal"] == 0, axis=1)
    assert started_inside.sum() > 50
    assert np.all((got["t"] > 0) | np.any(got["normal"] != 0, axis=1) | (got["instance"] == NO_HIT))


def test_any_hit(castle):
    ctx, scene, desc, wit = castle
    lo, hi, d = castle_sweeps(np.random.default_rng(3), desc, 1000)
    closest = scene.sweep_boxes(lo, hi, d)
    anyh = scene.sweep_boxes(lo, hi, d, any_hit=True)
    m = miss().tobytes()
    for i in range(len(lo)):
        if closest[i]["instance"] == NO_HIT:
            assert anyh[i].tobytes() == m, i
        else:
            hits = {h.tobytes() for h in wit.exact(lo[i], hi[i], d[i], any_hit=True)}
            assert anyh[i].tobytes() in hits, (i, anyh[i])


def test_zero_delta_agrees_with_overlap_boxes(castle):
    ctx, scene, desc, wit = castle
    rng = np.random.default_rng(4)
    wlo, whi = world_bounds(desc)
    c = wlo + rng.random((600, 3)) * (whi - wlo)
    c[:, 1] = rng.uniform(-6.0, 6.0, 600)
    c = np.round(c * 2.0) / 2.0
    lo, hi = c.astype(F), (c + rng.integers(0, 3, (600, 3))).astype(F)
    counts, _ = scene.overlap_boxes(lo, hi, capacity=0)
    got = scene.sweep_boxes(lo, hi, np.zeros((600, 3), F))
    assert np.array_equal(got["instance"] != NO_HIT, counts > 0)
    assert np.all(got["t"][counts > 0] == 0) and np.all(got["t"][counts == 0] == 1)
    assert 50 < (counts > 0).sum() < 550


# ------------------------------------------------------------------ 2. aligned scenes: 90-degree rotations, mirrors and scales
def test_aligned_rotations_mirrors_and_scales():
    base = P.small_scene(seed=5, n_models=3, n_instances=1)
    rng = np.random.default_rng(5)
    instances = []
    for i, s in enumerate([1.0, 0.5, 3.0, -2.0, 1.0, -1.0, 0.5, 3.0]):
        perm = np.eye(3)[rng.permutation(3)] * np.where(rng.random(3) < 0.3, -1.0, 1.0)[:, None]
        m = np.zeros((3, 4), F)
        m[:, :3] = perm * s
        m[:, 3] = rng.integers(-80, 80, 3) + rng.choice([0.0, 0.25, 0.5], 3)
        instances.append((i % len(base.models), m.reshape(12)))
    desc = scenes.SceneDesc(base.models, base.palette, instances)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    wit = SweepWitness(desc)
    wlo, whi = world_bounds(desc)
    n = 900
    c = wlo + rng.random((n, 3)) * (whi - wlo)
    c[: n // 3] = np.round(c[: n // 3] * 4.0) / 4.0
    size = rng.uniform(0.0, 3.0, (n, 3))
    size[n // 3: n // 2] = 0.0
    d = rng.normal(size=(n, 3)) * rng.choice([1.0, 10.0, 60.0], (n, 1))
    d[rng.random((n, 3)) < 0.2] = 0.0
    got = check_exact(scene, wit, c, c + size, d)
    assert (got["instance"] != NO_HIT).sum() > n // 10
    assert len(set(got["instance"][got["instance"] != NO_HIT].tolist())) >= 5


# ------------------------------------------------------------------ 3. a 4096^3 model: exact across 16-cell and 256-cell borders
def test_deep_model_exact():
    blocks, mats, pal = P.clustered_deep_model(n_cells=6000)
    ctx = api.Context(device=0)
    model = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    scene = api.Scene(ctx)
    xf = np.eye(3, 4, dtype=F)
    xf[:, 3] = (-2048.0, -2048.0, -2048.0)
    scene.add_instance(model, xf.reshape(12))
    scene.commit()
    desc = scenes.SceneDesc([(blocks, mats)], pal, [(0, xf.reshape(12))])
    wit = SweepWitness(desc)
    rng = np.random.default_rng(6)
    n = 200
    border = rng.choice([1792.0, 2048.0, 2304.0], (n, 3))
    border[: n // 2] = (96 + rng.integers(0, 64, (n // 2, 3))) * 16.0
    c = border - 2048.0 - rng.uniform(1.0, 40.0, (n, 3))
    d = rng.normal(size=(n, 3))
    d *= rng.uniform(8.0, 600.0, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    got = check_exact(scene, wit, c, c + rng.uniform(0.0, 4.0, (n, 3)), d)
    assert (got["instance"] != NO_HIT).sum() > n // 5


# ------------------------------------------------------------------ 4. rotated instances: the tolerance bracket
def check_bracket(desc, n, seed, long=True):
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    wit = SweepWitness(desc)
    wlo, whi = world_bounds(desc)
    rng = np.random.default_rng(seed)
    c = wlo + rng.random((n, 3)) * (whi - wlo)
    size = rng.uniform(0.0, 3.0, (n, 3))
    d = rng.normal(size=(n, 3)) * (rng.choice([1.0, 8.0, 40.0], (n, 1)) if long else 1.0)
    d[: n // 8] = 0.0
    lo, hi, d = c.astype(F), (c + size).astype(F), d.astype(F)
    got = scene.sweep_boxes(lo, hi, d)
    assert (got["instance"] != NO_HIT).sum() > n // 6
    for i in range(n):
        inner = wit.contact_times(lo[i], hi[i], d[i], -1.0)
        g = got[i]
        if g["instance"] == NO_HIT:
            assert not inner, (i, inner[:3])
            assert g.tobytes() == miss().tobytes()
            continue
        t = float(g["t"])
        assert t <= first_time(inner) + 1e-6, (i, t, first_time(inner))
        key = (int(g["instance"]), int(g["block"]), int(g["voxel"]))
        outer = [o for o in wit.contact_times(lo[i], hi[i], d[i], 1.0) if o[:3] == key]
        assert outer and max(outer[0][3], 0.0) <= t + 1e-6, (i, t, outer)
        nrm = g["normal"].astype(np.float64)
        if np.any(nrm != 0):
            assert abs(np.linalg.norm(nrm) - 1.0) < 1e-5 and float(nrm @ d[i]) <= 1e-6 * (1.0 + np.abs(d[i]).max()), (i, nrm)
        blocks, mats = desc.models[desc.instances[key[0]][0]]
        b = blocks[key[1]]
        v = key[2]
        assert (int(b["mask"]) >> v) & 1
        assert [int(b["x"]) + (v >> 4), int(b["y"]) + ((v >> 2) & 3), int(b["z"]) + (v & 3)] == [int(x) for x in g["xyz"]]


def test_rotated_instances_within_tolerance():
    check_bracket(scattered_scene(4096, seed=11), 160, seed=7)


def test_scene_without_a_usable_grid_within_tolerance():
    check_bracket(scattered_scene(4200, seed=23, n_models=3, span=(0.0, 0.0, 0.0)), 24, seed=8, long=False)


# ------------------------------------------------------------------ 5. a controller loop: gravity and walking, per-axis sweeps
def test_controller_loop_never_ends_inside(castle):
    ctx, scene, desc, wit = castle
    rng = np.random.default_rng(9)
    wlo, whi = world_bounds(desc)
    c = wlo + rng.random((400, 3)) * (whi - wlo)
    c[:, 1] = rng.uniform(0.5, 12.0, 400)
    lo, hi = c.astype(F), (c + [1.0, 2.0, 1.0]).astype(F)
    counts, _ = scene.overlap_boxes(lo, hi, capacity=0)
    free = np.nonzero(counts == 0)[0][:64]
    assert len(free) == 64
    lo, hi = lo[free].copy(), hi[free].copy()
    vel = np.zeros((64, 3), F)
    heading = rng.uniform(0.0, 2.0 * np.pi, 64)
    dt, skin, landed = F(1.0 / 30.0), F(1e-3), 0
    for step in range(256):
        vel[:, 0], vel[:, 2] = 4.0 * np.cos(heading), 4.0 * np.sin(heading)
        vel[:, 1] -= F(9.8) * dt
        for k in (1, 0, 2):
            d = np.zeros((64, 3), F)
            d[:, k] = vel[:, k] * dt
            h = scene.sweep_boxes(lo, hi, d)
            move = d[:, k] * h["t"]
            hit = h["instance"] != NO_HIT
            move = np.where(hit, np.where(move > 0, np.maximum(F(0), move - skin), np.minimum(F(0), move + skin)), move).astype(F)
            lo[:, k] += move
            hi[:, k] += move
            if k == 1:
                landed += int((hit & (h["normal"][:, 1] == 1.0)).sum())
                vel[hit, 1] = 0.0
            else:
                heading[hit] += np.pi / 2
        counts, _ = scene.overlap_boxes(lo, hi, capacity=0, any_hit=True)
        assert not counts.any(), (step, np.nonzero(counts)[0])
    assert landed > 64


# ------------------------------------------------------------------ 6. edits
def test_edit_reaches_the_next_voxel():
    base = P.small_scene(seed=6, n_models=2, n_instances=2)
    desc = scenes.SceneDesc(base.models, base.palette, [(0, base.instances[0][1]), (1, base.instances[1][1])])   # a model per instance
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    wit = SweepWitness(desc)
    mid, t = desc.instances[0]
    xyz = wit.mv[mid][0]
    m = np.asarray(t, np.float64).reshape(3, 4)
    rng = np.random.default_rng(10)
    down = np.array([[0.0, -30.0, 0.0]], F)
    # a point dropping straight down onto a voxel of instance 0 with more of instance 0 below it (a point names one voxel per
    # resting axis, so each answer is unique)
    for _ in range(2000):
        top = m @ np.append(xyz[int(rng.integers(0, len(xyz)))] + 0.5, 1.0)
        p = np.array([np.floor(top[0]) + 0.25, np.floor(top[1]) + 3.0, np.floor(top[2]) + 0.25], F)
        first = wit.exact(p, p, down[0])
        if first["instance"] == 0 and first["t"] > 0:
            q = (p + [0.0, -30.0 * float(first["t"]) - 1.5, 0.0]).astype(F)
            if wit.exact(q, q, down[0])["instance"] == 0:
                break
    got = scene.sweep_boxes(p[None], p[None], down)[0]
    assert got.tobytes() == first.tobytes()
    scene._models[0].set_voxels(got["xyz"][None].astype(np.uint32), np.array([-1], np.int32))
    with pytest.raises(L.DustError) as e:
        scene.sweep_boxes(p[None], p[None], down)
    assert e.value.status == L.ERR_NOT_READY
    scene.commit()
    after = scene.sweep_boxes(p[None], p[None], down)[0]
    keep = ~np.all(xyz == got["xyz"].astype(np.int64), axis=1)     # the witness without the removed voxel
    wit.mv[mid] = tuple(a[keep] for a in wit.mv[mid])
    wit.inst[0] = (True, wit.inst[0][1][keep], wit.inst[0][2][keep])
    want = wit.exact(p, p, down[0])
    assert want["instance"] != NO_HIT and want["t"] > got["t"]
    for f in ("t", "instance", "xyz", "palette", "voxel", "normal"):   # (block numbers may move with the edit)
        assert np.array_equal(after[f], want[f]), (f, after, want)


# ------------------------------------------------------------------ 7. the device path, n == 0, alignment; determinism; empty scene
def test_async_path_matches_sync(castle):
    import torch
    ctx, scene, desc, wit = castle
    lo, hi, d = castle_sweeps(np.random.default_rng(11), desc, 3000)
    host = scene.sweep_boxes(lo, hi, d)
    host_any = scene.sweep_boxes(lo, hi, d, any_hit=True, ignore_start=True)
    dev = torch.from_numpy(api.box_sweeps(lo, hi, d).view(np.int32).reshape(-1, 12).copy()).to("cuda")
    pipe = api.StandardPipeline(ctx, 64, 48)   # enqueued behind a rendered frame
    pipe.render(scene, P.camera_for((140.0, 80.0, 100.0)), P.sky_state(), L.PASS_PRIMARY, frame_index=1)
    outs = []
    for any_hit in (False, True):
        hits = torch.zeros((len(lo), 8), dtype=torch.int32, device="cuda")
        scene.sweep_boxes(dev, hits=hits, any_hit=any_hit, ignore_start=any_hit)
        outs.append(hits)
    ctx.sync()
    assert outs[0].cpu().numpy().tobytes() == host.tobytes()
    assert outs[1].cpu().numpy().tobytes() == host_any.tobytes()
    lib = L.load()
    assert lib.dust_hip_scene_sweep_boxes_async(scene._h, None, None, 0, 0) == L.OK
    assert lib.dust_hip_scene_sweep_boxes(scene._h, None, None, 0, 0) == L.OK
    assert lib.dust_hip_scene_sweep_boxes(scene._h, None, None, 3, 0) == L.ERR_INVALID_ARGUMENT
    buf = torch.zeros(64 * 12 + 4, dtype=torch.int32, device="cuda")
    out = torch.zeros(64 * 8 + 4, dtype=torch.int32, device="cuda")
    fn = lib.dust_hip_scene_sweep_boxes_async
    assert fn(scene._h, C.c_void_p(buf.data_ptr() + 4), C.c_void_p(out.data_ptr()), 64, 0) == L.ERR_INVALID_ARGUMENT
    assert fn(scene._h, C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr() + 8), 64, 0) == L.ERR_INVALID_ARGUMENT
    sweeps = api.box_sweeps(lo[:4], hi[:4], d[:4])
    h4 = np.zeros(4, api.SWEEP_HIT_DTYPE)
    assert lib.dust_hip_scene_sweep_boxes(scene._h, sweeps.ctypes.data_as(C.c_void_p), h4.ctypes.data_as(C.c_void_p), 4, 4) == L.ERR_INVALID_ARGUMENT
    ctx.sync()


def test_two_runs_give_the_same_bytes(castle):
    ctx, scene, desc, wit = castle
    lo, hi, d = castle_sweeps(np.random.default_rng(12), desc, 4000)
    a = scene.sweep_boxes(lo, hi, d)
    b = scene.sweep_boxes(lo, hi, d)
    assert a.tobytes() == b.tobytes()


def test_empty_scene_misses():
    ctx = api.Context(device=0)
    scene = api.Scene(ctx)
    scene.commit()
    got = scene.sweep_boxes(np.zeros((5, 3)), np.ones((5, 3)), np.full((5, 3), 3.0))
    assert got.tobytes() == miss().tobytes() * 5
