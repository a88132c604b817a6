"""One set-up per tile for the members of a view run (k_primary_ao_runs, view_run_packet, trace_run_ray): a tile whose AO candidate list holds
exactly ONE instance works out once which instance that is, where its record lies and the rays' origins in its object space; every member then
goes straight to its own direction, the world-box test and the walk. Lists of two or more, overflowing lists and DUST_HIP_DEBUG bit 64 walk the
list as before. dust_hip_render_frame knows nothing of runs, so every plane of every member must hold the bits the same frame holds when it is
rendered alone on a twin pipeline with the same past -- with the one set-up and, bit 64, without it."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import parity_util as P
from dust_amd import _lib as L
from dust_amd import api, synth
from test_gpu_many_instances import scattered_scene

gpu = pytest.mark.gpu

PAO = L.PASS_PRIMARY | L.PASS_AMBIENT_OCCLUSION
PLANES = [pid for _, pid in P.PLANES]
W, H = 64, 40            # 8 x 5 tiles
TILE = 8                 # dust_dev.h: kTileW, kTileH
AO_REACH = 8.0
GENERAL = "64"           # DUST_HIP_DEBUG bit 64: every tile walks its list


@functools.lru_cache(maxsize=None)
def _noise(layers=4):
    n5 = synth.stbn_unitvec3_cosine(layers=layers)
    n5.setflags(write=False)
    return n5


def _pipes(ctx, n, n5, w=W, h=H):
    out = []
    for _ in range(n):
        p = api.StandardPipeline(ctx, w, h)
        p.set_noise(5, n5)
        out.append(p)
    return out


def _same(batch, single, what):
    for i, (b, s) in enumerate(zip(batch, single)):
        for pl in PLANES:
            x, y = b.read_plane(pl), s.read_plane(pl)
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}, frame {i}: plane {pl} differs in {int(np.count_nonzero(x != y))} values"


def _check(monkeypatch, ctx, scene, cams, sky, idx, rnd, rows=(0, 0), layers=4):
    """the frames alone on pipelines of their own, then in ONE launch with the tile set-up and in one launch without it: seven planes, byte by byte"""
    n5 = _noise(layers)
    n = len(idx)
    cams = cams if isinstance(cams, list) else [cams] * n
    monkeypatch.delenv("DUST_HIP_DEBUG", raising=False)
    single = _pipes(ctx, n, n5)
    for i, p in enumerate(single):
        p.render(scene, cams[i], sky, PAO, frame_index=idx[i], rand=rnd[i], rows=rows)
    for dbg in (None, GENERAL):
        if dbg:
            monkeypatch.setenv("DUST_HIP_DEBUG", dbg)
        batch = _pipes(ctx, n, n5)
        api.StandardPipeline.render_frames(batch, scene, cams, sky, PAO, idx, rnd, rows=rows)
        monkeypatch.delenv("DUST_HIP_DEBUG", raising=False)
        _same(batch, single, f"launch of {n}, DUST_HIP_DEBUG={dbg}")
    return single


def _frames(first, n, seed):
    idx = [first + i for i in range(n)]
    return idx, [synth.frame_rand(seed, f) for f in idx]


# ---------------------------------------------------------------- scenes
def _at(offset, rot=None):
    m = np.zeros((3, 4), np.float32)
    m[:, :3] = np.eye(3) if rot is None else rot
    m[:, 3] = offset
    return m.reshape(12)


def _model(seed, size, fill=0.45, blobs=4):
    rng = np.random.default_rng(seed)
    pal = synth.make_palette(seed)
    return api.flatten_model(P.random_model(rng, size, fill=fill, blobs=blobs), size, pal), pal


def one_instance_scene():
    m, pal = _model(31, (40, 32, 24))
    return P.SceneDesc([m], pal, [(0, _at((-20.0, -16.0, -12.0)))])


def two_instance_scene():
    """two instances side by side, 2 voxels apart: the tiles over the middle of the frame have both boxes within the AO rays' reach, the outer ones one"""
    m, pal = _model(32, (24, 32, 24))
    return P.SceneDesc([m], pal, [(0, _at((-25.0, -16.0, -12.0))), (0, _at((1.0, -16.0, -12.0)))])


def rotated_scaled_scene():
    """rotated about two axes, scale 1.25: object-space origins and directions are not the world's"""
    m, pal = _model(33, (32, 32, 24))
    a, b = 0.4, 0.7
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    r = (rx @ ry * 1.25).astype(np.float32)
    off = -(r @ np.array([16.0, 16.0, 12.0], np.float32))
    return P.SceneDesc([m], pal, [(0, _at(off, r))])


BLOCK_AT, BLOCK_SIZE = (-12.0, -8.0, -12.0), (24, 16, 24)


def solid_block_scene():
    """a solid block with a step cut into its top: its outer faces are its box's, so hit point + 0.01 n lies OUTSIDE the instance's box and the
    world-box test decides which lanes enter; AO rays from the step's tread can hit its riser"""
    size = BLOCK_SIZE
    x, y, z = np.meshgrid(*[np.arange(s) for s in size], indexing="ij")
    keep = (y < 8) | (x < 12)
    x, y, z = x[keep], y[keep], z[keep]
    xyzi = np.stack([x.ravel(), y.ravel(), z.ravel(), (x.ravel() * 7 + z.ravel()) % 255], axis=1).astype(np.uint8)
    pal = synth.make_palette(34)
    return P.SceneDesc([api.flatten_model(xyzi, size, pal)], pal, [(0, _at(BLOCK_AT))])


FRONT = (3.0, 5.0, -30.0)   # close enough that the one- and two-instance scenes fill all 40 tiles


# ---------------------------------------------------------------- the test's own premise, on the host
def _world_boxes(desc):
    lo, hi, bounds = [], [], []
    for blocks, _ in desc.models:
        b = np.stack([blocks["x"], blocks["y"], blocks["z"]], axis=1).astype(np.float64)
        bounds.append((b.min(axis=0), b.max(axis=0) + 4.0))
    for mid, t in desc.instances:
        m = np.asarray(t, np.float64).reshape(3, 4)
        bmin, bmax = bounds[mid]
        corners = np.array([[(bmax if (c >> a) & 1 else bmin)[a] for a in range(3)] for c in range(8)])
        wc = corners @ m[:, :3].T + m[:, 3]
        lo.append(wc.min(axis=0))
        hi.append(wc.max(axis=0))
    return np.array(lo), np.array(hi)


def _hit_points(cam, depth):
    h, w = depth.shape
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    tan = float(cam.tan_half_fov)
    cx = (2.0 * (px + 0.5) / w - 1.0) * (w / h) * tan
    cy = -(2.0 * (py + 0.5) / h - 1.0) * tan
    c0, c1, c2 = (np.array(list(v), np.float64) for v in (cam.view_col0, cam.view_col1, cam.view_col2))
    d = cx[..., None] * c0 + cy[..., None] * c1 - c2
    return np.array(list(cam.position), np.float64) + depth.astype(np.float64)[..., None] * d


def _boxes_in_reach_per_tile(desc, cam, slack):
    """per tile of the frame: how many world boxes lie within Chebyshev distance AO_REACH + slack of the box of the tile's hit points (the cull's
    test; slack = -0.1 counts only what it must keep, +0.1 everything it may keep); -1 for a tile without a hit. The depth plane is the ORACLE's."""
    g = P.render_oracle(P.oracle_scene(desc), cam, P.sky_state(), W, H, L.PASS_PRIMARY)
    depth = g.depth
    blo, bhi = _world_boxes(desc)
    pts = _hit_points(cam, depth)
    out = []
    for ty in range(0, H, TILE):
        for tx in range(0, W, TILE):
            ok = np.isfinite(depth[ty:ty + TILE, tx:tx + TILE])
            if not ok.any():
                out.append(-1)
                continue
            p = pts[ty:ty + TILE, tx:tx + TILE][ok]
            gap = np.maximum(np.maximum(blo - p.max(axis=0), p.min(axis=0) - bhi), 0.0).max(axis=1)
            out.append(int(np.count_nonzero(gap <= AO_REACH + slack)))
    return np.array(out)


def test_the_scenes_have_the_tiles_the_cases_are_about():
    """one instance: every tile has one box within reach; two instances: at least a quarter of the frame's tiles surely keep both boxes and at least
    a quarter can keep only one -- both paths in one frame, in tiles next to each other"""
    cam = P.camera_for(FRONT)
    one = _boxes_in_reach_per_tile(one_instance_scene(), cam, -0.1)
    assert (one == 1).all(), one
    must = _boxes_in_reach_per_tile(two_instance_scene(), cam, -0.1)
    may = _boxes_in_reach_per_tile(two_instance_scene(), cam, 0.1)
    n = len(must)
    print("two instances: tiles that must keep both", int((must == 2).sum()), "tiles that can keep one only", int((may == 1).sum()), "of", n)
    assert (must == 2).sum() * 4 >= n and (may == 1).sum() * 4 >= n, (must, may)
    grid_two, grid_one = (must == 2).reshape(H // TILE, W // TILE), (may == 1).reshape(H // TILE, W // TILE)
    assert (grid_two[:, 1:] & grid_one[:, :-1]).any() or (grid_two[:, :-1] & grid_one[:, 1:]).any(), "no one-candidate tile beside a two-candidate tile"


# ---------------------------------------------------------------- runs of 2, 5 and 8
@gpu
@pytest.mark.parametrize("n", [2, 5, 8])
@pytest.mark.parametrize("which", ["one_instance", "two_instances", "rotated_scaled", "face_on_the_box"])
def test_members_of_a_run_equal_single_frames(monkeypatch, which, n):
    desc = {"one_instance": one_instance_scene, "two_instances": two_instance_scene, "rotated_scaled": rotated_scaled_scene,
            "face_on_the_box": solid_block_scene}[which]()
    ctx = api.Context(device=0)
    scene, sky, cam = P.hip_scene(ctx, desc), P.sky_state(), P.camera_for(FRONT)
    idx, rnd = _frames(3, n, 6)
    single = _check(monkeypatch, ctx, scene, cam, sky, idx, rnd)
    depth = single[0].read_plane(L.PLANE_DEPTH)
    assert np.isfinite(depth).sum() * 2 > depth.size, "the view misses the scene"
    if which == "face_on_the_box":   # the premise: the front face, seen by a quarter of the pixels at least, lies in the box's z = -12 plane
        on_face = np.isfinite(depth) & (np.abs(_hit_points(cam, depth)[..., 2] - BLOCK_AT[2]) < 1e-3)
        assert on_face.sum() * 4 >= depth.size, int(on_face.sum())
    else:
        ao = single[n - 1].read_plane(L.PLANE_ILLUMINANCE)
        assert ao[..., 3].any(), "no AO ray of the last member hit anything"


@gpu
def test_deep_tree(monkeypatch):
    """test_gpu_shared_view.test_one_view_of_a_deep_tree's model (4096^3, k_primary_ao_runs<2>): one instance, every tile sets up once"""
    from test_configs import deep_desc
    blocks, mats, pal = deep_desc(1e-4)
    ctx = api.Context(device=0)
    model = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    scene = api.Scene(ctx)
    xf = np.eye(3, 4, dtype=np.float32)
    xf[:, 3] = (-2048.0, -2048.0, -2048.0)
    scene.add_instance(model, xf.reshape(12))
    scene.commit()
    single = _check(monkeypatch, ctx, scene, P.camera_for((2600.0, 1900.0, 2300.0)), P.sky_state(), [1, 2, 3, 4, 5], [5, 6, 7, 8, 9], layers=2)
    assert np.isfinite(single[0].read_plane(L.PLANE_DEPTH)).any()


@gpu
def test_large_scene(monkeypatch):
    """more than kFlatCullMax instances (k_primary_ao_runs<4>): lists of one, of several and none in one frame"""
    desc = scattered_scene(1500)
    ctx = api.Context(device=0)
    idx, rnd = _frames(2, 5, 9)
    single = _check(monkeypatch, ctx, P.hip_scene(ctx, desc), P.camera_for((180.0, 90.0, 260.0)), P.sky_state(), idx, rnd)
    assert np.isfinite(single[0].read_plane(L.PLANE_DEPTH)).any()


@gpu
def test_row_band(monkeypatch):
    desc = two_instance_scene()
    ctx = api.Context(device=0)
    idx, rnd = _frames(3, 5, 7)
    single = _check(monkeypatch, ctx, P.hip_scene(ctx, desc), P.camera_for(FRONT), P.sky_state(), idx, rnd, rows=(8, 32))
    d = single[4].read_plane(L.PLANE_DEPTH)
    assert not d[:8].any() and not d[32:].any() and d[8:32].any()


@gpu
def test_mixed_launch(monkeypatch):
    """A A B B B A: a run of two, a run of three and a lone frame, each with its own tiles' set-ups"""
    desc = two_instance_scene()
    ctx = api.Context(device=0)
    A, B = P.camera_for(FRONT), P.camera_for((-40.0, 30.0, -50.0))
    idx, rnd = _frames(21, 6, 4)
    _check(monkeypatch, ctx, P.hip_scene(ctx, desc), [A, A, B, B, B, A], P.sky_state(), idx, rnd)


@gpu
def test_view_turned_away(monkeypatch):
    """no live pixel: no tile culls for its AO rays, none sets anything up, nothing is stored to illuminance"""
    desc = one_instance_scene()
    ctx = api.Context(device=0)
    away = P.camera_for(FRONT, target=(2.0 * FRONT[0], 2.0 * FRONT[1] + 40.0, 2.0 * FRONT[2]))
    idx, rnd = _frames(5, 8, 2)
    single = _check(monkeypatch, ctx, P.hip_scene(ctx, desc), away, P.sky_state(), idx, rnd)
    assert not np.isfinite(single[0].read_plane(L.PLANE_DEPTH)).any()
