"""One AO cull per tile and view run (k_primary_ao_runs, view_run_packet): the members of a run trace their AO rays through ONE candidate list,
built for every unit direction from the tile's hit points -- a superset of the list each member's own directions would give, in another order.
dust_hip_render_frame still culls per frame, so every plane of every frame of a render_frames launch must hold the bits the same frame holds
when it is rendered alone (fresh pipelines on both sides: the same past), and one frame per case is compared against the oracle. The cases are
the paths the list takes: lists longer than one and instances that touch, overlap or coincide (ties at equal t), lists that overflow (flat: every
instance is walked; LARGE: the groups of the mask behind the list), the DEEP variant, tiles and views without a live pixel, a row band, a mixed launch."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import parity_util as P
from dust_amd import _lib as L
from dust_amd import api, synth
from test_gpu_many_instances import scattered_scene

pytestmark = pytest.mark.gpu

PAO = L.PASS_PRIMARY | L.PASS_AMBIENT_OCCLUSION
PLANES = [pid for _, pid in P.PLANES]
W, H = 203, 117          # ragged tiles on both edges
TILE = 8                 # pixels of a ray packet each way (dust_dev.h: kTileW, kTileH)
MAX_CAND = 160           # dust_dev.h: kMaxCand
AO_REACH = 8.0           # the AO ray's tmax
EYE_A, EYE_B = (90.0, 60.0, -80.0), (70.0, 85.0, -60.0)


@functools.lru_cache(maxsize=None)
def _noise(layers=4):
    n5 = synth.stbn_unitvec3_cosine(layers=layers)
    n5.setflags(write=False)
    return n5


def _pipes(ctx, n, w, h, n5):
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


def _launch_and_twins(ctx, scene, cams, sky, idx, rnd, w=W, h=H, rows=(0, 0), layers=4):
    """the frames in ONE render_frames launch, and each alone on a pipeline of its own; every plane compared byte by byte"""
    n5 = _noise(layers)
    n = len(idx)
    cams = cams if isinstance(cams, list) else [cams] * n
    batch, single = _pipes(ctx, n, w, h, n5), _pipes(ctx, n, w, h, n5)
    api.StandardPipeline.render_frames(batch, scene, cams, sky, PAO, idx, rnd, rows=rows)
    for i, p in enumerate(single):
        p.render(scene, cams[i], sky, PAO, frame_index=idx[i], rand=rnd[i], rows=rows)
    _same(batch, single, f"launch of {n}")
    return batch


def _oracle(oscene, cam, sky, frame_index, rand, pipe, w=W, h=H, rows=None, layers=4):
    g = P.render_oracle(oscene, cam, sky, w, h, PAO, _noise(layers)[frame_index % layers], rand, rows=rows)
    P.assert_parity(P.compare_gbuffers(g, P.read_hip_gbuffer(pipe)))


def _frames(first, n, seed):
    idx = [first + i for i in range(n)]
    return idx, [synth.frame_rand(seed, f) for f in idx]


# ---------------------------------------------------------------- the host's count of the boxes an AO cull must keep
def _world_boxes(desc):
    """every instance's world box as dust_hip_scene_commit derives it, without its padding: the eight corners of the model's brick bounds"""
    lo, hi = [], []
    bounds = []
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
    """world positions of the camera rays' hits (camera.glsl:4-16 in float64; the 0.01 the AO origin is lifted along the normal is left out)"""
    h, w = depth.shape
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    tan = float(cam.tan_half_fov)
    cx = (2.0 * (px + 0.5) / w - 1.0) * (w / h) * tan
    cy = -(2.0 * (py + 0.5) / h - 1.0) * tan
    c0, c1, c2 = (np.array(list(v), np.float64) for v in (cam.view_col0, cam.view_col1, cam.view_col2))
    d = cx[..., None] * c0 + cy[..., None] * c1 - c2
    return np.array(list(cam.position), np.float64) + depth.astype(np.float64)[..., None] * d


def _boxes_in_reach(desc, cam, depth, reach=AO_REACH - 0.1):
    """per tile with a hit: the number of world boxes within Chebyshev distance `reach` of the box of the tile's hit points -- a LOWER bound of
    what the AO cull keeps (unpadded boxes, 0.1 off the reach for the float64 restatement of the hit points). The largest count of the frame."""
    blo, bhi = _world_boxes(desc)
    pts = _hit_points(cam, depth)
    h, w = depth.shape
    best = 0
    for ty in range(0, h, TILE):
        for tx in range(0, w, TILE):
            t = depth[ty:ty + TILE, tx:tx + TILE]
            ok = np.isfinite(t)
            if not ok.any():
                continue
            p = pts[ty:ty + TILE, tx:tx + TILE][ok]
            plo, phi = p.min(axis=0), p.max(axis=0)
            gap = np.maximum(np.maximum(blo - phi, plo - bhi), 0.0).max(axis=1)
            best = max(best, int(np.count_nonzero(gap <= reach)))
    return best


# ---------------------------------------------------------------- scenes
def touching_scene():
    """instances of two models on ONE voxel grid with the same orientation: side by side (box faces shared), shifted by whole voxels into each
    other (voxel faces of different instances in one plane: hits at equal t) and one exact duplicate (every hit is a tie)"""
    rng = np.random.default_rng(21)
    pal = synth.make_palette(21)
    models = []
    for sz in ((32, 24, 28), (24, 24, 24)):
        models.append(api.flatten_model(P.random_model(rng, sz, fill=0.12, blobs=5), sz, pal))
    places = [(0, (-30, -10, -20)), (0, (2, -10, -20)), (0, (-22, -4, -12)), (1, (-30, 14, -20)), (1, (-18, 14, -20)),
              (1, (2, 2, 8)), (1, (2, 2, 8)), (0, (-30, -10, 8))]
    instances = []
    for mid, at in places:
        m = np.zeros((3, 4), np.float32)
        m[:, :3] = np.eye(3)
        m[:, 3] = at
        instances.append((mid, m.reshape(12)))
    return P.SceneDesc(models, pal, instances)


def clustered_scene(n):
    """scattered_scene's instances drawn into a few voxels' span: every box holds a point near the origin"""
    return scattered_scene(n, seed=13, span=(6.0, 4.0, 6.0))


BELOW = (34.0, -46.0, -30.0)   # the cluster seen from under it: the instances' lowest layers, all of them near the origin, fill the middle of the frame


# ---------------------------------------------------------------- 1. lists longer than one
@pytest.mark.parametrize("n", [8, 11])
@pytest.mark.parametrize("which", ["seven_instances", "touching"])
def test_lists_longer_than_one(which, n):
    """a run of 8, and 11 frames = a run of 8 and a run of 3"""
    desc = P.small_scene(seed=5, n_models=3, n_instances=7) if which == "seven_instances" else touching_scene()
    ctx = api.Context(device=0)
    scene, sky, cam = P.hip_scene(ctx, desc), P.sky_state(), P.camera_for(EYE_A)
    idx, rnd = _frames(7, n, 3)
    batch = _launch_and_twins(ctx, scene, cam, sky, idx, rnd)
    depth = batch[0].read_plane(L.PLANE_DEPTH)
    assert _boxes_in_reach(desc, cam, depth) > 1, "no tile with more than one box in reach of its AO rays"
    _oracle(P.oracle_scene(desc), cam, sky, idx[n - 1], rnd[n - 1], batch[n - 1])


# ---------------------------------------------------------------- 2. + 3. lists that overflow
@pytest.mark.parametrize("n_instances", [256, 420])
def test_overflowing_lists(n_instances):
    """more than kMaxCand boxes in reach of one tile's AO rays: 256 instances (flat cull: trace_ray walks every instance) and 420 (LARGE,
    k_primary_ao_runs<4>: the groups of the mask behind the list). The count is made on the host from the instance boxes and the depth plane."""
    desc = clustered_scene(n_instances)
    ctx = api.Context(device=0)
    scene, sky, cam = P.hip_scene(ctx, desc), P.sky_state(), P.camera_for(BELOW)
    idx, rnd = _frames(4, 3, 8)
    batch = _launch_and_twins(ctx, scene, cam, sky, idx, rnd)
    reach = _boxes_in_reach(desc, cam, batch[0].read_plane(L.PLANE_DEPTH))
    print(f"{n_instances} instances: {reach} boxes in reach of one tile's AO rays")
    assert reach > MAX_CAND, f"only {reach} boxes in reach of a tile: the list does not overflow"
    _oracle(P.oracle_scene(desc), cam, sky, idx[1], rnd[1], batch[1])


def test_large_scene_unclustered():
    """scattered_scene(1500): the 64-wide hierarchy with lists that fit"""
    desc = scattered_scene(1500)
    ctx = api.Context(device=0)
    scene, sky, cam = P.hip_scene(ctx, desc), P.sky_state(), P.camera_for((180.0, 90.0, 260.0))
    idx, rnd = _frames(2, 3, 9)
    batch = _launch_and_twins(ctx, scene, cam, sky, idx, rnd)
    _oracle(P.oracle_scene(desc), cam, sky, idx[2], rnd[2], batch[2])


# ---------------------------------------------------------------- 4. DEEP
def test_deep_tree_run_of_three():
    """test_gpu_shared_view.test_one_view_of_a_deep_tree's scene (a 4096^3 model, k_primary_ao_runs<2>) as a run of 3"""
    from test_configs import deep_desc
    blocks, mats, pal = deep_desc(1e-4)
    ctx = api.Context(device=0)
    model = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    scene = api.Scene(ctx)
    xf = np.eye(3, 4, dtype=np.float32)
    xf[:, 3] = (-2048.0, -2048.0, -2048.0)
    scene.add_instance(model, xf.reshape(12))
    scene.commit()
    os_ = O.Scene()
    os_.add_model(blocks, mats, pal, extent=4096)
    os_.add_instance(0, xf.reshape(12))
    os_.commit()
    sky, cam = P.sky_state(), P.camera_for((2600.0, 1900.0, 2300.0))
    idx, rnd = [1, 2, 3], [5, 6, 7]
    batch = _launch_and_twins(ctx, scene, cam, sky, idx, rnd, layers=2)
    _oracle(os_, cam, sky, idx[2], rnd[2], batch[2], layers=2)


# ---------------------------------------------------------------- 5. nothing to cull for
def test_sky_only_and_tiles_without_a_live_pixel():
    """a view that sees only sky (no tile culls for its AO rays, nothing is stored to illuminance) and a view some of whose tiles see only sky"""
    desc = P.small_scene(seed=5, n_models=3, n_instances=7)
    ctx = api.Context(device=0)
    scene, sky, oscene = P.hip_scene(ctx, desc), P.sky_state(), P.oracle_scene(desc)
    away = P.camera_for(EYE_A, target=(2.0 * EYE_A[0], 2.0 * EYE_A[1] + 40.0, 2.0 * EYE_A[2]))
    idx, rnd = _frames(5, 4, 2)
    batch = _launch_and_twins(ctx, scene, away, sky, idx, rnd)
    assert not np.isfinite(batch[0].read_plane(L.PLANE_DEPTH)).any()
    _oracle(oscene, away, sky, idx[3], rnd[3], batch[3])
    cam = P.camera_for(EYE_A)
    batch = _launch_and_twins(ctx, scene, cam, sky, idx, rnd)
    hit = np.isfinite(batch[0].read_plane(L.PLANE_DEPTH))
    tiles = [hit[y:y + TILE, x:x + TILE].any() for y in range(0, H, TILE) for x in range(0, W, TILE)]
    assert any(tiles) and not all(tiles)
    _oracle(oscene, cam, sky, idx[0], rnd[0], batch[0])


# ---------------------------------------------------------------- 6. a row band
def test_row_band_of_a_run_of_five():
    desc = P.small_scene(seed=2, n_models=3, n_instances=6)
    ctx = api.Context(device=0)
    scene, sky, cam = P.hip_scene(ctx, desc), P.sky_state(), P.camera_for(EYE_A)
    rows = (40, 104)
    idx, rnd = _frames(3, 5, 7)
    batch = _launch_and_twins(ctx, scene, cam, sky, idx, rnd, rows=rows)
    for p in batch:
        d = p.read_plane(L.PLANE_DEPTH)
        assert not d[:40].any() and not d[104:].any() and d[40:104].any()
    _oracle(P.oracle_scene(desc), cam, sky, idx[4], rnd[4], batch[4], rows=rows)


# ---------------------------------------------------------------- 7. a mixed launch
def test_mixed_launch_of_two_cameras():
    """A A B B B A: a run of two, a run of three and a lone frame; every run culls for its own view"""
    desc = touching_scene()
    ctx = api.Context(device=0)
    scene, sky = P.hip_scene(ctx, desc), P.sky_state()
    A, B = P.camera_for(EYE_A), P.camera_for(EYE_B)
    cams = [A, A, B, B, B, A]
    idx, rnd = _frames(21, 6, 4)
    batch = _launch_and_twins(ctx, scene, cams, sky, idx, rnd)
    oscene = P.oracle_scene(desc)
    for i in (1, 4):
        _oracle(oscene, cams[i], sky, idx[i], rnd[i], batch[i])
