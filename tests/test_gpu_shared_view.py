"""Same-view frames of one persistent launch (dust_hip_render_frames, k_primary_ao_runs): consecutive frames with a byte-identical camera
and sky that read the same scene image form a VIEW RUN -- N samples per pixel of one view are N frames with a fresh frame_index and rand,
nothing else. The camera ray, the shading and the sun ray of a run are traced once and written to every member's planes; only the AO ray is
each frame's own. Every plane of every frame must hold the bits the same frame holds when dust_hip_render_frame renders it alone, and at
least one frame per case is compared against the oracle -- for runs of every length, mixed launches, and every kernel variant."""
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
EYE_A, EYE_B = (90.0, 60.0, -80.0), (70.0, 85.0, -60.0)


def _pipes(ctx, n, w, h, n5):
    out = []
    for _ in range(n):
        p = api.StandardPipeline(ctx, w, h)
        p.set_noise(5, n5)
        out.append(p)
    return out


def _planes(pipe):
    return [pipe.read_plane(pl) for pl in PLANES]


def _same(a, b, what):
    for pl, x, y in zip(PLANES, a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: plane {pl} differs in {int(np.count_nonzero(x != y))} values"


def _alone(ctx, scene, cams, skies, w, h, n5, idx, rnd, rows=(0, 0), single=None):
    """the same frames, one dust_hip_render_frame each on pipelines of their own (`single`: the twins of pipelines that have rendered before --
    a frame leaves the illuminance, normal and voxel-id texels of its miss pixels as they were, so a twin must have the same past)"""
    single = single or _pipes(ctx, len(idx), w, h, n5)
    for i, p in enumerate(single):
        p.render(scene, cams[i], skies[i], PAO, frame_index=idx[i], rand=rnd[i], rows=rows)
    return single


def _oracle(oscene, cam, sky, w, h, n5, layers, frame_index, rand, pipe):
    g = P.render_oracle(oscene, cam, sky, w, h, PAO, n5[frame_index % layers], rand)
    P.assert_parity(P.compare_gbuffers(g, P.read_hip_gbuffer(pipe)))


@pytest.mark.parametrize("n", [2, 3, 5, 8, 11])
def test_frames_of_one_view_equal_single_frames_and_the_oracle(n):
    """n frames of ONE camera with distinct frame_index and rand at a frame size that leaves ragged tiles (11: a run of 8 and one of 3). A
    follower of a run takes no tile order and measures nothing: its pipeline's cost map stays unmeasured, the leader's is written."""
    w, h = 203, 117
    desc = P.small_scene(seed=5, n_models=3, n_instances=7)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    oscene = P.oracle_scene(desc)
    sky = P.sky_state()
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    cam = P.camera_for(EYE_A)
    idx = [7 + i for i in range(n)]
    rnd = [synth.frame_rand(3, f) for f in idx]
    batch = _pipes(ctx, n, w, h, n5)
    api.StandardPipeline.render_frames(batch, scene, cam, sky, PAO, idx, rnd)
    single = _alone(ctx, scene, [cam] * n, [sky] * n, w, h, n5, idx, rnd)
    for i in range(n):
        _same(_planes(batch[i]), _planes(single[i]), f"frame {i} of {n}")
    for i in (0, n - 1):
        _oracle(oscene, cam, sky, w, h, n5, 4, idx[i], rnd[i], batch[i])
    assert batch[0].tile_costs(0) is not None and batch[0].tile_costs(0).any()   # the leader's cost map took the run's tile times
    assert batch[1].tile_costs(0) is None                                        # a follower's was never written: not marked measured
    # the frames differ (their AO rays do) and share what the view decides
    a, b = _planes(batch[0]), _planes(batch[1])
    assert not np.array_equal(a[0], b[0])
    for k in range(1, len(PLANES)):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))


def test_mixed_launch_of_runs_and_lone_frames():
    """cameras A A B B B A in one launch: a run of two, a run of three, a run of one -- and A B A B A B A B, eight runs of one in the run kernel's
    place (no sharing: today's kernel)."""
    w, h = 203, 117
    desc = P.small_scene(seed=5, n_models=3, n_instances=7)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    oscene = P.oracle_scene(desc)
    sky = P.sky_state()
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    A, B = P.camera_for(EYE_A), P.camera_for(EYE_B)
    for cams in ([A, A, B, B, B, A], [A, B, B, B, B, B, B, A], [A, B, A, B, A, B, A, B]):
        n = len(cams)
        idx = [21 + i for i in range(n)]
        rnd = [synth.frame_rand(4, f) for f in idx]
        batch = _pipes(ctx, n, w, h, n5)
        api.StandardPipeline.render_frames(batch, scene, cams, sky, PAO, idx, rnd)
        single = _alone(ctx, scene, cams, [sky] * n, w, h, n5, idx, rnd)
        for i in range(n):
            _same(_planes(batch[i]), _planes(single[i]), f"frame {i} of {n} (mixed)")
        for i in (1, n - 1):
            _oracle(oscene, cams[i], sky, w, h, n5, 4, idx[i], rnd[i], batch[i])


def test_equal_cameras_with_different_skies_share_nothing():
    """the sun direction decides the sun ray and the sky the miss pixels: frames of one camera whose skies differ are runs of one (every
    pipeline measures its own tiles, as in a launch of distinct views); two equal skies in a row share again"""
    w, h = 203, 117
    desc = P.small_scene(seed=5, n_models=3, n_instances=7)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    oscene = P.oracle_scene(desc)
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    cam = P.camera_for(EYE_A)
    s0, s1 = P.sky_state(), P.sky_state("low_sun")
    skies = [s0, s1, s0, s1, s1]
    n = len(skies)
    idx = [3 + i for i in range(n)]
    rnd = [synth.frame_rand(6, f) for f in idx]
    batch = _pipes(ctx, n, w, h, n5)
    api.StandardPipeline.render_frames(batch, scene, cam, skies, PAO, idx, rnd)
    single = _alone(ctx, scene, [cam] * n, skies, w, h, n5, idx, rnd)
    for i in range(n):
        _same(_planes(batch[i]), _planes(single[i]), f"frame {i}, sky {i % 2}")
    for i in (1, 2, 4):
        _oracle(oscene, cam, skies[i], w, h, n5, 4, idx[i], rnd[i], batch[i])
    for i in range(4):
        assert batch[i].tile_costs(0) is not None, f"frame {i} leads a run of its own"
    assert batch[4].tile_costs(0) is None   # ... and the fifth follows the fourth


def _mat4(o2w):
    m = np.eye(4, dtype=np.float32)
    m[:3, :] = np.asarray(o2w, np.float32).reshape(3, 4)
    return np.ascontiguousarray(m.T).reshape(16)


def test_a_move_in_the_middle_splits_the_run():
    """six frames of one camera, an instance moved (and the scene committed) before the fourth: frames 0-2 and 3-5 are two runs on two scene
    images. Against set_transform + commit + render_frame on a twin scene: every plane, motion vectors included; twice in a row."""
    w, h = 200, 120
    desc = P.small_scene(seed=6, n_models=3, n_instances=7)
    ctx = api.Context(device=0)
    sky = P.sky_state()
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    scene_a, scene_b = P.hip_scene(ctx, desc), P.hip_scene(ctx, desc)
    cam = P.camera_for(EYE_A)
    n = 6
    batch, single = _pipes(ctx, n, w, h, n5), _pipes(ctx, n, w, h, n5)
    cur = [np.array(t, np.float32).reshape(3, 4).copy() for _, t in desc.instances]
    f = 1
    for call in range(2):
        idx = [f + i for i in range(n)]
        rnd = [synth.frame_rand(2, v) for v in idx]
        j = 2 + call
        prev = _mat4(cur[j])
        cur[j] = cur[j].copy()
        cur[j][:, 3] += np.array((4.0, -2.5, 3.0), np.float32)
        moves = [[], [], [], [(j, cur[j].reshape(12).copy(), prev)], [], []]
        api.StandardPipeline.render_frames(batch, scene_a, cam, sky, PAO, idx, rnd, moves=moves)
        for i in range(n):
            for k, xf, pv in moves[i]:
                scene_b.set_transform(k, xf, pv)
                scene_b.commit()
            single[i].render(scene_b, cam, sky, PAO, frame_index=idx[i], rand=rnd[i])
        for i in range(n):
            _same(_planes(batch[i]), _planes(single[i]), f"call {call}, frame {i} around a move")
        f += n
    # the frame the move landed on carries the moved instance's motion vectors; the run before it does not
    assert not np.array_equal(batch[2].read_plane(L.PLANE_MOTION), batch[3].read_plane(L.PLANE_MOTION))
    final = P.SceneDesc(desc.models, desc.palette, [(m, cur[k].reshape(12)) for k, (m, _) in enumerate(desc.instances)])
    g = P.render_oracle(P.oracle_scene(final), cam, sky, w, h, PAO, n5[idx[n - 1] % 4], rnd[n - 1])
    res = P.compare_gbuffers(g, P.read_hip_gbuffer(batch[n - 1]))
    res["motion"] = 0   # (the oracle scene built at rest has no previous transforms: motion vectors are compared against the twin above)
    P.assert_parity(res)


def test_row_band_of_one_view():
    """four frames of one view on ONE row band: rows outside the band keep what they held, in every member's planes"""
    w, h = 256, 144
    desc = P.small_scene(seed=2, n_models=3, n_instances=6)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    oscene = P.oracle_scene(desc)
    sky = P.sky_state()
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    cam = P.camera_for(EYE_A)
    rows = (40, 104)
    idx = [3, 4, 5, 6]
    batch = _pipes(ctx, 4, w, h, n5)
    api.StandardPipeline.render_frames(batch, scene, cam, sky, PAO, idx, idx, rows=rows)
    single = _alone(ctx, scene, [cam] * 4, [sky] * 4, w, h, n5, idx, idx, rows=rows)
    for i in range(4):
        _same(_planes(batch[i]), _planes(single[i]), f"band frame {i}")
        d = batch[i].read_plane(L.PLANE_DEPTH)
        assert not d[:40].any() and not d[104:].any() and d[40:104].any()
    g = P.render_oracle(oscene, cam, sky, w, h, PAO, n5[idx[2] % 4], idx[2], rows=rows)
    P.assert_parity(P.compare_gbuffers(g, P.read_hip_gbuffer(batch[2])))


def test_one_view_of_a_deep_tree():
    """the DEEP variant (a 4096^3 model): views A A A B B in one launch == alone == oracle"""
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
    n5 = synth.stbn_unitvec3_cosine(layers=2)
    sky = P.sky_state()
    A, B = P.camera_for((2600.0, 1900.0, 2300.0)), P.camera_for((300.0, 200.0, -150.0))
    cams = [A, A, A, B, B]
    w, h = 160, 100
    idx = [1, 2, 3, 4, 5]
    rnd = [5, 6, 7, 8, 9]
    batch = _pipes(ctx, 5, w, h, n5)
    api.StandardPipeline.render_frames(batch, scene, cams, sky, PAO, idx, rnd)
    single = _alone(ctx, scene, cams, [sky] * 5, w, h, n5, idx, rnd)
    for i in range(5):
        _same(_planes(batch[i]), _planes(single[i]), f"deep frame {i}")
    for i in (2, 4):
        _oracle(os_, cams[i], sky, w, h, n5, 2, idx[i], rnd[i], batch[i])


def test_one_view_of_a_large_scene():
    """the LARGE variant (more than 256 instances: the cull's 64-wide hierarchy): views A A A A and then A B B A == alone == oracle"""
    desc = scattered_scene(1500)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    oscene = P.oracle_scene(desc)
    sky = P.sky_state()
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    A, B = P.camera_for((180.0, 90.0, 260.0)), P.camera_for((186.0, 86.0, 263.0))
    w, h = 192, 108
    batch, single = _pipes(ctx, 4, w, h, n5), _pipes(ctx, 4, w, h, n5)
    for cams, idx in (([A, A, A, A], [2, 3, 4, 5]), ([A, B, B, A], [6, 7, 8, 9])):
        rnd = [synth.frame_rand(9, f) for f in idx]
        api.StandardPipeline.render_frames(batch, scene, cams, sky, PAO, idx, rnd)
        _alone(ctx, scene, cams, [sky] * 4, w, h, n5, idx, rnd, single=single)
        for i in range(4):
            _same(_planes(batch[i]), _planes(single[i]), f"large-scene frame {i}")
        _oracle(oscene, cams[2], sky, w, h, n5, 4, idx[2], rnd[2], batch[2])


def test_launches_in_a_row_keep_every_members_counters_and_history():
    """Same-view launches of four on the same pipelines, ten times over (the leader's cost order comes in, its counters alternate, and so do the
    followers' although nobody pulls tiles from theirs); a single-frame call on a follower and on the leader in between; then the same pipelines
    grouped differently -- reversed, so that a former follower leads; two views, so that a former follower leads the second run; distinct views, every
    pipeline on its own order -- and back. Every launch's planes == the same frames alone, on a twin of each pipeline with the same past."""
    w, h = 320, 200
    desc = P.small_scene(seed=8, n_models=4, n_instances=9)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    oscene = P.oracle_scene(desc)
    sky = P.sky_state()
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    A, B = P.camera_for(EYE_A), P.camera_for(EYE_B)
    C_ = [P.camera_for((EYE_A[0] + 3.0 * i, EYE_A[1] - 2.0 * i, EYE_A[2] + 1.5 * i)) for i in range(4)]
    batch = _pipes(ctx, 4, w, h, n5)
    twin = dict(zip(batch, _pipes(ctx, 4, w, h, n5)))
    state = {"f": 1}

    def launch(pipes, cams, what):
        f = state["f"]
        idx = [f + i for i in range(len(pipes))]
        rnd = [synth.frame_rand(5, v) for v in idx]
        api.StandardPipeline.render_frames(pipes, scene, cams, sky, PAO, idx, rnd)
        state["f"] = f + len(pipes)
        for i, p in enumerate(pipes):
            twin[p].render(scene, cams[i], sky, PAO, frame_index=idx[i], rand=rnd[i])
            _same(_planes(p), _planes(twin[p]), f"{what}, frame {i}")
        return idx, rnd

    for k in range(10):
        launch(batch, [A] * 4, f"same-view launch {k}")
        if k == 4:   # a follower, then the leader, render a frame of their own between two launches
            for p, fi in ((batch[2], 999), (batch[0], 1000)):
                p.render(scene, B, sky, PAO, frame_index=fi, rand=17)
                twin[p].render(scene, B, sky, PAO, frame_index=fi, rand=17)
                _same(_planes(p), _planes(twin[p]), "a single frame between two launches")
    assert batch[0].tile_costs(0) is not None
    assert batch[1].tile_costs(0) is None and batch[3].tile_costs(0) is None   # followers all along
    launch(batch[::-1], [A] * 4, "reversed: a former follower leads")
    launch(batch, [A, A, B, B], "two runs: a former follower leads the second")
    launch(batch, [B, A, A, A], "a lone frame and a run of three")
    for k in range(3):
        launch(batch, C_, f"distinct views {k}: every pipeline on its own order")
    for p in batch:
        c = p.tile_costs(0)
        assert c is not None and c.shape == ((h + 7) // 8, (w + 7) // 8) and c.any()
    idx, rnd = launch(batch, [A] * 4, "and one view again")
    for k in range(3):
        idx, rnd = launch(batch[:3], [B] * 3, f"a launch of three {k}")
    _oracle(oscene, B, sky, w, h, n5, 4, idx[2], rnd[2], batch[2])


def test_the_switch_keeps_every_frame_to_itself(monkeypatch):
    """DUST_HIP_NO_SHARED_VIEW (read when a pipeline is created): same-view frames go through k_primary_ao_batch, a frame at a time -- the same
    bits, and every pipeline measures its own tiles. A pipeline made without the switch does not share a launch with one made with it."""
    w, h = 203, 117
    desc = P.small_scene(seed=5, n_models=3, n_instances=7)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    oscene = P.oracle_scene(desc)
    sky = P.sky_state()
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    cam = P.camera_for(EYE_A)
    n = 5
    idx = [7 + i for i in range(n)]
    rnd = [synth.frame_rand(3, f) for f in idx]
    shared = _pipes(ctx, n, w, h, n5)
    monkeypatch.setenv("DUST_HIP_NO_SHARED_VIEW", "1")
    apart = _pipes(ctx, n, w, h, n5)
    monkeypatch.delenv("DUST_HIP_NO_SHARED_VIEW")
    api.StandardPipeline.render_frames(shared, scene, cam, sky, PAO, idx, rnd)
    api.StandardPipeline.render_frames(apart, scene, cam, sky, PAO, idx, rnd)
    for i in range(n):
        _same(_planes(apart[i]), _planes(shared[i]), f"frame {i} with and without the switch")
        assert apart[i].tile_costs(0) is not None
    assert shared[1].tile_costs(0) is None
    single = _alone(ctx, scene, [cam] * n, [sky] * n, w, h, n5, idx, rnd)
    for i in range(n):
        _same(_planes(apart[i]), _planes(single[i]), f"frame {i} with the switch")
    _oracle(oscene, cam, sky, w, h, n5, 4, idx[3], rnd[3], apart[3])
    # pipelines of both kinds in one call: launches of their own kind, the same planes
    both = [shared[0], shared[1], apart[0], apart[1]]
    idx2 = [31, 32, 33, 34]
    api.StandardPipeline.render_frames(both, scene, cam, sky, PAO, idx2, idx2)
    _alone(ctx, scene, [cam] * 4, [sky] * 4, w, h, n5, idx2, idx2, single=single[:4])   # (twins with the same past: this view, rendered once)
    for i in range(4):
        _same(_planes(both[i]), _planes(single[i]), f"frame {i} of a call of both kinds")
