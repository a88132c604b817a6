"""Scene ray queries on the device (dust_hip_scene_trace_rays / _async, query.hip): caller-supplied primary-type rays against the committed
scene, bit-exact against the oracle's single-ray trace (orc_trace, hierarchical mode, ray type 0) and against the frame's own planes."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import parity_util as P
from dust_amd import _lib as L
from dust_amd import api, synth
from test_gpu_edit import host_model
from test_gpu_many_instances import scattered_scene

pytestmark = pytest.mark.gpu


def world_bounds(desc):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for mid, t in desc.instances:
        b = desc.models[mid][0]
        m = np.asarray(t, np.float64).reshape(3, 4)
        pts = np.array([[x, y, z] for x in (b["x"].min(), b["x"].max() + 4.0) for y in (b["y"].min(), b["y"].max() + 4.0)
                        for z in (b["z"].min(), b["z"].max() + 4.0)], np.float64)
        w = pts @ m[:, :3].T + m[:, 3]
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    return lo, hi


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def ray_mix(rng, lo, hi, n=600):
    """random rays from outside and from inside the scene's box, axis-aligned and zero-component directions, origins on brick planes,
    tmin / tmax windows: (origins, directions, tmin, tmax)"""
    c, ext = (lo + hi) / 2.0, (hi - lo) / 2.0
    o, d, t0, t1 = [], [], [], []
    k = n // 5
    out = c + unit(rng.normal(size=(k, 3))) * np.linalg.norm(ext) * 1.3          # from outside, towards points inside
    o.append(out); d.append(unit(lo + rng.random((k, 3)) * (hi - lo) - out))
    o.append(lo + rng.random((k, 3)) * (hi - lo)); d.append(unit(rng.normal(size=(k, 3))))   # from inside
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [0, -1, 1], [1, 0, -1]], np.float32)
    o.append(lo + rng.random((k, 3)) * (hi - lo)); d.append(axes[rng.integers(0, len(axes), k)] * np.float32(rng.uniform(0.5, 3.0)))
    plane = lo + rng.random((k, 3)) * (hi - lo)
    ax = int(rng.integers(0, 3))
    plane[:, ax] = np.round(plane[:, ax] / 4.0) * 4.0                                # origins on brick planes, some with zero components
    dd = unit(rng.normal(size=(k, 3)))
    dd[rng.random(k) < 0.5, rng.integers(0, 3)] = 0.0
    dd[np.all(dd == 0, axis=1)] = (0, 1, 0)
    o.append(plane); d.append(dd)
    rest = n - 4 * k
    o.append(c + unit(rng.normal(size=(rest, 3))) * np.linalg.norm(ext) * 1.1); d.append(unit(c - o[-1] + rng.normal(size=(rest, 3)) * ext * 0.3))
    o, d = np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)
    tmin = np.zeros(len(o), np.float32)
    tmax = np.full(len(o), np.float32(1e4))
    win = rng.random(len(o)) < 0.3                                                   # windows that cut hits off
    span = np.float32(np.linalg.norm(hi - lo))
    tmin[win] = rng.uniform(0.0, 0.5, win.sum()).astype(np.float32) * span
    tmax[win] = tmin[win] + rng.uniform(0.0, 0.5, win.sum()).astype(np.float32) * span
    return o, d, tmin, tmax


def inside_solid(scene, o, d, tmin, tmax):
    """rays that start inside a solid voxel: the hit points of the given rays, a third of a voxel further on"""
    h = scene.trace_rays(o, d, tmin, tmax)
    k = h["instance"] != L.NO_HIT
    step = (h["t"][k] + np.float32(0.3) / np.linalg.norm(d[k], axis=1).astype(np.float32))[:, None]
    return (o[k] + d[k] * step).astype(np.float32), d[k], np.zeros(k.sum(), np.float32), np.full(k.sum(), np.float32(1e4))


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def check_records(got, models):
    """every hit names a set voxel of its block (gl_PrimitiveID), at xyz, with the palette index the material stream holds there;
    models: per instance, its model's (blocks, materials)"""
    for g in got[got["instance"] != L.NO_HIT]:
        blocks, mats = models[g["instance"]]
        b = blocks[g["block"]]
        v, mask = int(g["voxel"]), int(b["mask"])
        assert (mask >> v) & 1, g
        assert [int(b["x"]) + (v >> 4), int(b["y"]) + ((v >> 2) & 3), int(b["z"]) + (v & 3)] == [int(x) for x in g["xyz"]], g
        assert mats[int(b["material_ptr"]) + bin(mask & ((1 << v) - 1)).count("1")] == g["palette"], g
        assert g["reserved"] == 0


def check_against_oracle(scene, oscene, o, d, tmin, tmax, any_hit=False, models=None):
    got = scene.trace_rays(o, d, tmin, tmax, any_hit=any_hit)
    closest = scene.trace_rays(o, d, tmin, tmax) if any_hit else got
    n_hit = 0
    for i in range(len(o)):
        ref = oscene.trace(O.ORC_MODE_HIER, 0, 0, o[i], d[i], float(tmin[i]), float(tmax[i]))
        g = got[i]
        if ref is None:
            assert g["instance"] == L.NO_HIT and bits(g["t"]) == bits(tmax[i]), (i, g, o[i], d[i], tmin[i], tmax[i])
            continue
        n_hit += 1
        if any_hit:
            assert g["instance"] != L.NO_HIT and closest[i]["t"] <= g["t"] <= tmax[i] and g["t"] >= tmin[i], (i, g, ref)
        else:
            assert (bits(g["t"]), g["instance"], g["block"], g["voxel"]) == (bits(ref[0]), ref[1], ref[2], ref[3]), (i, g, ref, o[i], d[i])
    # xyz and palette: the voxel the hit names is set, with that colour, in the hit instance's model -- as the Block array has it, and (256^3
    # models) as dust_hip_model_get_voxels reads it back. (A model's first get_voxels moves it into its editable form, which counts as an
    # edit: the scene is committed again.)
    if models is not None:
        check_records(got, models)
    if models is None or all(len(b) == 0 or int(b["x"].max()) < 256 for b, _ in models):
        hit = got["instance"] != L.NO_HIT
        for inst in np.unique(got["instance"][hit]):
            sel = got[got["instance"] == inst]
            assert np.all(scene._models[inst].get_voxels(sel["xyz"]) == sel["palette"])
        scene.commit()
    return got, n_hit


def hip_and_oracle(desc):
    ctx = api.Context(device=0)
    return ctx, P.hip_scene(ctx, desc), P.oracle_scene(desc)


def check_scene(scene, oscene, desc, seed, n=600):
    lo, hi = world_bounds(desc)
    models = [desc.models[mid] for mid, _ in desc.instances]
    rng = np.random.default_rng(seed)
    o, d, t0, t1 = ray_mix(rng, lo, hi, n)
    got, n_hit = check_against_oracle(scene, oscene, o, d, t0, t1, models=models)
    assert n_hit > n // 10
    check_against_oracle(scene, oscene, o, d, t0, t1, any_hit=True, models=models)
    io, idir, i0, i1 = inside_solid(scene, o, d, t0, t1)
    assert len(io) > 10
    check_against_oracle(scene, oscene, io, idir, i0, i1, models=models)
    check_against_oracle(scene, oscene, io, idir, i0, i1, any_hit=True, models=models)


def test_small_scene_matches_oracle():
    desc = P.small_scene(seed=3, n_instances=7)
    ctx, scene, oscene = hip_and_oracle(desc)
    check_scene(scene, oscene, desc, seed=1, n=1000)


def test_large_scene_matches_oracle():
    desc = scattered_scene(4096, seed=11)
    ctx, scene, oscene = hip_and_oracle(desc)
    check_scene(scene, oscene, desc, seed=2, n=500)


def test_scene_without_a_usable_grid_matches_oracle():
    desc = scattered_scene(4200, seed=23, n_models=3, span=(0.0, 0.0, 0.0))   # 4200 boxes round one point: no grid cell can list them
    boxes = []
    for mid, t in desc.instances:
        b, m = desc.models[mid][0], np.asarray(t, np.float64).reshape(3, 4)
        pts = np.array([[x, y, z] for x in (b["x"].min(), b["x"].max() + 4.0) for y in (b["y"].min(), b["y"].max() + 4.0)
                        for z in (b["z"].min(), b["z"].max() + 4.0)], np.float64) @ m[:, :3].T + m[:, 3]
        boxes.append(np.concatenate([pts.min(0), pts.max(0)]))
    with pytest.raises(L.DustError) as e:    # (the commit builds the same grid over the same boxes and marks it unusable)
        api.top_level_build(np.asarray(boxes, np.float32))
    assert e.value.status == L.ERR_UNSUPPORTED
    ctx, scene, oscene = hip_and_oracle(desc)
    check_scene(scene, oscene, desc, seed=3, n=300)


def test_deep_scene_matches_oracle():
    blocks, mats, pal = P.clustered_deep_model()
    ctx = api.Context(device=0)
    model = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    scene = api.Scene(ctx)
    xf = np.eye(3, 4, dtype=np.float32)
    xf[:, 3] = (-2048.0, -2048.0, -2048.0)
    scene.add_instance(model, xf.reshape(12))
    scene.commit()
    oscene = O.Scene()
    oscene.add_model(blocks, mats, pal, extent=4096)
    oscene.add_instance(0, xf.reshape(12))
    oscene.commit()
    rng = np.random.default_rng(4)
    o, d, t0, t1 = ray_mix(rng, np.full(3, 96.0 * 16 - 2048), np.full(3, 160.0 * 16 - 2048), 500)
    _, n_hit = check_against_oracle(scene, oscene, o, d, t0, t1, models=[(blocks, mats)])
    assert n_hit > 50
    check_against_oracle(scene, oscene, o, d, t0, t1, any_hit=True, models=[(blocks, mats)])


def test_degenerate_rays_miss():
    desc = P.small_scene(seed=5)
    ctx, scene, _ = hip_and_oracle(desc)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rays = api.ray_records(np.zeros((8, 3)), np.tile([[0.3, -0.2, 1.0]], (8, 1)), 0.0, 1e4)
    rays["direction"][0] = 0.0
    rays["origin"][1, 0] = nan
    rays["direction"][2, 1] = nan
    rays["direction"][3, 2] = inf
    rays["origin"][4, 1] = -inf
    rays["tmin"][5], rays["tmax"][5] = 10.0, 5.0
    rays["tmax"][6] = nan
    rays["tmin"][7] = -inf
    hits = np.zeros(8, api.HIT_DTYPE)
    L.check(L.load().dust_hip_scene_trace_rays(scene._h, rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), 8, 0))
    assert np.all(hits["instance"] == L.NO_HIT)
    assert np.all(bits(hits["t"]) == bits(rays["tmax"]))


def camera_rays(cam, w, h):
    oc = O.camera_from(cam)
    d = np.zeros((h, w, 3), np.float32)
    out = (C.c_float * 3)()
    for py in range(h):
        for px in range(w):
            O.lib().orc_camera_ray_dir(C.byref(oc), px, py, w, h, out)
            d[py, px] = out[:]
    o = np.tile(np.asarray(cam.position[:], np.float32), (w * h, 1))
    return o, d.reshape(-1, 3)


def unpack_normal(p):
    """nrd.glsl:54-94 of the normal plane, rounded to the axis it stands for -- or the two or three axes: a hit exactly on a voxel's edge or
    corner has CubedNormalize (normal.glsl:39-43) set every component that ties for the largest, and the plane then holds (1, 1, 0) / 2;
    float32 hit points of a 4096^3 tree tie on a few rays in a thousand. Ten bits tell 1/2 or 1/3 from 0 with room to spare."""
    p = np.asarray(p, np.uint32)
    px, py = (p & 1023) / 1023.0 * 2.0 - 1.0, ((p >> 10) & 1023) / 1023.0 * 2.0 - 1.0
    n = np.stack([px, py, 1.0 - np.abs(px) - np.abs(py)], axis=-1)
    t = np.clip(-n[:, 2], 0.0, 1.0)
    n[:, 0] -= t * np.where(n[:, 0] >= 0, 1.0, -1.0)
    n[:, 1] -= t * np.where(n[:, 1] >= 0, 1.0, -1.0)
    return np.sign(n) * (np.abs(n) > 0.5 * np.abs(n).max(axis=1, keepdims=True))


def face_id(n):  # normal.glsl:9-18 on axis normals
    s = np.clip(n.sum(axis=1), 0.0, 1.0)
    return (np.rint(s) + np.rint(np.abs(n[:, 2])) * 4 + np.rint(np.abs(n[:, 1])) * 2).astype(np.uint8)


def frame_and_query_agree(ctx, scene, cam, transforms, w=96, h=64):
    """a w x h primary frame (the packet walk) and the same camera rays through scene.trace_rays (the per-lane walk): the same hit set, t bit for
    bit, voxel id word and face; transforms: per instance, its 3 x 4 matrix. Returns the hit set."""
    pipe = api.StandardPipeline(ctx, w, h)
    pipe.render(scene, cam, P.sky_state(), L.PASS_PRIMARY, frame_index=1)
    depth, vid, nrm = pipe.read_plane(L.PLANE_DEPTH).reshape(-1), pipe.read_plane(L.PLANE_VOXEL_ID).reshape(-1), pipe.read_plane(L.PLANE_NORMAL).reshape(-1)
    o, d = camera_rays(cam, w, h)
    got = scene.trace_rays(o, d, cam.near_, cam.far_)
    hit = got["instance"] != L.NO_HIT
    assert 0.1 < hit.mean() < 0.95
    assert np.array_equal(hit, np.isfinite(depth))
    assert np.array_equal(bits(got["t"][hit]), bits(depth[hit]))
    want = (got["voxel"].astype(np.uint32) << 24) | (got["palette"].astype(np.uint32) << 16) | (got["instance"] & 0xFFFF)
    assert np.array_equal(want[hit], vid[hit])
    # face: the normal plane's world normal rotated into the hit instance's model space
    nw = unpack_normal(nrm[hit])
    rot = np.stack([np.asarray(transforms[i], np.float32).reshape(3, 4)[:, :3] for i in got["instance"][hit]])
    nm = np.einsum("kji,kj->ki", rot, nw)
    assert np.array_equal(face_id(nm), got["face"][hit])
    return hit


def test_camera_rays_reproduce_the_frame():
    desc = P.small_scene(seed=2, n_instances=6)
    ctx, scene, _ = hip_and_oracle(desc)
    frame_and_query_agree(ctx, scene, P.camera_for((150.0, 90.0, 120.0)), [t for _, t in desc.instances])


def test_camera_rays_reproduce_the_frame_in_a_deep_tree():
    """the same in the 4096^3 tree of test_deep_scene_matches_oracle, from outside the cluster: the one place where the packet walk and the
    per-lane walk take whole 16-cells, and refine the near-plane screen for them (walk_cell.hpp, whole_cell_screen), on the same rays. The
    oracle's single-ray trace hits with 5 082 of these 6 144 rays (0.827); both walks must hit with exactly those."""
    blocks, mats, pal = P.clustered_deep_model()
    xf = np.eye(3, 4, dtype=np.float32)
    xf[:, 3] = (-2048.0, -2048.0, -2048.0)
    oscene = O.Scene()
    oscene.add_model(blocks, mats, pal, extent=4096)
    oscene.add_instance(0, xf.reshape(12))
    oscene.commit()
    w, h = 96, 64
    cam = P.camera_for((-620.0, 90.0, 40.0))
    o, d = camera_rays(cam, w, h)
    ref = np.array([oscene.trace(O.ORC_MODE_HIER, 0, 0, o[i], d[i], float(cam.near_), float(cam.far_)) is not None for i in range(w * h)])
    assert 0.1 < ref.mean() < 0.95
    ctx = api.Context(device=0)
    model = api.Model(ctx, blocks, mats, pal, tree_extent_log2=12)
    scene = api.Scene(ctx)
    scene.add_instance(model, xf.reshape(12))
    scene.commit()
    hit = frame_and_query_agree(ctx, scene, cam, [xf.reshape(12)], w, h)
    assert np.array_equal(hit, ref)


def voxels_of(blocks, mats):
    vox = {}
    for b in blocks:
        rank = 0
        for v in range(64):
            if (int(b["mask"]) >> v) & 1:
                vox[(int(b["x"]) + (v >> 4), int(b["y"]) + ((v >> 2) & 3), int(b["z"]) + (v & 3))] = int(mats[int(b["material_ptr"]) + rank])
                rank += 1
    return vox


def test_pick_dig_and_place():
    desc = P.small_scene(seed=6, n_instances=4)
    ctx, scene, _ = hip_and_oracle(desc)
    lo, hi = world_bounds(desc)
    eye = ((lo + hi) / 2 + np.array([0.0, 0.0, 1.5]) * (hi - lo)).astype(np.float32)
    rng = np.random.default_rng(9)
    for _ in range(50):   # the first ray from the eye that hits
        d = unit((lo + rng.random(3) * (hi - lo)) - eye)
        h0 = scene.trace_rays(eye[None], d[None])[0]
        if h0["instance"] != L.NO_HIT:
            break
    assert h0["instance"] != L.NO_HIT
    inst = int(h0["instance"])
    mid = desc.instances[inst][0]
    model = scene._models[inst]
    xyz = [int(v) for v in h0["xyz"]]
    vox = voxels_of(*desc.models[mid])
    assert vox[tuple(xyz)] == h0["palette"]
    # dig: remove the voxel, commit, ask again: the oracle on a host rebuild of the edited voxels
    model.set_voxels([xyz], [-1])
    scene.commit()
    del vox[tuple(xyz)]
    models = list(desc.models)
    models[mid] = host_model(vox, desc.palette)
    oscene = P.oracle_scene(P.SceneDesc(models, desc.palette, desc.instances))
    h1 = scene.trace_rays(eye[None], d[None])[0]
    ref = oscene.trace(O.ORC_MODE_HIER, 0, 0, eye, d, 0.0, float(api.FLT_MAX))
    if ref is None:
        assert h1["instance"] == L.NO_HIT
    else:
        assert (bits(h1["t"]), h1["instance"], h1["block"], h1["voxel"]) == (bits(ref[0]), ref[1], ref[2], ref[3])
    assert not (h1["instance"] == inst and list(h1["xyz"]) == xyz)
    # place: a voxel on the face the first hit came in through; the ray meets it first
    place = list(xyz)
    place[int(h0["face"]) >> 1] += 1 if int(h0["face"]) & 1 else -1
    model.set_voxels([place], [17])
    scene.commit()
    h2 = scene.trace_rays(eye[None], d[None])[0]
    assert h2["instance"] == inst and list(h2["xyz"]) == place and h2["palette"] == 17 and h2["t"] < h0["t"]


def _torch():
    import torch
    return torch


def to_device(rays):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def from_device(t):
    return t.cpu().numpy().reshape(-1).view(api.HIT_DTYPE)


def test_async_queries_read_their_own_commit_across_the_ring():
    """twenty commits of a moving instance, each followed by an asynchronous query, one sync at the end: every result is the oracle's
    on the state committed before it (the scene image is a ring of 16 slots: the queries hold theirs like frames do)"""
    torch = _torch()
    desc = P.small_scene(seed=8, n_instances=5)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    lo, hi = world_bounds(desc)
    rng = np.random.default_rng(12)
    o, d, t0, t1 = ray_mix(rng, lo, hi, 2000)
    rays = to_device(api.ray_records(o, d, t0, t1))
    outs, states = [], []
    base = np.asarray(desc.instances[0][1], np.float32).reshape(3, 4).copy()
    for step in range(20):
        m = base.copy()
        m[:, 3] += np.float32(step * 3.5)
        scene.set_transform(0, m.reshape(12))
        scene.commit()
        hits = torch.zeros((len(o), 8), dtype=torch.int32, device="cuda")
        scene.trace_rays(rays, hits=hits)
        outs.append(hits)
        states.append(m.reshape(12))
    ctx.sync()
    for step in (0, 7, 16, 19):
        inst = list(desc.instances)
        inst[0] = (inst[0][0], states[step])
        oscene = P.oracle_scene(P.SceneDesc(desc.models, desc.palette, inst))
        got = from_device(outs[step])
        for i in range(0, len(o), 4):
            ref = oscene.trace(O.ORC_MODE_HIER, 0, 0, o[i], d[i], float(t0[i]), float(t1[i]))
            g = got[i]
            if ref is None:
                assert g["instance"] == L.NO_HIT, (step, i)
            else:
                assert (bits(g["t"]), g["instance"], g["block"], g["voxel"]) == (bits(ref[0]), ref[1], ref[2], ref[3]), (step, i)


def test_query_between_frames_leaves_the_frames_alone():
    desc = P.small_scene(seed=4)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    n5 = synth.stbn_unitvec3_cosine(layers=4)
    sky, cam = P.sky_state(), P.camera_for((140.0, 80.0, 100.0))
    passes = L.PASS_PRIMARY | L.PASS_AMBIENT_OCCLUSION
    lo, hi = world_bounds(desc)
    o, d, t0, t1 = ray_mix(np.random.default_rng(1), lo, hi, 3000)
    rays = to_device(api.ray_records(o, d, t0, t1))
    hits = _torch().zeros((len(o), 8), dtype=_torch().int32, device="cuda")
    planes = []
    for with_query in (False, True):
        pipe = api.StandardPipeline(ctx, 64, 48)
        pipe.set_noise(5, n5)
        got = []
        for f in (1, 2):
            pipe.render(scene, cam, sky, passes, frame_index=f, rand=synth.frame_rand(2, f))
            if with_query:
                scene.trace_rays(rays, hits=hits)
            got.append([pipe.read_plane(p).tobytes() for _, p in P.PLANES])
        planes.append(got)
    assert planes[0] == planes[1]


@pytest.mark.parametrize("n", [1, 63, 65, 2073600])
def test_host_and_device_paths_agree(n):
    desc = P.small_scene(seed=7)
    ctx, scene, oscene = hip_and_oracle(desc)
    lo, hi = world_bounds(desc)
    rng = np.random.default_rng(n)
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    d = unit(rng.normal(size=(n, 3)))
    for any_hit in (False, True):
        host = scene.trace_rays(o, d, any_hit=any_hit)
        hits = _torch().zeros((n, 8), dtype=_torch().int32, device="cuda")
        scene.trace_rays(to_device(api.ray_records(o, d)), hits=hits, any_hit=any_hit)
        ctx.sync()
        assert from_device(hits).tobytes() == host.tobytes()
    k = rng.choice(n, min(n, 300), replace=False)
    check_against_oracle(scene, oscene, o[k], d[k], np.zeros(len(k), np.float32), np.full(len(k), np.float32(api.FLT_MAX)))


def test_zero_rays_and_argument_checks():
    desc = P.small_scene(seed=1)
    ctx, scene, _ = hip_and_oracle(desc)
    lib = L.load()
    assert lib.dust_hip_scene_trace_rays(scene._h, None, None, 0, 0) == L.OK
    assert lib.dust_hip_scene_trace_rays_async(scene._h, None, None, 0, 0) == L.OK
    assert lib.dust_hip_scene_trace_rays(scene._h, None, None, 3, 0) == L.ERR_INVALID_ARGUMENT
    rays, hits = api.ray_records(np.zeros((2, 3)), np.ones((2, 3))), np.zeros(2, api.HIT_DTYPE)
    assert lib.dust_hip_scene_trace_rays(scene._h, rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), 2, 2) == L.ERR_INVALID_ARGUMENT
    assert len(scene.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    # uncommitted changes: refused, as a frame is
    scene.set_transform(0, np.asarray(desc.instances[0][1], np.float32))
    with pytest.raises(L.DustError) as e:
        scene.trace_rays(rays["origin"], rays["direction"])
    assert e.value.status == L.ERR_NOT_READY
    scene.commit()
    scene.trace_rays(rays["origin"], rays["direction"])
