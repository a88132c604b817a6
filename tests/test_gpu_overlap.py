"""Scene box queries on the device (dust_hip_scene_overlap_boxes / _async, overlap.hip): every solid voxel of the committed scene inside
caller-supplied world-space boxes. A numpy brute-force witness in this file does the checking: each instance's voxels from its Block
array, each voxel's world box by the header's float32 formula, the header's per-axis rule, ordered by (instance, block, voxel).
Axis-aligned instances are exact; rotated ones are held between the witness of the box shrunk and grown by the tolerance (float64 SAT)."""
import ctypes as C

import numpy as np
import pytest

import parity_util as P
from dust_amd import _lib as L
from dust_amd import api, scenes, synth
from test_gpu_many_instances import scattered_scene

pytestmark = pytest.mark.gpu

F = np.float32


# ------------------------------------------------------------------ the witness
def model_voxels(blocks, mats):
    """every solid voxel of a model in (block, voxel bit) order: (xyz (n, 3) int64, block (n,), voxel (n,), palette (n,))"""
    if len(blocks) == 0:
        z = np.zeros(0, np.int64)
        return np.zeros((0, 3), np.int64), z, z, z
    mask = blocks["mask"].astype(np.uint64)
    bits = ((mask[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    rank = np.cumsum(bits, axis=1) - 1
    bi, v = np.nonzero(bits)
    xyz = np.stack([blocks["x"][bi].astype(np.int64) + (v >> 4), blocks["y"][bi].astype(np.int64) + ((v >> 2) & 3),
                    blocks["z"][bi].astype(np.int64) + (v & 3)], axis=1)
    pal = mats[blocks["material_ptr"][bi].astype(np.int64) + rank[bi, v]]
    return xyz, bi.astype(np.int64), v.astype(np.int64), pal.astype(np.int64)


def world_boxes32(xyz, t):
    """the header's formula: each of the 8 corners w_r = ((m[r][0] px + m[r][1] py) + m[r][2] pz) + m[r][3] in float32, per-axis min / max"""
    m = np.asarray(t, F).reshape(3, 4)
    lo = np.full((len(xyz), 3), np.inf, F)
    hi = np.full((len(xyz), 3), -np.inf, F)
    for c in range(8):
        p = [(xyz[:, k] + ((c >> k) & 1)).astype(F) for k in range(3)]
        for r in range(3):
            w = ((m[r, 0] * p[0] + m[r, 1] * p[1]) + m[r, 2] * p[2]) + m[r, 3]
            lo[:, r] = np.minimum(lo[:, r], w)
            hi[:, r] = np.maximum(hi[:, r], w)
    return lo, hi


class Witness:
    def __init__(self, desc, exact=True):
        self.desc = desc
        self.mv = {}
        self.inst = []
        self.boxes = []
        for i, (mid, t) in enumerate(desc.instances):
            if mid not in self.mv:
                self.mv[mid] = model_voxels(*desc.models[mid])
            xyz, blk, vox, pal = self.mv[mid]
            if exact:
                lo, hi = world_boxes32(xyz, t)
            else:   # (the sandwich only needs each instance's box)
                m = np.asarray(t, np.float64).reshape(3, 4)
                w = np.concatenate([xyz, xyz + 1]) @ m[:, :3].T + m[:, 3] if len(xyz) else np.zeros((0, 3))
                lo = hi = w
            blo = lo.min(0) if len(lo) else np.full(3, np.inf, F)
            bhi = hi.max(0) if len(hi) else np.full(3, -np.inf, F)
            self.inst.append((lo, hi, blo, bhi))
            self.boxes.append(np.concatenate([blo, bhi]))
        self.boxes = np.asarray(self.boxes, np.float64).reshape(-1, 6)

    def exact(self, qlo, qhi):
        """records (instance, block, voxel, x, y, z, palette) of the voxels the header's rule reports, in order"""
        qlo, qhi = np.asarray(qlo, F), np.asarray(qhi, F)
        if not (np.all(np.isfinite(qlo)) and np.all(np.isfinite(qhi)) and np.all(qlo <= qhi)):
            return np.zeros((0, 7), np.int64)
        out = []
        for i, (lo, hi, blo, bhi) in enumerate(self.inst):
            if np.any(bhi < qlo) or np.any(blo > qhi):
                continue
            ok = np.ones(len(lo), bool)
            for r in range(3):
                if qlo[r] < qhi[r]:
                    ok &= (lo[:, r] < qhi[r]) & (qlo[r] < hi[:, r])
                else:
                    ok &= (lo[:, r] <= qlo[r]) & (qlo[r] < hi[:, r])
            if ok.any():
                xyz, blk, vox, pal = self.mv[self.desc.instances[i][0]]
                k = np.nonzero(ok)[0]
                out.append(np.stack([np.full(len(k), i), blk[k], vox[k], xyz[k, 0], xyz[k, 1], xyz[k, 2], pal[k]], axis=1))
        return np.concatenate(out) if out else np.zeros((0, 7), np.int64)

    def sat(self, qlo, qhi, sign):
        """set of (instance, block, voxel) whose world parallelepiped overlaps the box shrunk (sign -1) or grown (+1) by
        tau = 1e-5 (1 + M), M the largest magnitude of the box's and the voxel's corner coordinates (float64, 15 axes)"""
        qlo, qhi = np.asarray(qlo, np.float64), np.asarray(qhi, np.float64)
        ctr, half = (qlo + qhi) / 2.0, (qhi - qlo) / 2.0
        mbox = np.abs(np.concatenate([qlo, qhi])).max()
        found = set()
        near = np.all(self.boxes[:, 3:] >= qlo - 1.0, axis=1) & np.all(self.boxes[:, :3] <= qhi + 1.0, axis=1)
        for i in np.nonzero(near)[0]:
            i = int(i)
            mid, t = self.desc.instances[i]
            xyz, blk, vox, _ = self.mv[mid]
            m = np.asarray(t, np.float64).reshape(3, 4)
            a, tr = m[:, :3], m[:, 3]
            cols = [a[:, k] for k in range(3)]
            axes = [np.eye(3)[r] for r in range(3)] + [np.cross(cols[(k + 1) % 3], cols[(k + 2) % 3]) for k in range(3)] + \
                   [np.cross(np.eye(3)[r], cols[k]) for r in range(3) for k in range(3)]
            ax = np.array(axes)                                                    # (15, 3)
            c = (xyz + 0.5) @ a.T + tr                                             # voxel centres (n, 3)
            ext = 0.5 * np.abs(a).sum(axis=1)                                      # half extent per world axis
            big = np.maximum(mbox, (np.abs(c) + ext).max(axis=1))
            tau = 1e-5 * (1.0 + big)                                               # (n,)
            rp = 0.5 * np.abs(ax @ a).sum(axis=1)                                  # (15,)
            h = half[None, :] + sign * tau[:, None]                                # (n, 3)
            valid = np.all(h >= 0.0, axis=1)
            rq = h @ np.abs(ax).T                                                  # (n, 15)
            dist = np.abs((c - ctr) @ ax.T)
            ok = valid & np.all(dist <= rp[None, :] + rq, axis=1)
            for k in np.nonzero(ok)[0]:
                found.add((i, int(blk[k]), int(vox[k])))
        return found


def as_rows(recs):
    return np.stack([recs["instance"].astype(np.int64), recs["block"].astype(np.int64), recs["voxel"].astype(np.int64),
                     recs["xyz"][:, 0].astype(np.int64), recs["xyz"][:, 1].astype(np.int64), recs["xyz"][:, 2].astype(np.int64),
                     recs["palette"].astype(np.int64)], axis=1) if len(recs) else np.zeros((0, 7), np.int64)


def check_exact(scene, wit, lo, hi, capacity=None):
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    want = [wit.exact(lo[i], hi[i]) for i in range(len(lo))]
    cap = np.array([min(len(w), 3000) for w in want]) if capacity is None else capacity
    counts, per = scene.overlap_boxes(lo, hi, capacity=cap)
    for i in range(len(lo)):
        assert counts[i] == len(want[i]), (i, lo[i], hi[i], counts[i], len(want[i]))
        got = as_rows(per[i])
        assert np.array_equal(got, want[i][: len(got)]), (i, lo[i], hi[i])
    return counts, per, want


def world_bounds(desc):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for mid, t in desc.instances:
        b = desc.models[mid][0]
        m = np.asarray(t, np.float64).reshape(3, 4)
        pts = np.array([[x, y, z] for x in (b["x"].min(), b["x"].max() + 4.0) for y in (b["y"].min(), b["y"].max() + 4.0)
                        for z in (b["z"].min(), b["z"].max() + 4.0)], np.float64) @ m[:, :3].T + m[:, 3]
        lo, hi = np.minimum(lo, pts.min(0)), np.maximum(hi, pts.max(0))
    return lo, hi


def box_mix(rng, lo, hi, n):
    """points, flat boxes, boxes on voxel faces (integer and half-integer bounds), player-sized boxes, 64^3 boxes, boxes that straddle
    the scene: (lo, hi) float32"""
    k = n // 6
    c = lo + rng.random((n, 3)) * (hi - lo)
    size = np.zeros((n, 3))
    size[k:2 * k] = rng.uniform(0.0, 9.0, (k, 3))
    size[np.arange(k, 2 * k), rng.integers(0, 3, k)] = 0.0           # flat
    size[2 * k:3 * k] = rng.integers(1, 9, (k, 3))
    c[2 * k:3 * k] = np.round(c[2 * k:3 * k] * 2.0) / 2.0            # faces on integer and half-integer planes
    size[3 * k:4 * k] = (1.0, 2.0, 1.0)
    c[3 * k:4 * k] = np.round(c[3 * k:4 * k])                         # player-sized, standing on voxel faces
    size[4 * k:5 * k] = 64.0
    size[5 * k:] = rng.uniform(10.0, 300.0, (n - 5 * k, 3))          # straddling instances
    blo = c.astype(F)
    bhi = (c + size).astype(F)
    return blo, bhi


def castle_desc():
    data, _ = synth.castle_scene(scale=0.25)
    return scenes.SceneDesc.from_vox(data)


@pytest.fixture(scope="module")
def castle():
    desc = castle_desc()
    ctx = api.Context(device=0)
    scene = scenes.hip_scene(ctx, desc)
    return ctx, scene, desc, Witness(desc)


def check_records(per, desc):
    """every record names a set voxel of its block, at xyz, with the palette index the material stream holds there"""
    for recs in per:
        for g in recs:
            blocks, mats = desc.models[desc.instances[int(g["instance"])][0]]
            b = blocks[int(g["block"])]
            v, mask = int(g["voxel"]), int(b["mask"])
            assert (mask >> v) & 1, g
            assert [int(b["x"]) + (v >> 4), int(b["y"]) + ((v >> 2) & 3), int(b["z"]) + (v & 3)] == [int(x) for x in g["xyz"]], g
            assert mats[int(b["material_ptr"]) + bin(mask & ((1 << v) - 1)).count("1")] == g["palette"], g


# ------------------------------------------------------------------ 1. the castle stand-in: exact
def test_castle_boxes_match_the_witness_exactly(castle):
    ctx, scene, desc, wit = castle
    for mid, t in desc.instances:   # (90-degree rotations and mirrors only)
        a = np.asarray(t, F).reshape(3, 4)[:, :3]
        assert np.all((a != 0).sum(0) == 1) and np.all((a != 0).sum(1) == 1)
    lo, hi = world_bounds(desc)
    rng = np.random.default_rng(1)
    blo, bhi = box_mix(rng, lo, hi, 2000)
    counts, per, want = check_exact(scene, wit, blo, bhi)
    assert (counts > 0).sum() > 400 and counts.max() > 1000
    check_records(per[::7], desc)


# ------------------------------------------------------------------ 2. rotated instances: the tolerance sandwich
def test_rotated_instances_within_tolerance():
    check_sandwich(scattered_scene(4096, seed=11), 160, seed=2)


def test_scene_without_a_usable_grid_within_tolerance():
    # no grid cell can list 4200 boxes round one point; small boxes (every instance meets the scene's centre)
    check_sandwich(scattered_scene(4200, seed=23, n_models=3, span=(0.0, 0.0, 0.0)), 24, seed=12, big=False)


def check_sandwich(desc, n, seed, big=True):
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    wit = Witness(desc, exact=False)
    lo, hi = world_bounds(desc)
    rng = np.random.default_rng(seed)
    c = lo + rng.random((n, 3)) * (hi - lo)
    size = rng.uniform(0.0, 12.0 if big else 1.5, (n, 3))
    if big:
        size[: n // 4] = rng.uniform(20.0, 90.0, (n // 4, 3))    # (many cells: the group boxes or the ordered scan)
    blo, bhi = c.astype(F), (c + size).astype(F)
    counts, per = scene.overlap_boxes(blo, bhi, capacity=200000)
    assert (counts > 0).sum() > n // 5
    for i in range(n):
        r = per[i]
        assert len(r) == counts[i]
        key = [(int(x["instance"]), int(x["block"]), int(x["voxel"])) for x in r]
        assert key == sorted(set(key)), i
        got = set(key)
        inner, outer = wit.sat(blo[i], bhi[i], -1.0), wit.sat(blo[i], bhi[i], 1.0)
        assert inner <= got, (i, len(inner - got))
        assert got <= outer, (i, len(got - outer))
    check_records(per[::9], desc)


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
    wit = Witness(desc)
    rng = np.random.default_rng(3)
    n = 120
    border = rng.choice([1792.0, 2048.0, 2304.0], (n, 3))
    border[: n // 2] = (96 + rng.integers(0, 64, (n // 2, 3))) * 16.0       # 16-cell borders
    size = rng.uniform(8.0, 64.0, (n, 3))
    c = border - 2048.0 - size * rng.uniform(0.2, 0.8, (n, 3))                # (straddling the border)
    blo, bhi = c.astype(F), (c + size).astype(F)
    counts, per, _ = check_exact(scene, wit, blo, bhi)
    assert (counts > 0).sum() > n // 4


# ------------------------------------------------------------------ 4. capacity
def test_capacity(castle):
    ctx, scene, desc, wit = castle
    lo, hi = world_bounds(desc)
    rng = np.random.default_rng(4)
    blo, bhi = box_mix(rng, lo, hi, 300)
    full, per_full = scene.overlap_boxes(blo, bhi, capacity=0)
    assert all(len(p) == 0 for p in per_full) and full.max() > 100
    cap = rng.integers(0, 40, len(blo))
    counts, per, _ = check_exact(scene, wit, blo, bhi, capacity=cap)
    assert np.array_equal(counts, full)
    # slots past the count are untouched: a sentinel in every slot
    lib = L.load()
    boxes = api.box_queries(blo, bhi, 50)
    recs = np.zeros(len(blo) * 50, api.VOXEL_REF_DTYPE)
    recs.view(np.uint8)[:] = 0xA5
    cnt = np.zeros(len(blo), np.uint32)
    L.check(lib.dust_hip_scene_overlap_boxes(scene._h, boxes.ctypes.data_as(C.c_void_p), len(blo), cnt.ctypes.data_as(C.c_void_p),
                                             recs.ctypes.data_as(C.c_void_p), len(recs), 0))
    assert np.array_equal(cnt, full)
    for i in range(len(blo)):
        tail = recs[i * 50 + min(int(cnt[i]), 50): (i + 1) * 50]
        assert np.all(tail.view(np.uint8) == 0xA5), i
    # a slice past n_records is refused before anything runs
    bad = api.box_queries(blo[:2], bhi[:2], 50)
    assert lib.dust_hip_scene_overlap_boxes(scene._h, bad.ctypes.data_as(C.c_void_p), 2, cnt.ctypes.data_as(C.c_void_p),
                                            recs.ctypes.data_as(C.c_void_p), 99, 0) == L.ERR_INVALID_ARGUMENT
    bad["first"][1] = 0xFFFFFFF0
    assert lib.dust_hip_scene_overlap_boxes(scene._h, bad.ctypes.data_as(C.c_void_p), 2, cnt.ctypes.data_as(C.c_void_p),
                                            recs.ctypes.data_as(C.c_void_p), len(recs), 0) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_scene_overlap_boxes(scene._h, bad.ctypes.data_as(C.c_void_p), 2, cnt.ctypes.data_as(C.c_void_p),
                                            recs.ctypes.data_as(C.c_void_p), len(recs), 4) == L.ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ 5. any hit
def test_any_hit(castle):
    ctx, scene, desc, wit = castle
    lo, hi = world_bounds(desc)
    blo, bhi = box_mix(np.random.default_rng(5), lo, hi, 400)
    full, per_full = scene.overlap_boxes(blo, bhi, capacity=100000)
    counts, per = scene.overlap_boxes(blo, bhi, capacity=1, any_hit=True)
    assert np.array_equal(counts, (full > 0).astype(np.uint32))
    for i in np.nonzero(full)[0]:
        assert len(per[i]) == 1
        assert per[i][0].tobytes() in {r.tobytes() for r in per_full[i]}, i


# ------------------------------------------------------------------ 6. degenerate boxes; points against get_voxels and a ray
def test_degenerate_boxes_and_points(castle):
    ctx, scene, desc, wit = castle
    nan, inf = F(np.nan), F(np.inf)
    lo = np.zeros((7, 3), F)
    hi = np.full((7, 3), 10.0, F)
    lo[0, 0] = nan
    hi[1, 1] = nan
    lo[2, 2] = -inf
    hi[3, 0] = inf
    lo[4, 1] = 11.0                      # lo > hi
    lo[5] = hi[5] = (nan, nan, nan)
    lo[6], hi[6] = (-inf, -inf, -inf), (inf, inf, inf)
    counts, _ = scene.overlap_boxes(lo, hi)
    assert np.all(counts == 0)
    # points at voxel centres: one voxel each (where one instance holds it); it agrees with a ray from the point and with get_voxels
    rng = np.random.default_rng(6)
    inst = rng.integers(0, len(desc.instances), 60)
    pts = []
    for i in inst:
        mid, t = desc.instances[int(i)]
        xyz = wit.mv[mid][0]
        v = xyz[int(rng.integers(0, len(xyz)))] + 0.5
        pts.append(np.asarray(t, np.float64).reshape(3, 4) @ np.append(v, 1.0))
    pts = np.asarray(pts, F)
    counts, per, want = check_exact(scene, wit, pts, pts)
    assert np.all(counts >= 1)
    one = [k for k in range(len(pts)) if counts[k] == 1]
    assert len(one) > 30
    hits = scene.trace_rays(pts[one], np.tile([[0.3, -0.7, 0.2]], (len(one), 1)))
    for j, k in enumerate(one):
        r = per[k][0]
        assert (hits[j]["instance"], hits[j]["block"], hits[j]["voxel"]) == (r["instance"], r["block"], r["voxel"]), k
    for k in one:   # (last: a model's first get_voxels moves it into its editable form)
        r = per[k][0]
        assert scene._models[int(r["instance"])].get_voxels(r["xyz"][None].astype(np.uint32))[0] == r["palette"]
    scene.commit()


# ------------------------------------------------------------------ 7. the edit round trip
def test_edit_round_trip():
    base = P.small_scene(seed=6, n_models=2, n_instances=2)
    desc = scenes.SceneDesc(base.models, base.palette, [(0, base.instances[0][1]), (1, base.instances[1][1])])   # a model per instance
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    wit = Witness(desc)
    lo, hi = world_bounds(desc)
    rng = np.random.default_rng(7)
    for _ in range(200):   # a box with voxels of instance 0 only, and a control box of instance 1 that does not meet it
        c = lo + rng.random(3) * (hi - lo)
        a = wit.exact(c.astype(F), (c + 6.0).astype(F))
        if len(a) > 5 and np.all(a[:, 0] == 0):
            break
    assert len(a) > 5 and np.all(a[:, 0] == 0)
    box = (c.astype(F), (c + 6.0).astype(F))
    for _ in range(400):
        d = lo + rng.random(3) * (hi - lo)
        b = wit.exact(d.astype(F), (d + 5.0).astype(F))
        if len(b) > 3 and np.all(b[:, 0] == 1):
            break
    assert len(b) > 3 and np.all(b[:, 0] == 1)
    ctrl = (d.astype(F), (d + 5.0).astype(F))
    q_lo, q_hi = np.stack([box[0], ctrl[0]]), np.stack([box[1], ctrl[1]])
    counts, per = scene.overlap_boxes(q_lo, q_hi, capacity=1000)
    assert counts[0] == len(a) and counts[1] == len(b)
    scene._models[0].set_voxels(per[0]["xyz"].astype(np.uint32), -np.ones(len(per[0]), np.int32))
    with pytest.raises(L.DustError) as e:
        scene.overlap_boxes(q_lo, q_hi)
    assert e.value.status == L.ERR_NOT_READY
    scene.commit()
    counts2, per2 = scene.overlap_boxes(q_lo, q_hi, capacity=1000)
    assert counts2[0] == 0
    assert counts2[1] == counts[1] and per2[1].tobytes() == per[1].tobytes()
    # place: one voxel back, with a colour of its own
    at = per[0][len(per[0]) // 2]
    scene._models[0].set_voxels(at["xyz"][None].astype(np.uint32), [77])
    scene.commit()
    counts3, per3 = scene.overlap_boxes(q_lo[:1], q_hi[:1], capacity=10)
    assert counts3[0] == 1 and list(per3[0][0]["xyz"]) == list(at["xyz"]) and per3[0][0]["palette"] == 77 and per3[0][0]["instance"] == 0


# ------------------------------------------------------------------ 8. the device path
def _torch():
    import torch
    return torch


def test_async_path_matches_sync(castle):
    torch = _torch()
    ctx, scene, desc, wit = castle
    lo, hi = world_bounds(desc)
    blo, bhi = box_mix(np.random.default_rng(8), lo, hi, 3000)
    boxes = api.box_queries(blo, bhi, 40)
    host_counts, host_per = scene.overlap_boxes(blo, bhi, capacity=40)
    host = np.zeros(len(blo) * 40, api.VOXEL_REF_DTYPE)
    for i, p in enumerate(host_per):
        host[i * 40: i * 40 + len(p)] = p
    dboxes = torch.from_numpy(boxes.view(np.int32).reshape(-1, 8).copy()).to("cuda")
    # enqueued behind a rendered frame
    pipe = api.StandardPipeline(ctx, 64, 48)
    pipe.render(scene, P.camera_for((140.0, 80.0, 100.0)), P.sky_state(), L.PASS_PRIMARY, frame_index=1)
    outs = []
    for _ in range(2):
        counts = torch.zeros(len(blo), dtype=torch.int32, device="cuda")
        recs = torch.zeros((len(blo) * 40, 4), dtype=torch.int32, device="cuda")
        scene.overlap_boxes(dboxes, counts=counts, records=recs)
        outs.append((counts, recs))
    ctx.sync()
    for counts, recs in outs:
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), host_counts)
        assert recs.cpu().numpy().reshape(-1).view(api.VOXEL_REF_DTYPE).tobytes() == host.tobytes()
    lib = L.load()
    assert lib.dust_hip_scene_overlap_boxes_async(scene._h, None, 0, None, None, 0, 0) == L.OK
    assert lib.dust_hip_scene_overlap_boxes(scene._h, None, 0, None, None, 0, 0) == L.OK
    assert lib.dust_hip_scene_overlap_boxes(scene._h, None, 3, None, None, 0, 0) == L.ERR_INVALID_ARGUMENT


def test_empty_scene_counts_zero():
    ctx = api.Context(device=0)
    scene = api.Scene(ctx)
    scene.commit()
    counts, per = scene.overlap_boxes(np.zeros((5, 3)), np.full((5, 3), 100.0))
    assert np.all(counts == 0) and all(len(p) == 0 for p in per)
