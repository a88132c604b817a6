"""The numpy float64 witness of the two passes every frame begins with: the camera-ray pass (k_primary*, primary_shade in
dust_amd/csrc/kernels.hip; orc_pass_primary in oracle/shade.c) and the sun-shadow + ambient-occlusion pass (ao_packet; orc_pass_ao), and
the small scenes its tests run on. A helper module, not a test: tests/test_frame_witness.py holds the C oracle to it on the CPU,
tests/test_gpu_frame_witness.py the kernels. Written from the shader text -- camera.glsl:4-16, primary/hit.rint:43-131, hit.rchit:16-95,
miss.rmiss:7-17, final_gather/ambient_occlusion.rgen:14-66, .rint:46-134, .rchit, .rmiss, nee.rmiss:11-22, normal.glsl:31-43,
nrd.glsl:2-147 --: it binds neither library and shares no code with oracle/ or csrc/. The sky and the sun are radiance_witness's.

There is NO stepping loop here. What a ray hits is found by interval arithmetic over every solid voxel of every instance: one slab test
per brick and one per voxel, all rays of a chunk at once. What the shaders' brick walk adds to plain geometry is restated as five rules
(`trace`), because they are the reference's DEFINITION of a hit, not geometry. For a brick whose slab interval in the ray's object space
is [t0, t1]:
  1  the brick takes part only if t0 < t1 and t1 > 0;
  2  sun and AO rays only (ambient_occlusion.rint:62-73): with t0 <= 8 <= t1 a brick that holds any voxel reports t0 and its voxels
     are never walked;
  3  hd = max(t0, tmin); the start voxel is clamp(floor(o + d hd), 0, 3); if it is solid the brick reports hd -- EVEN WHEN hd > t1: a
     ray that left the brick before tmin still hits whatever voxel the clamp lands on, at t = tmin;
  4  any other solid voxel is reported at its own slab entry te > hd, and only if te + 0.001 < t1 (the start voxel is not asked);
  5  a report is accepted iff tmin <= t <= the best so far, equal t goes to the lower (instance, block); the sun ray stops at any
     accepted report, the AO ray takes the closest below tmax = 8, both with tmin = 0.1; the camera ray runs from near to far.
Traps for a plain "first solid voxel on the ray" caster (it is wrong there, the shaders define the answer): the second half of rule 3
-- a sun ray that starts inside a brick and is out of it by t = 0.1 is still shadowed by the voxel the clamp lands on --, and rule 4's
0.001, which is not asked of the start voxel. A trap met while writing this one: one tolerance for every t. A ray that enters a face at
a grazing angle has a t that moves by many times the error of its origin (an AO distance lay 2.4e-4 from the oracle's on a ray
entering at two degrees), so every t carries its own tolerance here, and the checks state their bounds across the entered face.

Decisions. Every comparison above is evaluated in float64 with its margin; a float32 evaluation of `t d + o` at this scene's coordinates
(below 64: half an ulp is 3.8e-6, three roundings and the rounded inverse matrix make it 1e-5) may fall on the other side of any comparison
closer than that. BAND is ten times it, in world units; along an instance's object axis it is BAND x the norm of that row of the
inverse, and the crossing of a plane moves by that over the direction's component across the plane. A candidate is `robust` when
every comparison that makes it one clears the band, `possible` when none fails by more than the band. A closest-hit ray is DECIDED
when its winner is robust and no other possible candidate lies within the band of it or in front of it; an any-hit ray when a robust
candidate exists or no possible one does. The normal is decided apart: the two largest components of (hit point - voxel centre) must
differ by more than the band. Undecided quantities are counted, capped, never compared.

The AO stage is checked from the depth and normal texels that the stage under test READ (the oracle's, or the device's own): its
witness never runs on this module's primary planes, so nothing compounds."""
import functools
from types import SimpleNamespace

import numpy as np

import radiance_witness as RW
from denoise_witness import ray_dirs, unpack_normal
from image_witness import half_value, lit, pack_radiance

F = np.float32
INF = np.inf
BAND = 1e-4
UNDECIDED_CAP = 0.02
AO_REACH = 8.0                        # AMBIENT_OCCLUSION_THRESHOLD
RAY_TMIN = lit(0.1)
SUN_TMAX = 10000.0
NORMAL_SLACK = 16.0 * 2.0 ** -24 * 1023.0   # a dozen float32 roundings of a value below 1, in ten-bit codes: 1e-3
# Worst deviation of the C oracle from this witness over decided pixels of every case of frame_cases(), both traversal modes, measured by
# tests/test_frame_witness.py::test_recorded_deviations_are_the_measurement; test_oracle_against_witness holds the oracle to the bounds
# (docs/EXPERIMENTS.md, the section on this witness). Each bound is the measurement rounded up, by less than a factor of two. They are float32's
# own: t is a quotient of two values rounded at the size of the coordinates (up to 50 here), the motion vector a difference of two
# points near 40, the sky a chain of exp, pow and acos. The radiance figure is measured on the oracle's float32 sky itself
# (orc_sky_radiance + orc_sun_radiance along the pixel's ray), not on the few texels whose rounding happens to show it. The sun term
# carries 1 - cosf(solar radius), which the witness takes in float32 as the shader does (1.0e-5: its float32 rounding alone is 3e-3
# of it).
# A t is the crossing of a voxel's or brick's face, so an error e of the ray's points across that face moves it by e over the direction's
# component across the face: the two t bounds are stated as that e, in world units (`reach` of trace() is the factor; a ray that grazes
# the face it enters has a large one, and its t is worth that much less).
FRAME_T_DEV_MEASURED, FRAME_T_DEV = 7.10e-6, 1.0e-5                # camera rays: |t - witness| / reach
FRAME_AO_T_DEV_MEASURED, FRAME_AO_T_DEV = 2.46e-6, 4.0e-6          # AO rays: (|t - witness| beyond half an fp16 step) / reach
FRAME_MOTION_DEV_MEASURED, FRAME_MOTION_DEV = 2.09e-6, 3.0e-6      # |motion - witness| beyond half an fp16 step, world units
FRAME_RADIANCE_DEV_MEASURED, FRAME_RADIANCE_DEV = 4.64e-7, 8.0e-7  # |Y, Co, Cg - witness| beyond half an fp16 step, relative to the largest of rgb


# ------------------------------------------------------------------ the scene as voxel lists
def decode_model(blocks, materials, palette):
    """Flattened blocks (brick origin, 64-bit mask, pointer into the material stream) -> the voxels they hold. Bit x << 4 | y << 2 | z
    of the mask is voxel (x, y, z) of the brick (hit.rint:30-32); the stream holds a brick's palette indices in ascending bit order
    (hit.rchit:63-71 counts the set bits below the voxel's)."""
    b = np.asarray(blocks)
    origin = np.stack([b["x"], b["y"], b["z"]], axis=1).astype(np.int64)
    mask = b["mask"].astype(np.uint64)
    bits = ((mask[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    brick, code = np.nonzero(bits)
    rank = np.cumsum(bits, axis=1)[brick, code] - 1
    pal = np.asarray(materials, np.uint8)[b["material_ptr"].astype(np.int64)[brick] + rank]
    xyz = origin[brick] + np.stack([code >> 4, (code >> 2) & 3, code & 3], axis=1)
    index = np.full((len(b), 64), -1, np.int64)
    index[brick, code] = np.arange(len(brick))
    return SimpleNamespace(origin=origin.astype(np.float64), bits=bits, brick=brick, code=code, xyz=xyz.astype(np.float64), pal=pal,
                           index=index, palette=np.asarray(palette, np.uint8).reshape(-1, 4)[:255])


def make_scene(models, palette, instances):
    """models: [(blocks, materials)]; instances: [(model index, obj_to_world 3x4 row-major float32, previous mat4 column-major float32 or
    None: the same transform)]. Inverses are taken here, in float64."""
    ms = [decode_model(b, m, palette) for b, m in models]
    out = []
    for mid, o2w, prev in instances:
        a = np.asarray(o2w, F).reshape(3, 4).astype(np.float64)
        if prev is None:
            p = np.eye(4)
            p[:3] = a
        else:
            p = np.asarray(prev, F).reshape(4, 4).astype(np.float64).T
        inv = np.linalg.inv(a[:, :3])
        out.append(SimpleNamespace(model=ms[mid], m=a[:, :3], t=a[:, 3], inv=inv, prev=p, inv_rows=np.sqrt((inv * inv).sum(axis=1))))
    return SimpleNamespace(models=ms, instances=out)


# ------------------------------------------------------------------ rays against boxes
def _slab(oo, od, lo, hi, bp):
    """oo, od: (n, 1, 3); lo, hi: (m, 3); bp (3,): how far a point may be off along each object axis -> entry and exit parameter (n, m) of each ray in each box; how far each may be off (n, m): a
    point known to bp moves the crossing of a plane by bp over the direction's component across that plane; and `edge` (n, m): the ray
    runs along a face plane of the box (a zero direction component with the origin within bp of that plane)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (lo - oo) / od, (hi - oo) / od
    zero = od == 0.0
    inside = (oo > lo) & (oo < hi)
    t_in = np.where(zero, np.where(inside, -INF, INF), np.minimum(a, b))
    t_out = np.where(zero, np.where(inside, INF, -INF), np.maximum(a, b))
    edge = (zero & (np.minimum(np.abs(oo - lo), np.abs(oo - hi)) <= bp)).any(axis=-1)
    tol = np.broadcast_to(bp / np.maximum(np.abs(od), 1e-300), t_in.shape)
    k_in, k_out = t_in.argmax(axis=-1)[..., None], t_out.argmin(axis=-1)[..., None]
    return (np.take_along_axis(t_in, k_in, -1)[..., 0], np.take_along_axis(t_out, k_out, -1)[..., 0],
            np.take_along_axis(tol, k_in, -1)[..., 0], np.take_along_axis(tol, k_out, -1)[..., 0], edge)


def _instance_candidates(inst, o, d, tmin, tmax, shadow_type, rules, band):
    """Every report the bricks of one instance can make to rays (o, d): -> t (n, c); tol (n, c): how far a float32 evaluation's t may
    lie from it; valid, robust, possible (n, c) bool; exact (n, c): t is tmin itself; block (c,), voxel (n, c): index into the model's voxel
    list or -1; edge (n,). Every comparison is written as `x > 0` with the tolerance of x next to it."""
    m = inst.model
    n, nb = len(o), len(m.origin)
    oo = (o - inst.t) @ inst.inv.T
    od = d @ inst.inv.T
    bp = band * inst.inv_rows
    thr = lit(0.001) if 4 in rules else 0.0
    t0, t1, b0, b1, edge_b = _slab(oo[:, None, :], od[:, None, :], m.origin, m.origin + 4.0, bp)
    yes, never = np.ones((n, nb), bool), np.zeros((n, nb), bool)
    with np.errstate(invalid="ignore"):
        # rule 1
        part = (t1 - t0 > 0.0) & (t1 > 0.0)
        part_r, part_p = (t1 - t0 > b0 + b1) & (t1 > b1), (t1 - t0 > -(b0 + b1)) & (t1 > -b1)
        # rule 2
        if shadow_type and 2 in rules:
            r2 = part & (AO_REACH - t0 >= 0.0) & (t1 - AO_REACH >= 0.0)
            r2_r, r2_p = (AO_REACH - t0 > b0) & (t1 - AO_REACH > b1), (AO_REACH - t0 > -b0) & (t1 - AO_REACH > -b1)
            no2_r, no2_p = (AO_REACH - t0 < -b0) | (t1 - AO_REACH < -b1), (AO_REACH - t0 < b0) | (t1 - AO_REACH < b1)
        else:
            r2, r2_r, r2_p, no2_r, no2_p = never, never, never, yes, yes
        # rule 3
        hd = np.maximum(t0, tmin)
        bh = np.where(t0 > tmin - b0, b0, 0.0)                                # tmin itself is exact
        s_exact = t0 < tmin - b0
        p = oo[:, None, :] + od[:, None, :] * np.where(np.isfinite(hd), hd, 0.0)[..., None] - m.origin
        cell = np.clip(np.floor(p), 0, 3).astype(np.int64)
        scode = (cell[..., 0] << 4) | (cell[..., 1] << 2) | cell[..., 2]
        bidx = np.broadcast_to(np.arange(nb), (n, nb))
        s_solid = m.bits[bidx, scode]
        m_start = np.abs(p[..., None] - np.array([1.0, 2.0, 3.0])).min(axis=-1)         # the clamp leaves only these planes to decide
        loose = (m_start <= bp + bh[..., None] * np.abs(od)[:, None, :]).any(axis=-1)
        if 3 in rules:
            inside, inside_r, inside_p = yes, yes, yes
        else:                                                                  # switched off: a brick the ray has left reports nothing
            inside, inside_r, inside_p = t1 - hd > 0.0, t1 - hd > b1 + bh, t1 - hd > -(b1 + bh)
        # the start voxel's report
        s_valid = part & ~r2 & s_solid & inside & (tmax - hd >= 0.0)
        s_robust = s_valid & part_r & no2_r & ~loose & inside_r & (tmax - hd > bh)
        s_poss = part_p & no2_p & (s_solid | loose) & inside_p & (tmax - hd > -bh)
        # rule 2's report
        q_valid = r2 & (t0 - tmin >= 0.0) & (tmax - t0 >= 0.0)
        q_robust = q_valid & part_r & r2_r & (t0 - tmin > b0) & (tmax - t0 > b0)
        q_poss = part_p & r2_p & (t0 - tmin > -b0) & (tmax - t0 > -b0)
        # rule 4: the other solid voxels
        te, tx, be, bx, edge_v = _slab(oo[:, None, :], od[:, None, :], m.xyz, m.xyz + 1.0, bp)
        bv = m.brick
        gaps = ((te - hd[:, bv], be + bh[:, bv]), (tx - te, be + bx), (t1[:, bv] - te - thr, b1[:, bv] + be), (tmax - te, be))
        v_valid = part[:, bv] & ~r2[:, bv] & ~s_solid[:, bv] & inside[:, bv]
        v_robust = part_r[:, bv] & no2_r[:, bv] & ~loose[:, bv] & inside_r[:, bv]
        v_poss = part_p[:, bv] & no2_p[:, bv] & (~s_solid | loose)[:, bv] & inside_p[:, bv]
        for x, tol in gaps:
            v_valid, v_robust, v_poss = v_valid & (x > 0.0), v_robust & (x > tol), v_poss & (x > -tol)
        v_robust &= v_valid
    svox = m.index[bidx, scode]
    none = np.full((n, nb), -1, np.int64)
    return SimpleNamespace(
        t=np.concatenate([hd, t0, te], axis=1), tol=np.concatenate([bh, b0, be], axis=1), valid=np.concatenate([s_valid, q_valid, v_valid], axis=1),
        robust=np.concatenate([s_robust, q_robust, v_robust], axis=1), possible=np.concatenate([s_poss, q_poss, v_poss], axis=1),
        exact=np.concatenate([s_exact, never, np.zeros(te.shape, bool)], axis=1),
        block=np.concatenate([np.arange(nb), np.arange(nb), bv]), voxel=np.concatenate([svox, none, np.broadcast_to(np.arange(len(bv)), te.shape)], axis=1),
        edge=edge_b.any(axis=1) | edge_v.any(axis=1))


def trace(scene, o, d, tmin, tmax, shadow_type=False, any_hit=False, rules=(2, 3, 4), band=BAND, chunk=512):
    """What rays (o, d) (n, 3) hit between tmin and tmax. shadow_type: the sun and AO rays' intersection routine (rule 2). rules: which of
    rules 2, 3 and 4 are in force (tests switch one off to count the rays it decides). -> namespace(hit, t, inst, block, voxel: index
    into the instance's model's voxel list, -1 for a rule-2 report; undecided; reach: t's tolerance over the band, that is how many
    units of t one world unit of error in the hit point is worth (0 where t is tmin itself)), all (n,). An any-hit ray's t and
    identity mean nothing."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(o)
    res = SimpleNamespace(hit=np.zeros(n, bool), t=np.full(n, INF), inst=np.full(n, -1, np.int64), block=np.full(n, -1, np.int64),
                          voxel=np.full(n, -1, np.int64), undecided=np.zeros(n, bool), reach=np.zeros(n))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        k = e - s
        rows = np.arange(k)
        best_t, best_tol, best_robust, best_exact = np.full(k, INF), np.zeros(k), np.zeros(k, bool), np.zeros(k, bool)
        other_t = np.full(k, INF)                                                             # the nearest other candidate, less its tolerance
        any_robust, any_poss, edge = np.zeros(k, bool), np.zeros(k, bool), np.zeros(k, bool)
        for ii, inst in enumerate(scene.instances):
            c = _instance_candidates(inst, o[s:e], d[s:e], tmin, tmax, shadow_type, rules, band)
            edge |= c.edge
            any_robust |= c.robust.any(axis=1)
            any_poss |= c.possible.any(axis=1)
            tv = np.where(c.valid, c.t, INF)
            w_t = tv.min(axis=1)
            win = np.where(tv == w_t[:, None], c.block[None, :], 1 << 30).argmin(axis=1)     # equal t: the lower block
            w_robust, w_exact, w_tol = c.robust[rows, win] & (w_t < INF), c.exact[rows, win], c.tol[rows, win]
            tp = np.where(c.possible | c.valid, c.t - c.tol, INF)
            tp[rows, win] = np.where(w_t < INF, INF, tp[rows, win])
            tp = np.where((w_robust & w_exact)[:, None] & c.exact & c.robust & (c.t == w_t[:, None]), INF, tp)   # exact ties are rule 5's, not the band's
            o_t = tp.min(axis=1)
            take = w_t < best_t                                                               # equal t: the lower instance
            loser_t = np.where(take, best_t - best_tol, w_t - w_tol)
            tie = (w_t == best_t) & w_robust & w_exact & best_robust & best_exact
            other_t = np.minimum(other_t, np.minimum(o_t, np.where(tie, INF, loser_t)))
            res.inst[s:e] = np.where(take, ii, res.inst[s:e])
            res.block[s:e] = np.where(take, c.block[win], res.block[s:e])
            res.voxel[s:e] = np.where(take, c.voxel[rows, win], res.voxel[s:e])
            best_robust, best_exact = np.where(take, w_robust, best_robust), np.where(take, w_exact, best_exact)
            best_tol = np.where(take, w_tol, best_tol)
            best_t = np.where(take, w_t, best_t)
        res.hit[s:e] = best_t < INF
        res.t[s:e] = best_t
        res.reach[s:e] = np.where(best_t < INF, best_tol / band, 0.0)
        if any_hit:
            res.undecided[s:e] = edge | ~(any_robust | ~any_poss)
        else:
            res.undecided[s:e] = edge | (res.hit[s:e] & ~best_robust) | ((other_t < INF) & (other_t <= best_t + best_tol))
    return res


def differs(a, b, d, band=BAND, identity=True):
    """rays whose outcome differs between two traces of the same rays (hit or miss; t by more than the band; the voxel reported)"""
    bt = band / np.sqrt((np.asarray(d, np.float64) ** 2).sum(axis=-1))
    both = a.hit & b.hit
    out = a.hit != b.hit
    with np.errstate(invalid="ignore"):
        out |= both & (np.abs(a.t - b.t) > bt)
    if identity:
        out |= both & ((a.inst != b.inst) | (a.block != b.block) | (a.voxel != b.voxel))
    return out


# ------------------------------------------------------------------ the camera-ray pass
def camera_of(cam):
    return SimpleNamespace(c0=np.array(list(cam.view_col0), np.float64), c1=np.array(list(cam.view_col1), np.float64),
                           c2=np.array(list(cam.view_col2), np.float64), pos=np.array(list(cam.position), np.float64),
                           tan=float(F(cam.tan_half_fov)), near=float(F(cam.near_)), far=float(F(cam.far_)))


def pixel_rays(cam, w, h):
    """camera.glsl:4-16 for every pixel, row-major: pixel centre + 0.5, the aspect the float32 quotient w / h, cy negated,
    d = col0 cx + col1 cy - col2, not normalised. -> (camera, d (w h, 3))"""
    c = camera_of(cam)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return c, ray_dirs(c, w, h, xx, yy).reshape(-1, 3)


def unorm10(v):
    return np.rint(np.clip(v, 0.0, 1.0) * 1023.0).astype(np.uint32)


def octahedral(nw):
    """nrd.glsl:2-10, unsigned: -> (..., 2) in [0, 1], and `seam`: z < 0 with x or y within 1e-6 of a sign change that is not an exact 0"""
    v = nw / np.abs(nw).sum(axis=-1, keepdims=True)
    sx, sy = np.where(v[..., 0] >= 0.0, 1.0, -1.0), np.where(v[..., 1] >= 0.0, 1.0, -1.0)
    wx, wy = (1.0 - np.abs(v[..., 1])) * sx, (1.0 - np.abs(v[..., 0])) * sy
    neg = v[..., 2] < 0.0
    ex, ey = np.where(neg, wx, v[..., 0]), np.where(neg, wy, v[..., 1])
    tiny = lambda a: (a != 0.0) & (np.abs(a) < 1e-6)
    seam = (neg & (tiny(v[..., 0]) | tiny(v[..., 1]))) | tiny(v[..., 2])
    return np.stack([ex * 0.5 + 0.5, ey * 0.5 + 0.5], axis=-1), seam


def primary(scene, cam, sky, w, h, rules=(2, 3, 4), band=BAND):
    """The planes primary/hit.rchit and miss.rmiss write, per pixel in row-major order -> namespace:
    hit, undecided (n,) bool; t; voxel_id, albedo (uint32); normal_xy (n, 2): the two ten-bit codes BEFORE rounding, normal_high: the
    texel's upper twelve bits (roughness code 1023, material code), normal_undecided; face: 2 x axis + (1 for the + side), object space;
    motion (n, 3); miss_rgb (n, 3): (sky + sun) / 3.14; denoised (n, 4) uint16: the miss texel; trace: the trace's own namespace."""
    c, d = pixel_rays(cam, w, h)
    n = len(d)
    o = np.broadcast_to(c.pos, (n, 3))
    tr = trace(scene, o, d, c.near, c.far, rules=rules, band=band)
    hit = tr.hit
    out = SimpleNamespace(hit=hit, undecided=tr.undecided, t=tr.t, reach=tr.reach, trace=tr, d=d, voxel_id=np.zeros(n, np.uint32), albedo=np.full(n, 0xFFFFFFFF, np.uint32),
                          normal_xy=np.zeros((n, 2)), normal_high=np.zeros(n, np.uint32), normal_undecided=np.zeros(n, bool),
                          face=np.full(n, -1, np.int64), motion=np.zeros((n, 3)))
    t = np.where(hit, tr.t, 0.0)
    world = t[:, None] * d + c.pos
    for ii, inst in enumerate(scene.instances):
        sel = np.nonzero(hit & (tr.inst == ii))[0]
        if not len(sel):
            continue
        m = inst.model
        vox = tr.voxel[sel]
        local = (world[sel] - inst.t) @ inst.inv.T                       # hit point in object space
        q = local - (m.xyz[vox] + 0.5)                                   # hit.rchit:26-29
        aq = np.abs(q)
        axis = aq.argmax(axis=1)
        rest = np.where(np.arange(3)[None, :] == axis[:, None], -INF, aq + band * inst.inv_rows)
        out.normal_undecided[sel] = aq.max(axis=1) - band * inst.inv_rows[axis] <= rest.max(axis=1)
        sign = np.sign(q[np.arange(len(sel)), axis])
        n_obj = np.zeros((len(sel), 3))
        n_obj[np.arange(len(sel)), axis] = sign
        out.face[sel] = 2 * axis + (sign > 0)
        n_world = n_obj @ inst.m.T                                       # gl_ObjectToWorldEXT * vec4(n, 0): the matrix itself
        xy, seam = octahedral(n_world)
        out.normal_undecided[sel] |= seam
        out.normal_xy[sel] = xy * 1023.0
        pal = m.pal[vox].astype(np.uint32)
        out.normal_high[sel] = np.uint32(1023 << 20) | (np.minimum(pal, 3) << 30)        # clamp(pal / 3, 0, 1) in two bits
        col = m.palette[pal].astype(np.float64) / 255.0
        out.albedo[sel] = unorm10(col[:, 0]) | (unorm10(col[:, 1]) << 10) | (unorm10(col[:, 2]) << 20) | np.uint32(3 << 30)
        out.voxel_id[sel] = (m.code[vox].astype(np.uint32) << 24) | (pal << 16) | np.uint32(ii & 0xFFFF)
        h4 = np.concatenate([local, np.ones((len(sel), 1))], axis=1) @ inst.prev.T
        out.motion[sel] = h4[:, :3] / h4[:, 3:4] - world[sel]
    dirs = RW.normalize32(d)
    with np.errstate(invalid="ignore"):
        out.miss_rgb = (RW.sky_radiance(sky, dirs) + RW.sun_radiance(sky, dirs)[0]) / lit(3.14)
    out.denoised = pack_radiance(out.miss_rgb, np.full(n, 100000.0))    # the hit distance overflows to the fp16 infinity
    return out


def half_step(v):
    """half the distance between the fp16 values around v"""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 11.0)


def _excess(got_halves, want, scale=None):
    """how far fp16 texels lie from float64 values beyond half an fp16 step of those, relative to `scale` when given; 0 inside"""
    err = np.abs(half_value(got_halves) - want) - half_step(want)
    if scale is not None:
        err = err / np.maximum(scale, 1e-30)[..., None]
    return np.maximum(err, 0.0)


def _fail(what, text, mask, w):
    at = np.nonzero(mask)[0][:4]
    raise AssertionError(f"{what}: {text} at pixels (x, y) {[(int(i % w), int(i // w)) for i in at]} ({int(mask.sum())} in all)")


def check_primary(planes, wit, w, what="", bounds=None):
    """planes: dict of depth, voxel_id, albedo, normal, motion, denoised as read from a G-buffer, (h, w[, 4]). Holds them to the witness
    on decided pixels; -> the worst figures met. bounds: (t, motion, radiance) deviations allowed, by default the recorded ones."""
    b_t, b_m, b_r = bounds or (FRAME_T_DEV, FRAME_MOTION_DEV, FRAME_RADIANCE_DEV)
    n = len(wit.hit)
    depth = np.asarray(planes["depth"], F).reshape(n)
    dec, hit = ~wit.undecided, wit.hit
    got_hit = depth != F(INF)
    if (dec & (got_hit != hit)).any():
        _fail(what, "hit or miss differs", dec & (got_hit != hit), w)
    dh, dm = dec & hit, dec & ~hit
    for name, want, where in (("voxel_id", wit.voxel_id, dh), ("albedo", wit.albedo, dec)):   # (a miss leaves the id plane alone)
        got = np.asarray(planes[name], np.uint32).reshape(n)
        if (where & (got != want)).any():
            bad = where & (got != want)
            i = np.nonzero(bad)[0][0]
            _fail(what, f"{name} (got {int(got[i]):#010x}, witness {int(want[i]):#010x})", bad, w)
    nrm = np.asarray(planes["normal"], np.uint32).reshape(n)
    if (dh & ((nrm >> 20) != (wit.normal_high >> 20))).any():
        _fail(what, "roughness or material code of the normal texel", dh & ((nrm >> 20) != (wit.normal_high >> 20)), w)
    codes = np.stack([nrm & 1023, (nrm >> 10) & 1023], axis=1).astype(np.float64)
    off = np.where((dh & ~wit.normal_undecided)[:, None], np.abs(codes - wit.normal_xy), 0.0).max(axis=1)
    if (off > 0.5 + NORMAL_SLACK).any():
        _fail(what, f"normal code off by {off.max():.4f}", off > 0.5 + NORMAL_SLACK, w)
    t_err = np.where(dh, np.abs(depth.astype(np.float64) - np.where(dh, wit.t, 0.0)), 0.0)
    if (dh & (wit.reach == 0.0) & (t_err != 0.0)).any():
        _fail(what, "a hit at `near` itself is not at `near`", dh & (wit.reach == 0.0) & (t_err != 0.0), w)
    t_dev = np.where(dh & (wit.reach > 0.0), t_err / np.where(wit.reach > 0.0, wit.reach, 1.0), 0.0)
    if (t_dev > b_t).any():
        _fail(what, f"depth: the hit point off by {t_dev.max():.3e} across the face it entered (bound {b_t:.3e})", t_dev > b_t, w)
    mot = np.asarray(planes["motion"], np.uint16).reshape(n, 4)
    if (dec & (mot[:, 3] != 0)).any() or (dm[:, None] & (mot != 0)).any():
        _fail(what, "motion: fourth half or a miss pixel not 0", dec & (mot != 0).any(axis=1) & (~hit | (mot[:, 3] != 0)), w)
    m_dev = np.where(dh[:, None], _excess(mot[:, :3], wit.motion), 0.0).max(axis=1)
    if (m_dev > b_m).any():
        _fail(what, f"motion off by {m_dev.max():.3e} beyond half a step (bound {b_m:.3e})", m_dev > b_m, w)
    if (dm & (depth.view(np.uint32) != 0x7F800000)).any():
        _fail(what, "a miss pixel's depth is not +inf", dm & (depth.view(np.uint32) != 0x7F800000), w)
    den = np.asarray(planes["denoised"], np.uint16).reshape(n, 4)
    if (dm & (den[:, 3] != 0x7C00)).any():
        _fail(what, "a miss pixel's hit distance is not the fp16 infinity", dm & (den[:, 3] != 0x7C00), w)
    fin = dm & np.isfinite(wit.miss_rgb).all(axis=1) & (half_value(wit.denoised[:, :3]) < 65504.0).all(axis=1)
    ycc = _ycocg(wit.miss_rgb)
    r_dev = np.where(fin[:, None], _excess(den[:, :3], np.where(fin[:, None], ycc, 0.0), np.abs(np.where(fin[:, None], wit.miss_rgb, 1.0)).max(axis=1)), 0.0).max(axis=1)
    if (r_dev > b_r).any():
        _fail(what, f"sky radiance off by {r_dev.max():.3e} beyond half a step (bound {b_r:.3e})", r_dev > b_r, w)
    return dict(t=float(t_dev.max()), motion=float(m_dev.max()), radiance=float(r_dev.max()), normal=float(off.max()),
                motion_half_steps=float(np.where(dh[:, None], np.abs(half_value(mot[:, :3]) - wit.motion) / half_step(wit.motion), 0.0).max()))


def _ycocg(rgb):
    return np.stack([rgb[..., 0] * 0.25 + rgb[..., 1] * 0.5 + rgb[..., 2] * 0.25, rgb[..., 0] * 0.5 - rgb[..., 2] * 0.5,
                     rgb[..., 0] * -0.25 + rgb[..., 1] * 0.5 + rgb[..., 2] * -0.25], axis=-1)


# ------------------------------------------------------------------ the sun-shadow and ambient-occlusion pass
def rotate_by_normal(nrm, v):
    """normal.glsl:31-37 -> (rotated, near: n.z within 1e-6 of the -0.99999 branch)"""
    quat = np.stack([-nrm[:, 1], nrm[:, 0], np.zeros(len(nrm)), 1.0 + nrm[:, 2]], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        quat = quat / np.sqrt((quat * quat).sum(axis=1, keepdims=True))
    flip = nrm[:, 2] < -lit(0.99999)
    quat = np.where(flip[:, None], np.array([-1.0, 0.0, 0.0, 0.0]), quat)
    q, qw = quat[:, :3], quat[:, 3:4]
    out = 2.0 * (q * v).sum(axis=1, keepdims=True) * q + (qw * qw - (q * q).sum(axis=1, keepdims=True)) * v + 2.0 * qw * np.cross(q, v)
    return out, np.abs(nrm[:, 2] + lit(0.99999)) <= 1e-6


def sun_term(sky):
    """nee.rmiss:18-19 for the one direction every sun ray has: sun_radiance(normalize(sun)) (1 - cos(solar radius)), the factor in
    float32 as the shader takes it; and that direction (float64)"""
    s = np.asarray(sky, F)
    sd = s[48:51].astype(np.float64)
    sd = sd / np.sqrt((sd * sd).sum())
    k = F(1.0) - F(np.cos(np.float64(s[55])))
    return RW.sun_radiance(sky, RW.normalize32(sd[None]))[0][0] * float(k), sd


def ambient_occlusion(scene, cam, sky, w, h, depth, normal, noise_slice, rand, rules=(2, 3, 4), band=BAND):
    """ambient_occlusion.rgen:14-66 on the depth and normal planes GIVEN (what the stage under test read), per pixel in row-major order ->
    namespace: hit (depth is not +inf); lit: dot(sun, n) > 0; sun_undecided, ao_undecided; shadowed; ao_hit, ao_t; rgb (n, 3): what the
    sun adds; sun, ao: the traces' own namespaces (rows: the hit pixels, in order)"""
    c, d = pixel_rays(cam, w, h)
    n = len(d)
    depth = np.asarray(depth, F).reshape(n)
    hit = depth != F(INF)
    sel = np.nonzero(hit)[0]
    nrm = unpack_normal(np.asarray(normal, np.uint32).reshape(n)[sel])
    loc = (depth[sel].astype(np.float64)[:, None] * d[sel] + c.pos) + nrm * lit(0.01)
    py, px = sel // w, sel % w
    tex = np.asarray(noise_slice, np.uint8).reshape(128, 128, 4)[(py + 183 + int(rand)) % 128, (px + 7 + int(rand)) % 128, :3]
    ns, near_flip = rotate_by_normal(nrm, tex.astype(np.float64) / 255.0 * 2.0 - 1.0)
    ad = ns / np.sqrt((ns * ns).sum(axis=1, keepdims=True))
    sun = np.asarray(sky, F)[48:51].astype(np.float64)
    gate = nrm @ sun
    term, sd = sun_term(sky)
    out = SimpleNamespace(hit=hit, lit=np.zeros(n, bool), sun_undecided=np.zeros(n, bool), ao_undecided=np.zeros(n, bool),
                          shadowed=np.zeros(n, bool), ao_hit=np.zeros(n, bool), ao_t=np.zeros(n), ao_reach=np.zeros(n), rgb=np.zeros((n, 3)), rows=sel, loc=loc, ao_dir=ad, sun_dir=sd)
    out.lit[sel] = gate > 0.0
    st = trace(scene, loc, np.broadcast_to(sd, loc.shape), RAY_TMIN, SUN_TMAX, shadow_type=True, any_hit=True, rules=rules, band=band)
    at = trace(scene, loc, ad, RAY_TMIN, AO_REACH, shadow_type=True, rules=rules, band=band)
    out.sun, out.ao = st, at
    out.sun_undecided[sel] = (np.abs(gate) <= 1e-6) | ((gate > 0.0) & st.undecided)
    out.shadowed[sel] = (gate > 0.0) & st.hit
    out.ao_undecided[sel] = at.undecided | near_flip
    out.ao_hit[sel] = at.hit
    out.ao_t[sel] = np.where(at.hit, at.t, 0.0)
    out.ao_reach[sel] = at.reach
    out.rgb[sel] = np.where(((gate > 0.0) & ~st.hit)[:, None], term[None, :] * (nrm @ sd)[:, None], 0.0)
    return out


def check_ao(illuminance, wit, w, what="", bounds=None):
    """illuminance: (h, w, 4) fp16 bit patterns after the pass. -> the worst figures met."""
    b_t, b_r = bounds or (FRAME_AO_T_DEV, FRAME_RADIANCE_DEV)
    n = len(wit.hit)
    ill = np.asarray(illuminance, np.uint16).reshape(n, 4)
    ao = wit.hit & ~wit.ao_undecided
    got_t = half_value(ill[:, 3])
    if (ao & ((got_t != 0.0) != wit.ao_hit)).any():
        _fail(what, "AO ray: hit or miss differs", ao & ((got_t != 0.0) != wit.ao_hit), w)
    t_err = np.where(ao & wit.ao_hit, _excess(ill[:, 3], np.where(wit.ao_hit, wit.ao_t, 1.0)), 0.0)
    if ((wit.ao_reach == 0.0) & (t_err != 0.0)).any():
        _fail(what, "an AO hit at tmin itself is not at tmin", (wit.ao_reach == 0.0) & (t_err != 0.0), w)
    t_dev = np.where(wit.ao_reach > 0.0, t_err / np.where(wit.ao_reach > 0.0, wit.ao_reach, 1.0), 0.0)
    if (t_dev > b_t).any():
        _fail(what, f"AO distance: the hit point off by {t_dev.max():.3e} across the face it entered, beyond half a step (bound {b_t:.3e})", t_dev > b_t, w)
    sun = wit.hit & ~wit.sun_undecided
    dark = sun & (~wit.lit | wit.shadowed)
    got = half_value(ill[:, :3])
    if (dark[:, None] & (got != 0.0)).any():
        _fail(what, "an unlit or shadowed pixel carries sunlight", dark & (got != 0.0).any(axis=1), w)
    bright = sun & wit.lit & ~wit.shadowed
    if (bright & ~(got[:, 0] > 0.0)).any():
        _fail(what, "a lit pixel carries no sunlight", bright & ~(got[:, 0] > 0.0), w)
    r_dev = np.where(bright[:, None], _excess(ill[:, :3], _ycocg(wit.rgb), np.abs(np.where(bright[:, None], wit.rgb, 1.0)).max(axis=1)), 0.0).max(axis=1)
    if (r_dev > b_r).any():
        _fail(what, f"sun radiance off by {r_dev.max():.3e} beyond half a step (bound {b_r:.3e})", r_dev > b_r, w)
    return dict(ao_t=float(t_dev.max()), radiance=float(r_dev.max()))


def input_conditions(pw, aw):
    """the counts a case must reach for its checks to mean something (asserted by the CPU test): -> dict"""
    dec = ~pw.undecided
    n_hit = int(pw.hit.sum())
    ao, sun = aw.hit & ~aw.ao_undecided, aw.hit & ~aw.sun_undecided
    n_lit = int((aw.hit & aw.lit).sum())
    return dict(hit=int((dec & pw.hit).sum()), miss=int((dec & ~pw.hit).sum()), camera_undecided=float(pw.undecided.mean()),
                ao_hit=int((ao & aw.ao_hit).sum()), ao_miss=int((ao & ~aw.ao_hit).sum()), ao_undecided=float((aw.hit & aw.ao_undecided).sum() / max(1, aw.hit.sum())),
                lit_open=int((sun & aw.lit & ~aw.shadowed).sum()), lit_shadowed=int((sun & aw.lit & aw.shadowed).sum()), unlit=int((sun & ~aw.lit).sum()),
                sun_undecided=float((aw.hit & aw.lit & aw.sun_undecided).sum() / max(1, n_lit)), hit_share=n_hit / len(pw.hit),
                normal_undecided=float((dec & pw.hit & pw.normal_undecided).sum() / max(1, n_hit)))


MINIMA = dict(hit=200, miss=200, ao_hit=100, ao_miss=100, lit_open=100, lit_shadowed=100, unlit=20)


# ------------------------------------------------------------------ inputs: small scenes
SIZES = ((64, 40), (61, 37))          # the second: no multiple of the 8 x 8 packet, and w / h is no dyadic rational
NOISE_LAYERS = 4
TARGET = (0.0, 5.0, 0.0)
# name -> (eye, frame size, sky, frame index, rand)
CASES = {
    "A": ((21.0, 17.0, 19.0), SIZES[0], "default", 1, 777),
    "B": ((24.0, 8.0, -6.0), SIZES[1], "low_sun", 2, 0x9E3779B9),
    "C": ((8.0, 27.0, -23.0), SIZES[0], "low_sun", 3, 31),
    "D": ((21.0, 17.0, 19.0), SIZES[1], "low_sun", 6, 4000000000),
    "E": (None, SIZES[1], "default", 5, 12345),     # the eye inside the scene's box, inside a brick: rule 3 acts on `near`
    "F": ((5.0, 13.0, 14.0), SIZES[0], "default", 4, 2024),   # the hand-built scene of rules 3 and 4 (stack_inputs)
}
WAFER_SCALE, WAFER_GAP = 0.00028, 0.05
RUN_CASE, RUN_MEMBERS = "A", ((1, 777), (2, 99), (7, 0xFFFFFF85))   # (frame index, rand) of three frames of one view


def frame_cases():
    return sorted(CASES)


def _model_voxels(rng, size, balls):
    """sparse noise plus a few balls -> xyzi (file axes, colour index 0-based)"""
    solid = rng.random(size) < 0.06
    x, y, z = np.ogrid[:size[0], :size[1], :size[2]]
    for _ in range(balls):
        c = [rng.uniform(2.5, s - 2.5) for s in size]
        r = rng.uniform(2.4, 3.4)
        solid |= (x + 0.5 - c[0]) ** 2 + (y + 0.5 - c[1]) ** 2 + (z + 0.5 - c[2]) ** 2 <= r * r
    x, y, z = np.nonzero(solid)
    return np.stack([x, y, z, rng.integers(0, 255, x.size)], axis=1).astype(np.uint8)


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


def _mat4_cols(m3, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = m3, t
    return m.T.reshape(16).astype(F)


@functools.lru_cache(maxsize=None)
def scene_inputs():
    """-> (models [(blocks, materials)], palette, instances [(model, obj_to_world[12], previous mat4[16] or None)]): two models of at most
    16 x 12 x 16 with 300 to 600 voxels; three instances: identity with an integer offset; an axis-permuting rotation with a half-integer
    offset, which stood elsewhere a frame ago; the scale (1.5, 0.75, 1) times an oblique rotation, which stood turned and elsewhere. The
    scale acts on the rotated model, so the object axes are not orthogonal in the world: the matrix and its inverse transpose send a
    face normal to different directions (with the scale applied first they would agree on every axis-aligned normal)."""
    from dust_amd import api, synth      # late: the witness functions need nothing of the package
    rng = np.random.default_rng(20240607)
    pal = synth.make_palette(11)
    models = []
    for size, balls in (((16, 16, 12), 3), ((14, 16, 11), 2)):
        xyzi = _model_voxels(rng, size, balls)
        assert 300 <= len(xyzi) <= 600, len(xyzi)
        models.append(api.flatten_model(xyzi, size, pal))
    perm = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    obl = np.diag([1.5, 0.75, 1.0]) @ _rotation((1.0, 2.0, 3.0), 0.7)    # scaled along WORLD axes: the voxels stand sheared
    placed = [(0, np.eye(3), (-9.0, 0.0, -7.0)), (1, perm, (2.5, 1.5, 9.5)), (0, obl, (-3.25, 8.5, -15.0))]
    inst = []
    for k, (mid, m3, t) in enumerate(placed):
        m = np.zeros((3, 4), F)
        m[:, :3], m[:, 3] = m3, t
        cur3, cur_t = m[:, :3].astype(np.float64), m[:, 3].astype(np.float64)
        prev = None
        if k == 1:
            prev = _mat4_cols(cur3, cur_t + np.array([0.75, -0.5, 0.25]))
        elif k == 2:
            turn = _rotation((0.0, 1.0, 0.2), 0.03)
            prev = _mat4_cols(turn @ cur3, turn @ cur_t + np.array([-0.4, 0.3, 0.6]))
        inst.append((mid, m.reshape(12), prev))
    return models, pal, inst


def _flatten(solid, colour, pal):
    """solid, colour: (x, y, z) arrays in the engine's axes (y up) -> (blocks, materials); the loader takes MagicaVoxel's axes (z up) and maps
    file (x, y, z) to (x, z, size.y - 1 - y) (loader.rs:247-253)"""
    from dust_amd import api
    sx, sy, sz = solid.shape
    x, y, z = np.nonzero(solid)
    xyzi = np.stack([x, sz - 1 - z, y, colour[x, y, z]], axis=1).astype(np.uint8)
    return api.flatten_model(xyzi, (sx, sz, sy), pal)


@functools.lru_cache(maxsize=None)
def stack_inputs():
    """The hand-built scene in which rules 3 and 4 decide many rays, under the default sun, whose x component is 0 in both object spaces.
    A plate (a slab two voxels thick with eight pillars on it, identity, integer offset) and, WAFER_GAP above the slab, a wafer: one layer
    of bricks holding voxels in their top and bottom layers only, squeezed to WAFER_SCALE along y, so that a ray crosses a voxel
    layer in 0.0004 of t and the whole wafer in 0.0016.
      rule 4: a camera ray that comes down a column whose top voxel is missing reaches the bottom voxel 0.0004 before it leaves the
        brick, which is inside the 0.001: not reported, the plate shows through.
      rule 3: a sun or AO ray that starts on the slab has crossed the wafer by t = 0.054 < tmin. Every voxel entry lies before tmin; the
        brick it crossed still reports t = 0.1 where the clamp lands on a solid voxel of its top layer."""
    from dust_amd import synth
    rng = np.random.default_rng(424242)
    pal = synth.make_palette(12)
    plate = np.zeros((16, 8, 16), bool)
    plate[:, :2, :] = True
    for x, z in ((2, 3), (5, 10), (9, 6), (12, 12), (13, 2), (7, 1), (3, 8), (10, 9)):
        plate[x, 2:7, z] = True
    wafer = np.zeros((16, 4, 16), bool)
    wafer[:, 3, :] = rng.random((16, 16)) < 0.5
    wafer[:, 0, :] = rng.random((16, 16)) < 0.6
    models = [_flatten(m, rng.integers(0, 255, m.shape), pal) for m in (plate, wafer)]
    inst = []
    for mid, scale, t in ((0, 1.0, (-8.0, 0.0, -8.0)), (1, WAFER_SCALE, (-8.0, 2.0 + WAFER_GAP, -8.0))):
        m = np.zeros((3, 4), F)
        m[:, :3], m[:, 3] = np.diag([1.0, scale, 1.0]), t
        inst.append((mid, m.reshape(12), None))
    return models, pal, inst


def scene_of(name):
    """the inputs of a case's scene, as scene_inputs() gives them"""
    return stack_inputs() if name == "F" else scene_inputs()


@functools.lru_cache(maxsize=None)
def witness_scene(name="A"):
    models, pal, inst = scene_of(name)
    return make_scene(models, pal, inst)


def _eye_inside(scene):
    """a point inside a brick of instance 0, in an empty voxel whose 26 neighbours are empty too, nearest the box's +x, +z corner"""
    m, inst = scene.models[0], scene.instances[0]
    size = m.xyz.max(axis=0).astype(int) + 1
    grid = np.zeros(tuple(size) + (), bool)
    grid[tuple(m.xyz.astype(int).T)] = True
    pad = np.pad(grid, 1)
    crowd = sum(pad[1 + dx: 1 + dx + size[0], 1 + dy: 1 + dy + size[1], 1 + dz: 1 + dz + size[2]] for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
    bricks = {tuple(b) for b in (m.origin // 4).astype(int)}
    free = [v for v in np.argwhere(crowd == 0) if tuple(v // 4) in bricks and 2 <= v[1] <= size[1] - 3]
    v = max(free, key=lambda v: (v[0] + v[2], v[1]))
    return tuple(float(x) for x in (inst.m @ (v + np.array([0.37, 0.61, 0.43])) + inst.t))


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> dict(cam, sky, w, h, frame_index, rand, noise5: (layers, 128, 128, 4) uint8). Everything from fixed seeds."""
    import json
    import os
    from dust_amd import scenes, synth
    eye, (w, h), sky_name, frame_index, rand = CASES[name]
    target = (0.0, 2.0, 0.0) if name == "F" else TARGET
    if eye is None:
        eye = _eye_inside(witness_scene(name))
        target = (-30.0, 8.0, -10.0)
    if sky_name == "default":
        sky = scenes.sky_state()
    else:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sky_states.json")) as f:
            sky = np.asarray(json.load(f)[sky_name]["state"], F)
    noise5 = synth.stbn_unitvec3_cosine(layers=NOISE_LAYERS)
    noise5.setflags(write=False)
    return dict(cam=scenes.camera_for(eye, target=target), sky=sky, w=w, h=h, frame_index=frame_index, rand=rand, noise5=noise5)


@functools.lru_cache(maxsize=None)
def primary_witness(name, rules=(2, 3, 4)):
    c = case_inputs(name)
    return primary(witness_scene(name), c["cam"], c["sky"], c["w"], c["h"], rules=rules)
