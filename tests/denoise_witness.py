"""The numpy float64 witness of the denoiser (k_denoise_temporal, k_denoise_spatial in dust_amd/csrc/denoise.hip; oracle/denoise.c) and the
synthetic planes its tests run on. A helper module, not a test: tests/test_denoise_witness.py holds the C oracle to it on the CPU,
tests/test_gpu_denoise_planes.py the kernels. Written from the filter's description (the header of denoise.hip):
it binds neither library and shares no code with oracle/ or csrc/; the disc and its rotations are computed from their formulas.

The filter, as described.
  temporal: a hit pixel's surface point (camera position + depth x the un-normalised camera.glsl ray, local z = -1) plus its motion is
    where the point was a frame ago. Seen from the previous camera it lands at a real-valued pixel position, snapped to the pixel centre
    when within 1/512 of it. The four pixels around that position are its taps, with bilinear weights; a tap counts when it lies in the
    frame, held a surface, of the same instance (low 16 bits of the id), whose normal agrees (dot >= 0.9) and whose surface point lies
    on this pixel's plane within disocclusion x distance. With more than 1e-3 of weight alive the history is the weighted mean of the
    live taps' accumulation (rgb and frame count). Antilag: the history's luminance is clamped to mean +- sigma_scale x sigma of the
    current frame's 5x5 window (hit pixels inside the frame); where that changes it, the radiance is pulled towards the clamped value by
    `power` and the count shrinks by power x min(1, |change| / luminance). The count grows by one up to max_frames and the sample is
    blended in with weight 1 / count. A miss pixel's accumulation is 0.
  spatial: eight taps on a golden-angle spiral (radius sqrt((k + 0.5) / 8), weight exp(-2 r^2)), turned by one of 16 rotations
    ((k + 0.5) 2 pi / 16) picked by a hash of pixel and frame index, scaled by radius = min(R, R (0.25 + 0.75 hd / (hd + 8)) / sqrt(count))
    and rounded to pixels; skipped altogether when radius < 0.5. A tap counts under the same four tests against the current frame's
    geometry, with weight x (1 - plane offset / tolerance). The weighted mean (the pixel itself with weight 1) is packed as YCoCg +
    hit distance halves. Miss pixels are not written.

Decisions. Wherever the filter compares floats the witness evaluates both sides in float64, states next to the comparison a forward
bound on what a float32 evaluation can be off by, and marks the pixel UNDECIDED when the sides are closer than that. Undecided pixels
are not compared (tests cap them at UNDECIDED_CAP of the hit pixels). EPS = 2^-24 is float32's half ulp; a chain of k roundings on
values of magnitude S is bounded by k EPS S, and the bounds below take k generously (16 for a reconstructed point).

Every check is ONE step: the history that goes in is what the caller uploaded or downloaded, never something this module ran."""
import functools
from types import SimpleNamespace

import numpy as np

from image_witness import half_steps, half_value, lit, pack_radiance, to_half, unpack_radiance

F = np.float32
EPS = 2.0 ** -24
UNDECIDED_CAP = 0.05
SNAP = 1.0 / 512.0
# worst |oracle - witness| / M of the accumulation's rgb over decided pixels of every case (M: largest magnitude among the sample and
# the live taps' history). Measured by tests/test_denoise_witness.py::test_oracle_against_witness, which holds the oracle to it:
# measured 2.98e-5 at S2w 64x48, recorded rounded up to two digits. It is float32's own: a reprojected position is good to 2e-5 of a
# pixel (a point near 100 units rebuilt and projected), and where only a tap with a weight of a few thousandths survives, that error
# is divided by the weight. Cases whose taps are snapped stay below 2e-7.
DENOISE_ORACLE_DEV_MEASURED = 2.98e-5
DENOISE_ORACLE_DEV = 3.0e-5
INF = np.inf


# ------------------------------------------------------------------ cameras and geometry
def cam64(cam):
    """dust_amd._lib.Camera (float32 members) -> float64 arrays"""
    return SimpleNamespace(c0=np.array(list(cam.view_col0), np.float64), c1=np.array(list(cam.view_col1), np.float64),
                           c2=np.array(list(cam.view_col2), np.float64), pos=np.array(list(cam.position), np.float64),
                           tan=float(F(cam.tan_half_fov)))


def aspect_of(w, h):
    return float(F(w) / F(h))


def ray_dirs(c, w, h, px, py):
    """camera.glsl:4-16: the un-normalised primary ray through the centre of pixel (px, py); (..., 3)"""
    cx = (2.0 * (px + 0.5) / w - 1.0) * aspect_of(w, h) * c.tan
    cy = -(2.0 * (py + 0.5) / h - 1.0) * c.tan
    return cx[..., None] * c.c0 + cy[..., None] * c.c1 - c.c2


def unpack_normal(p):
    """nrd.glsl:54-94 on an A2B10G10R10 texel: octahedral x, y in the low twenty bits -> unit normal (..., 3)"""
    p = np.asarray(p, np.uint32)
    x = (p & 1023).astype(np.float64) / 1023.0 * 2.0 - 1.0
    y = ((p >> 10) & 1023).astype(np.float64) / 1023.0 * 2.0 - 1.0
    z = 1.0 - np.abs(x) - np.abs(y)
    t = np.clip(-z, 0.0, 1.0)
    x = x - t * np.where(x >= 0.0, 1.0, -1.0)
    y = y - t * np.where(y >= 0.0, 1.0, -1.0)
    n = np.stack([x, y, z], axis=-1)
    return n / np.sqrt((n * n).sum(axis=-1, keepdims=True))


def pack_normal(n):
    """nrd.glsl:25-52 as the product stores it: octahedral encoding, ten bits each, roughness 1, material 0"""
    n = np.asarray(n, np.float64)
    v = n / np.abs(n).sum(axis=-1, keepdims=True)
    wx = (1.0 - np.abs(v[..., 1])) * np.where(v[..., 0] >= 0.0, 1.0, -1.0)
    wy = (1.0 - np.abs(v[..., 0])) * np.where(v[..., 1] >= 0.0, 1.0, -1.0)
    ex, ey = np.where(v[..., 2] >= 0.0, v[..., 0], wx), np.where(v[..., 2] >= 0.0, v[..., 1], wy)
    cx, cy = np.rint((ex * 0.5 + 0.5) * 1023.0).astype(np.uint32), np.rint((ey * 0.5 + 0.5) * 1023.0).astype(np.uint32)
    return (cx | (cy << 10) | np.uint32(1023 << 20)).astype(np.uint32)


def luminance(rgb):
    return rgb[..., 0] * 0.25 + rgb[..., 1] * 0.5 + rgb[..., 2] * 0.25


def _mag(*vs):
    """sum of the magnitudes of every component of every vector: the scale S of a reconstructed point's rounding"""
    return sum(np.abs(v).sum(axis=-1) for v in vs)


def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx] where that lies in the frame, `fill` elsewhere"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if h - abs(dy) > 0 and w - abs(dx) > 0:
        out[yd, xd] = a[ys, xs]
    return out


def params(max_frames=30, disocclusion=0.01, sigma=2.0, power=0.8, radius=15.0):
    return dict(max_frames=max_frames, disocclusion=disocclusion, sigma=sigma, power=power, radius=radius)


def _p32(p):
    return float(p["max_frames"]), lit(p["disocclusion"]), lit(p["sigma"]), lit(p["power"]), lit(p["radius"])


# ------------------------------------------------------------------ the temporal step
def temporal(prev_planes, hist_accum_in, cur_planes, cam, prev_cam, par, have_history):
    """One temporal step -> namespace(accum (h, w, 4) float64, undecided (h, w) bool, scale (h, w): the M of the tolerance,
    count_exact (h, w) bool, flags: dict of (h, w) bool, one per branch taken).
    prev_planes: the planes of the frame before (their depth, normal and id are the history's geometry); hist_accum_in: (h, w, 4)
    float32, the accumulation that frame left (or whatever was uploaded in its place). Both ignored unless have_history."""
    max_frames, dis, sig, power, _ = _p32(par)
    depth = np.asarray(cur_planes["depth"], np.float64)
    h, w = depth.shape
    hit = depth != INF
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c, pc = cam64(cam), cam64(prev_cam)
    cur, _ = unpack_radiance(cur_planes["illuminance"])
    n = unpack_normal(cur_planes["normal"])
    ident = np.asarray(cur_planes["voxel_id"], np.uint32) & 0xFFFF
    und = np.zeros((h, w), bool)
    fl = {}
    hist = np.zeros((h, w, 3))
    hist_n = np.zeros((h, w))
    scale = np.abs(cur).max(axis=-1)
    blended = np.zeros((h, w), bool)         # the history came through weights other than exactly 1 and 0
    alive = np.zeros((h, w))                 # the weight of the live taps
    cmag = np.zeros((h, w))                  # the largest frame count among the live taps
    hmag = np.zeros((h, w))                  # the largest history magnitude among the live taps
    e_hist = np.zeros((h, w))                # relative error of the history a float32 evaluation carries in from its weights
    fl["no_history"] = hit & (not have_history)
    if have_history:
        pdepth = np.asarray(prev_planes["depth"], np.float64)
        phit = pdepth != INF
        pn = unpack_normal(prev_planes["normal"])
        pid = np.where(phit, np.asarray(prev_planes["voxel_id"], np.uint32) & 0xFFFF, 0xFFFFFFFF).astype(np.uint32)
        pacc = np.asarray(hist_accum_in, np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            d = ray_dirs(c, w, h, xx, yy)
            td = np.where(hit, depth, 0.0)[..., None] * d
            mv = half_value(cur_planes["motion"])[..., :3]
            xp = c.pos + td + mv
            rel = xp - pc.pos
            vx, vy, vz = rel @ pc.c0, rel @ pc.c1, rel @ pc.c2
        # the point is rebuilt from four vectors and projected on a unit axis: some 12 roundings at scale S
        e_v = 16.0 * EPS * (_mag(td, mv) + np.abs(c.pos).sum() + np.abs(pc.pos).sum())
        # (1) in front of the previous camera: vz < -1e-6
        front = hit & (vz < -lit(1e-6))
        und |= hit & (np.abs(vz + lit(1e-6)) <= e_v)
        fl["behind_prev"] = hit & ~front
        tp = np.where(front, -vz, 1.0)
        ku, kv = aspect_of(w, h) * pc.tan, pc.tan
        u, v = vx / tp / ku, vy / tp / kv
        fx, fy = (u * 0.5 + 0.5) * w - 0.5, (-v * 0.5 + 0.5) * h - 0.5

        def pos_bound(q, kq, size, coord):   # a quotient of two values off by e_v each, scaled to pixels, plus the chain's own roundings
            e_q = (e_v / tp) * (1.0 + np.abs(q)) + 2.0 * EPS * np.abs(q)
            return 0.5 * size * (e_q / kq + 3.0 * EPS * np.abs(q / kq)) + 4.0 * EPS * (size + np.abs(coord) + 1.0)
        e_fx, e_fy = pos_bound(vx / tp, ku, w, fx), pos_bound(vy / tp, kv, h, fy)
        # (2) snap within 1/512 of a pixel centre; (3) floor of the tap coordinate: a position that is not snapped lies 1/512 - e from
        # every integer, so its floor is decided whenever the snap is; a snapped one is an integer exactly
        snapped = []
        for coord, e in ((fx, e_fx), (fy, e_fy)):
            off = np.abs(coord - np.rint(coord))
            und |= front & (np.abs(off - SNAP) <= e)
            snapped.append(off < SNAP)
        fx, fy = np.where(snapped[0], np.rint(fx), fx), np.where(snapped[1], np.rint(fy), fy)
        fl["snapped"] = front & snapped[0] & snapped[1]
        fl["unsnapped"] = front & ~(snapped[0] & snapped[1])
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        e_ax, e_ay = np.where(snapped[0], 0.0, e_fx) + 2.0 * EPS, np.where(snapped[1], 0.0, e_fy) + 2.0 * EPS
        e_w = e_ax + e_ay                    # of any one bilinear weight
        e_sum = np.zeros((h, w))             # of the live taps' weights together
        sum_w, acc, acc_n = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
        live_n = np.zeros((h, w), np.int32)
        in_n = np.zeros((h, w), np.int32)
        hist_mag = np.zeros((h, w))
        cnt_mag = np.zeros((h, w))
        rej = {k: np.zeros((h, w), bool) for k in ("hole", "id", "normal", "plane")}
        off_edge = {k: np.zeros((h, w), bool) for k in ("left", "right", "top", "bottom")}
        for k in range(4):
            xi, yi = x0 + (k & 1), y0 + (k >> 1)
            # (4) tap in frame: integers against integers, exact
            inside = front & (xi >= 0) & (yi >= 0) & (xi < w) & (yi < h)
            off_edge["left"] |= front & (xi < 0); off_edge["right"] |= front & (xi >= w)
            off_edge["top"] |= front & (yi < 0); off_edge["bottom"] |= front & (yi >= h)
            in_n += inside
            jx, jy = np.where(inside, xi, 0).astype(np.int64), np.where(inside, yi, 0).astype(np.int64)
            th = pdepth[jy, jx]
            ok = inside & (th != INF)
            rej["hole"] |= inside & ~ok
            # (5) instance id: integers, exact
            same = pid[jy, jx] == ident
            rej["id"] |= ok & ~same
            ok &= same
            # (6) normal dot below 0.9: two unit vectors from ten-bit codes, a dozen roundings at scale 1
            nd = (n * pn[jy, jx]).sum(axis=-1)
            und |= ok & (np.abs(nd - lit(0.9)) <= 32.0 * EPS)
            rej["normal"] |= ok & (nd < lit(0.9))
            ok &= nd >= lit(0.9)
            # (7) plane offset against the tolerance: the difference of two rebuilt points on a unit normal, against a product of three
            with np.errstate(invalid="ignore", over="ignore"):
                dh = ray_dirs(pc, w, h, xi, yi)
                thd = np.where(ok, th, 0.0)[..., None] * dh
                off = np.abs((n * (pc.pos + thd - xp)).sum(axis=-1))
                tol = dis * tp * np.sqrt((dh * dh).sum(axis=-1))
            e_off = 16.0 * EPS * (_mag(thd) + np.abs(pc.pos).sum()) + e_v + 8.0 * EPS * tol
            und |= ok & (np.abs(off - tol) <= e_off)
            rej["plane"] |= ok & (off > tol)
            ok &= ~(off > tol)
            wx, wy = np.where(k & 1, ax, 1.0 - ax), np.where(k >> 1, ay, 1.0 - ay)
            wk = np.where(ok, wx * wy, 0.0)
            e_sum += np.where(ok, wx * e_ay + wy * e_ax + 4.0 * EPS, 0.0)   # a product of two factors, each off by its coordinate's error
            tap = pacc[jy, jx]
            acc += wk[..., None] * tap[..., :3]
            acc_n += wk * tap[..., 3]
            sum_w += wk
            live_n += ok
            hist_mag = np.maximum(hist_mag, np.where(ok & (wk > 0), np.abs(tap[..., :3]).max(axis=-1), 0.0))
            cnt_mag = np.maximum(cnt_mag, np.where(ok & (wk > 0), np.abs(tap[..., 3]), 0.0))
        # (8) sum_w > 1e-3: the live weights' errors, and three additions
        have = front & (sum_w > lit(1e-3))
        und |= front & (live_n > 0) & (np.abs(sum_w - lit(1e-3)) <= e_sum + 4.0 * EPS)
        sw = np.where(have, sum_w, 1.0)
        hist = np.where(have[..., None], acc / sw[..., None], 0.0)
        hist_n = np.where(have, acc_n / sw, 0.0)
        scale = np.maximum(scale, np.where(have, hist_mag, 0.0))
        alive = np.where(front, sum_w, 0.0)
        hmag, cmag = np.where(have, hist_mag, 0.0), np.where(have, cnt_mag, 0.0)
        blended = have & ~((sum_w == 1.0) & fl["snapped"])
        e_hist = np.where(blended, 8.0 * e_w / sw + 16.0 * EPS, 0.0)
        fl["sum_w_small"] = front & (live_n > 0) & ~have
        fl["all_taps_off"] = front & (in_n == 0)
        fl["own_pixel_weight_1"] = have & ~blended
        for k in range(5):
            fl[f"live_taps_{k}"] = front & (live_n == k) & (in_n > 0)
        for k, m in rej.items():
            fl["reject_" + k] = m
        for k, m in off_edge.items():
            fl["tap_off_" + k] = m
    # ---- antilag
    fl["antilag_off"] = hit & (hist_n > 0) & (power <= 0.0)
    changed = np.zeros((h, w), bool)
    if power > 0.0:
        ylum = np.where(hit, luminance(cur), 0.0)
        s1, s2, cnt = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        held_miss = np.zeros((h, w), bool)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                m = _shift(hit, dy, dx, False)
                y = _shift(ylum, dy, dx, 0.0)
                s1 += np.where(m, y, 0.0); s2 += np.where(m, y * y, 0.0); cnt += m
                held_miss |= _shift(~hit, dy, dx, False)
        use = hit & (hist_n > 0)
        cn = np.maximum(cnt, 1.0)
        mean = s1 / cn
        var = s2 / cn - mean * mean
        # 25 additions of squares, a quotient and a difference that cancels: the variance is known to 32 EPS of the mean square
        e_var = 32.0 * EPS * (s2 / cn)
        sigma = np.sqrt(np.maximum(var, 0.0))
        e_sigma = np.maximum(np.sqrt(np.maximum(var + e_var, 0.0)) - sigma, sigma - np.sqrt(np.maximum(var - e_var, 0.0))) + 2.0 * EPS * sigma
        lo, hi = mean - sig * sigma, mean + sig * sigma
        yh = luminance(hist)
        e_yh = (e_hist + 4.0 * EPS) * np.maximum(yh, hmag)   # the weights' error acts on the taps' magnitudes, not on their mean
        e_edge = 32.0 * EPS * mean + sig * e_sigma + 4.0 * EPS * (np.abs(mean) + sig * sigma) + e_yh
        # (9) the clamp changed the luminance: yh outside [lo, hi]
        yc = np.clip(yh, lo, hi)
        und |= use & ((np.abs(yh - lo) <= e_edge) | (np.abs(yh - hi) <= e_edge))
        # (10) yh > 1e-12
        big = yh > lit(1e-12)
        und |= use & (yc != yh) & (np.abs(yh - lit(1e-12)) <= e_yh + 4.0 * EPS * 1e-12)
        changed = use & (yc != yh) & big
        yh1 = np.where(changed, yh, 1.0)
        pull = np.where(changed, power * (yc / yh1 - 1.0) + 1.0, 1.0)
        hist = hist * pull[..., None]
        hist_n = hist_n * np.where(changed, 1.0 - power * np.minimum(1.0, np.abs(yh - yc) / yh1), 1.0)
        # what the clamp's own edges carry into the pulled history: power x e_edge / yh of it
        e_hist = e_hist + np.where(changed, power * e_edge / yh1 + 8.0 * EPS, 0.0)
        fl["clamp_above"] = use & big & (yh > hi)
        fl["clamp_below"] = use & big & (yh < lo)
        fl["clamp_inside"] = use & (yc == yh) & big
        fl["yh_tiny"] = use & ~big
        px, py = xx.astype(np.int64), yy.astype(np.int64)
        near_l, near_r, near_t, near_b = px < 2, px >= w - 2, py < 2, py >= h - 2
        fl["win_corner_tl"], fl["win_corner_tr"] = use & near_t & near_l, use & near_t & near_r
        fl["win_corner_bl"], fl["win_corner_br"] = use & near_b & near_l, use & near_b & near_r
        fl["win_miss"] = use & held_miss
        fl["win_tile_x"] = use & ((px % 16 < 2) | (px % 16 >= 14)) & (px >= 2) & (px < w - 2) & ((px + 2) // 16 != (px - 2) // 16)
        fl["win_tile_y"] = use & ((py % 16 < 2) | (py % 16 >= 14)) & (py >= 2) & (py < h - 2) & ((py + 2) // 16 != (py - 2) // 16)
    # (11) the max_frames cap: min() is continuous, so the value does not hang on the decision; the flag does
    grown = hist_n + 1.0
    e_n = np.where(blended | changed, (e_hist + 8.0 * EPS) * np.maximum(grown, 1.0), 0.0)
    capped = hit & (grown > max_frames)
    fl["cap_hit"] = capped & (np.abs(grown - max_frames) > e_n)
    fl["cap_fractional"] = fl["cap_hit"] & (grown != np.rint(grown))
    fl["cap_not_hit"] = hit & (hist_n > 0) & (grown < max_frames - e_n)
    nn = np.minimum(grown, max_frames)
    al = 1.0 / nn
    out = np.zeros((h, w, 4))
    out[..., :3] = hist * (1.0 - al)[..., None] + cur * al[..., None]
    out[..., 3] = nn
    out[~hit] = 0.0
    for k in fl:
        fl[k] = fl[k] & hit & ~und
    return SimpleNamespace(accum=out, undecided=und & hit, scale=np.where(hit, scale, 0.0), count_scale=np.maximum(cmag, 1.0), weight=alive, count_exact=hit & ~blended & ~changed,
                           flags=fl, hit=hit)


# ------------------------------------------------------------------ the spatial step
def disc():
    """golden-angle spiral of 8 points: (x, y, weight), to float32 as any table of literals is"""
    k = np.arange(8, dtype=np.float64)
    r = np.sqrt((k + 0.5) / 8.0)
    a = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(a), r * np.sin(a), np.exp(-2.0 * r * r)], axis=1).astype(F).astype(np.float64)


def rotations():
    a = (np.arange(16, dtype=np.float64) + 0.5) * (2.0 * np.pi / 16.0)
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(F).astype(np.float64)


def rotation_index(w, h, frame_index):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.uint64)
    m = 0xFFFFFFFF
    hh = ((xx * 0x9E3779B1) & m) ^ ((yy * 0x85EBCA77) & m) ^ ((int(frame_index) * 0xC2B2AE3D) & m)
    hh ^= hh >> 15
    hh = (hh * 0x2C1B3C6D) & m
    hh ^= hh >> 12
    return (hh & 15).astype(np.int64)


def spatial(accum, cur_planes, cam, par, frame_index):
    """One spatial step on the accumulation plane as it stood (float32 values) -> namespace(denoised (h, w, 4) uint16: the pack of the
    float64 result, `denoised` of cur_planes where nothing is written; undecided, flags, rotation (h, w) int, -1 where no tap is taken)."""
    _, dis, _, _, maxr = _p32(par)
    acc = np.asarray(accum, np.float64)
    depth = np.asarray(cur_planes["depth"], np.float64)
    h, w = depth.shape
    hit = depth != INF
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c = cam64(cam)
    hd = half_value(np.asarray(cur_planes["illuminance"])[..., 3])
    n = unpack_normal(cur_planes["normal"])
    ident = np.asarray(cur_planes["voxel_id"], np.uint32) & 0xFFFF
    und = np.zeros((h, w), bool)
    fl = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        radius = np.minimum(maxr, maxr * (0.25 + 0.75 * (hd / (hd + 8.0))) / np.sqrt(np.where(hit, acc[..., 3], 1.0)))
        # (12) radius >= 0.5: five roundings at scale radius
        wide = hit & (radius >= 0.5)
        und |= hit & (np.abs(radius - 0.5) <= 8.0 * EPS)
        d = ray_dirs(c, w, h, xx, yy)
        td = np.where(hit, depth, 0.0)[..., None] * d
        x = c.pos + td
        tol = dis * np.where(hit, depth, 0.0) * np.sqrt((d * d).sum(axis=-1))
    rot = rotation_index(w, h, frame_index)
    rc, rs = rotations()[rot, 0], rotations()[rot, 1]
    total, wsum = acc[..., :3].copy(), np.ones((h, w))
    rej = {k: np.zeros((h, w), bool) for k in ("frame", "miss", "id", "normal", "plane")}
    off_edge = {k: np.zeros((h, w), bool) for k in ("left", "right", "top", "bottom")}
    taken = np.zeros((h, w), np.int32)
    rad = np.where(wide, radius, 0.0)
    for dx, dy, wt in disc():
        ox, oy = (dx * rc - dy * rs) * rad, (dx * rs + dy * rc) * rad
        # (13) rint of the tap offset: three roundings at scale |o|, and the radius's own
        for o in (ox, oy):
            und |= wide & (np.abs(np.abs(o - np.floor(o)) - 0.5) <= 16.0 * EPS * (np.abs(o) + 1.0))
        xi, yi = xx + np.rint(ox), yy + np.rint(oy)
        inside = wide & (xi >= 0) & (yi >= 0) & (xi < w) & (yi < h)
        off_edge["left"] |= wide & (xi < 0); off_edge["right"] |= wide & (xi >= w)
        off_edge["top"] |= wide & (yi < 0); off_edge["bottom"] |= wide & (yi >= h)
        rej["frame"] |= wide & ~inside
        jx, jy = np.where(inside, xi, 0).astype(np.int64), np.where(inside, yi, 0).astype(np.int64)
        tj = depth[jy, jx]
        ok = inside & (tj != INF)
        rej["miss"] |= inside & ~ok
        same = ident[jy, jx] == ident
        rej["id"] |= ok & ~same
        ok &= same
        nd = (n * n[jy, jx]).sum(axis=-1)
        und |= ok & (np.abs(nd - lit(0.9)) <= 32.0 * EPS)
        rej["normal"] |= ok & (nd < lit(0.9))
        ok &= nd >= lit(0.9)
        with np.errstate(invalid="ignore", over="ignore"):
            dj = ray_dirs(c, w, h, xi, yi)
            tdj = np.where(ok, tj, 0.0)[..., None] * dj
            off = np.abs((n * (c.pos + tdj - x)).sum(axis=-1))
        e_off = 16.0 * EPS * (_mag(tdj, td) + 2.0 * np.abs(c.pos).sum()) + 8.0 * EPS * tol
        und |= ok & (np.abs(off - tol) <= e_off)
        rej["plane"] |= ok & (off > tol)
        ok &= ~(off > tol)
        with np.errstate(invalid="ignore", divide="ignore"):
            wk = np.where(ok, wt * (1.0 - off / np.where(ok, tol, 1.0)), 0.0)
        total += wk[..., None] * acc[jy, jx, :3]
        wsum += wk
        taken += ok
    res = total / wsum[..., None]
    den = pack_radiance(res, hd)
    den = np.where(hit[..., None], den, np.asarray(cur_planes["denoised"], np.uint16))
    fl["radius_small"], fl["radius_wide"] = hit & ~wide, wide
    fl["hitdist_zero"] = hit & (hd == 0.0)
    fl["hitdist_floor"] = hit & (hd != 0.0) & (hd < lit(1e-7))
    for k, m in rej.items():
        fl["reject_" + k] = m
    for k, m in off_edge.items():
        fl["tap_off_" + k] = m
    fl["taps_taken"] = wide & (taken > 0)
    for k in fl:
        fl[k] = fl[k] & hit & ~und
    return SimpleNamespace(denoised=den, undecided=und & hit, flags=fl, rotation=np.where(wide & ~und, rot, -1), hit=hit, result=res)


# ------------------------------------------------------------------ the comparisons both test files make
def check_temporal(got, wit, bound, what=""):
    """got: (h, w, 4) float32 accumulation. -> worst |got - witness| / M over decided pixels. Raises AssertionError."""
    got = np.asarray(got, np.float64)
    hit, dec = wit.hit, wit.hit & ~wit.undecided
    assert np.all(got[~hit] == 0.0), f"{what}: a miss pixel's accumulation is not 0"
    assert np.isfinite(got[hit]).all(), f"{what}: a hit pixel's accumulation is not finite"
    err = np.abs(got[..., :3] - wit.accum[..., :3]).max(axis=-1)
    m = np.where(wit.scale > 0, wit.scale, 1.0)
    assert np.all(err[dec & (wit.scale == 0)] == 0.0), f"{what}: black in, not black out"
    rel = np.where(dec, err / m, 0.0)
    worst = float(rel.max()) if rel.size else 0.0
    if worst > bound:
        at = np.unravel_index(np.argmax(rel), rel.shape)
        raise AssertionError(f"{what}: accumulation off by {worst:.3e} M (bound {bound:.3e}) at pixel (x {at[1]}, y {at[0]}): "
                             f"got {got[at]}, witness {wit.accum[at]}")
    exact = dec & wit.count_exact
    bad = exact & (got[..., 3] != wit.accum[..., 3])
    assert not bad.any(), f"{what}: frame count differs at {np.argwhere(bad)[:4].tolist()}: got {got[..., 3][bad][:4]}, witness {wit.accum[..., 3][bad][:4]}"
    loose = dec & ~wit.count_exact
    cerr = np.abs(got[..., 3] - wit.accum[..., 3]) / wit.count_scale   # the same M, on the count channel
    assert np.all(cerr[loose] <= bound), f"{what}: blended frame count off by {float(cerr[loose].max()):.3e}"
    return worst


def check_spatial(got, wit, what=""):
    """got: (h, w, 4) uint16 denoised plane. -> worst half steps over decided pixels. Raises AssertionError."""
    got = np.asarray(got, np.uint16)
    hit, dec = wit.hit, wit.hit & ~wit.undecided
    assert np.array_equal(got[~hit], wit.denoised[~hit]), f"{what}: a miss pixel's denoised texel was written"
    assert np.array_equal(got[hit][:, 3], wit.denoised[hit][:, 3]), f"{what}: hit distance"
    steps = half_steps(got[..., :3], wit.denoised[..., :3]).max(axis=-1)
    steps = np.where(dec, steps, 0)
    worst = int(steps.max()) if steps.size else 0
    if worst > 1:
        at = np.unravel_index(np.argmax(steps), steps.shape)
        raise AssertionError(f"{what}: denoised off by {worst} half steps at pixel (x {at[1]}, y {at[0]}): got {half_value(got[at])}, "
                             f"witness {half_value(wit.denoised[at])}")
    return worst


# ------------------------------------------------------------------ inputs: an analytic scene
EYE = (30.0, 40.0, 60.0)
TARGET_SKY, TARGET_DOWN = (0.0, 14.0, 0.0), (0.0, 0.0, 0.0)     # the first sees over the wall (sky in the top rows), the second does not
WALL_Z, WALL_TOP, BOX_Y = -20.0, 30.0, 6.0
BOX_X, BOX_Z = (-12.0, 6.0), (-8.0, 12.0)
NORMAL_UP, NORMAL_WALL = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
PATCHES = ("other_id", "high_bits", "normal", "depth", "hole")
SIZES = ((1, 1), (16, 16), (17, 3), (37, 21), (64, 48))


def camera(eye=EYE, target=TARGET_SKY):
    from dust_amd.scenes import camera_for   # late: the witness functions need nothing of the package
    return camera_for(eye, target=target)


def scene_geometry(w, h, cam, box_at=(0.0, 0.0)):
    """-> depth (h, w) float32 (+inf: sky), normal (h, w) uint32, voxel_id (h, w) uint32 of the analytic scene: floor y = 0 up to the wall
    (instance 0), wall z = WALL_Z up to WALL_TOP (1), a plate at y = BOX_Y moved by box_at in x and z (2), sky elsewhere."""
    c = cam64(cam)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = ray_dirs(c, w, h, xx, yy)
    best = np.full((h, w), INF)
    ident = np.zeros((h, w), np.uint32)
    nrm = np.zeros((h, w, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        for inst, (axis, level, normal) in enumerate(((1, 0.0, NORMAL_UP), (2, WALL_Z, NORMAL_WALL), (1, BOX_Y, NORMAL_UP))):
            t = (level - c.pos[axis]) / d[..., axis]
            p = c.pos + np.where(np.isfinite(t), t, 0.0)[..., None] * d
            ok = np.isfinite(t) & (t > 0)
            if inst == 0:
                ok &= p[..., 2] >= WALL_Z
            elif inst == 1:
                ok &= (p[..., 1] >= 0.0) & (p[..., 1] <= WALL_TOP)
            else:
                ok &= (p[..., 0] >= BOX_X[0] + box_at[0]) & (p[..., 0] <= BOX_X[1] + box_at[0])
                ok &= (p[..., 2] >= BOX_Z[0] + box_at[1]) & (p[..., 2] <= BOX_Z[1] + box_at[1])
            ok &= t < best
            best = np.where(ok, t, best)
            ident = np.where(ok, np.uint32(inst), ident)
            nrm = np.where(ok[..., None], np.asarray(normal), nrm)
    hit = np.isfinite(best)
    normal = np.where(hit, pack_normal(np.where(hit[..., None], nrm, NORMAL_UP)), 0).astype(np.uint32)
    return best.astype(F), normal, ident


def apply_patches(geo, rng, region, density):
    """lay the five patches over hit pixels of `region` with probability `density`; -> (depth, normal, voxel_id, kind (h, w) int: 0 none,
    1 + index into PATCHES)"""
    depth, normal, ident = (a.copy() for a in geo)
    hit = np.isfinite(depth)
    kind = np.where(hit & region & (rng.uniform(size=depth.shape) < density), rng.integers(1, 6, depth.shape), 0)
    ident = np.where(kind == 1, ident + 4, ident)
    ident = np.where(kind == 2, ident | (rng.integers(1, 0xFFFF, depth.shape).astype(np.uint32) << 16), ident).astype(np.uint32)
    n = unpack_normal(normal)
    turned = n + 0.58 * np.array([1.0, 0.0, 0.0])          # 30 degrees off: dot 0.865
    normal = np.where(kind == 3, pack_normal(turned), normal).astype(np.uint32)
    depth = np.where(kind == 4, (depth.astype(np.float64) * 1.05).astype(F), depth)
    depth = np.where(kind == 5, F(INF), depth).astype(F)
    normal = np.where(kind == 5, 0, normal).astype(np.uint32)
    return depth, normal, ident, kind


def _chroma_sign(ident):
    """Co and Cg keep one sign per instance, so that no mean of texels the filter may mix cancels its chroma (a float32 pack rounds Cg at
    the size of g: image_witness.accumulate_inputs); instance 2 is grey"""
    k = np.asarray(ident, np.uint32) & 3
    return np.stack([np.where(k == 0, 1.0, np.where(k == 1, -1.0, 0.0)), np.where(k == 0, -1.0, np.where(k == 1, 1.0, 0.0))], axis=-1)


def radiance(rng, ident, y_lo, y_hi):
    """-> (Y, Co, Cg) (h, w, 3) float64: luminance log-uniform over 2^lo .. 2^hi, chroma 0.05 .. 0.3 of it"""
    y = 2.0 ** rng.uniform(y_lo, y_hi, ident.shape)
    ch = _chroma_sign(ident) * rng.uniform(0.05, 0.3, ident.shape + (2,)) * y[..., None]
    return np.stack([y, ch[..., 0], ch[..., 1]], axis=-1)


def hit_distances(rng, shape):
    """halves: 0, the smallest subnormal (below the pack's 1e-7 floor), or 0.01 .. 60000"""
    pick = rng.uniform(size=shape)
    return np.where(pick < 0.15, 0, np.where(pick < 0.3, 1, to_half(10.0 ** rng.uniform(-2.0, np.log10(60000.0), shape)))).astype(np.uint16)


def make_planes(rng, geo, motion=None, y_range=(-4.0, 4.0), hitdist=None):
    depth, normal, ident = geo[:3]
    h, w = depth.shape
    ycc = radiance(rng, ident, *y_range)
    hd = hit_distances(rng, (h, w)) if hitdist is None else np.full((h, w), hitdist, np.uint16)
    ill = np.concatenate([to_half(ycc), hd[..., None]], axis=-1).astype(np.uint16)
    mot = np.zeros((h, w, 4), np.uint16) if motion is None else motion
    return dict(depth=depth, normal=normal, voxel_id=ident, illuminance=ill, motion=mot,
                denoised=np.full((h, w, 4), 0xFFFF, np.uint16))   # a texel the pass should not write shows


def history(rng, prev_geo, counts, y_range=(-4.0, 4.0), scale=None):
    """an accumulation plane unrelated to any sample: rgb from the same recipe as the texels, counts drawn from `counts`; 0 at misses"""
    depth, _, ident = prev_geo[:3]
    ycc = radiance(rng, ident, *y_range)
    if scale is not None:
        ycc = ycc * scale[..., None]
    t = ycc[..., 0] - ycc[..., 2]
    rgb = np.stack([t + ycc[..., 1], ycc[..., 0] + ycc[..., 2], t - ycc[..., 1]], axis=-1)
    acc = np.concatenate([rgb, rng.choice(np.asarray(counts, np.float64), depth.shape)[..., None]], axis=-1).astype(F)
    acc[~np.isfinite(depth)] = 0.0
    return acc


COUNTS = (1.0, 2.0, 2.5, 28.75, 29.0, 30.0)
# Under a pan the taps are blended with weights that carry the reprojected position's rounding, and what that does to a channel grows
# with the contrast between the taps. The radiance has all the contrast there is (eight octaves); the counts of the pan cases keep
# theirs at 3/4 of the largest, so that the count channel, measured on its own largest tap, stays inside the radiance's bound.
PAN_COUNTS = (8.0, 16.0, 24.0, 29.5)
# name -> (what it exercises, sizes). One table, as image_witness.tone_cases() is.
CASES = {
    "S0": ("first frame: no history", SIZES),
    "S1": ("static camera, uploaded history, counts meeting the cap at 30; the plate creeps through the snap threshold", SIZES),
    "S1m6": ("the same with max_frames 6", SIZES),
    "S2": ("sub-pixel pan, four live taps, rejection patches under them", SIZES[3:]),
    "S2w": ("a pan of a few hundredths of a pixel: surviving weights on both sides of 1e-3", SIZES[3:]),
    "S3a": ("pan of several pixels up-left: taps off the frame", SIZES[3:]),
    "S3b": ("pan of several pixels down-right", SIZES[3:]),
    "S4": ("previous camera turned away: every point behind it", SIZES[3:]),
    "S5a": ("antilag, power 0.8, sigma scale 2", SIZES[3:]),
    "S5b": ("antilag, power 0.8, sigma scale 0.5", SIZES[3:]),
    "S5c": ("antilag power 0: the window is never staged", SIZES[3:]),
    "S6r0n1": ("spatial, max_blur_radius 0, count 1", SIZES[3:]),
    "S6r3n1": ("spatial, max_blur_radius 3, count 1", SIZES[3:]),
    "S6r15n1": ("spatial, max_blur_radius 15, count 1", SIZES[3:]),
    "S6r3n30": ("spatial, max_blur_radius 3, count 30: radius on both sides of 0.5", SIZES[3:]),
    "S6r15n30": ("spatial, max_blur_radius 15, count 30", SIZES[3:]),
}


def cases():
    return [(name, w, h) for name, (_, sizes) in CASES.items() for (w, h) in sizes]


def _pan(target, right, up):
    """a look-at target moved so that the view turns: the previous frame's camera"""
    return (target[0] + right, target[1] + up, target[2] - 0.4 * right)


@functools.lru_cache(maxsize=None)
def case_inputs(name, w, h):
    """-> dict(cur, prev: plane dicts (prev None without history); cam, prev_cam; hist: (h, w, 4) float32 or None; params; have_history;
    frame_index). Everything from fixed seeds: the CPU tests measure their margins on exactly what the GPU tests upload."""
    rng = np.random.default_rng([71, sorted(CASES).index(name), w, h])
    yy, xx = np.mgrid[0:h, 0:w]
    par = params()
    frame_index = 3 + sorted(CASES).index(name)
    target = TARGET_DOWN if name[:2] in ("S3", "S5") else TARGET_SKY
    cam = camera(EYE, target)
    prev_cam, have = cam, True
    y_range = (-4.0, 4.0)
    box_prev, box_cur = (0.0, 0.0), (0.0, 0.0)
    prev_patch = cur_patch = None      # (region, density)
    counts, hist_scale = COUNTS, None
    if name == "S0":
        have = False
    elif name in ("S1", "S1m6"):
        par = params(power=0.0, max_frames=6 if name == "S1m6" else 30)
        box_prev = (-0.006, 0.004)     # a few thousandths of a pixel at this distance: offsets on both sides of 1/512
    elif name in ("S2", "S2w"):
        par, counts = params(power=0.0), PAN_COUNTS
        a = 0.55 if name == "S2" else 0.07
        prev_cam = camera(EYE, _pan(target, a * 1.1, -a * 0.9))
        box_prev = (-0.75, 0.5) if name == "S2" else (0.0, 0.0)
        prev_patch = (xx >= w // 3, 0.5)
    elif name in ("S3a", "S3b"):
        par, counts = params(power=0.0), PAN_COUNTS
        s = 1.0 if name == "S3a" else -1.0
        prev_cam = camera(EYE, _pan(target, 6.0 * s, -4.5 * s))
    elif name == "S4":
        prev_cam = camera(EYE, (2.0 * EYE[0] - target[0], 2.0 * EYE[1] - target[1], 2.0 * EYE[2] - target[2]))
    elif name[:2] == "S5":
        par = params(power=0.0 if name == "S5c" else 0.8, sigma=0.5 if name == "S5b" else 2.0)
        y_range = (-1.0, 1.0)
        cur_patch = (np.ones((h, w), bool), 0.12)
        counts = (4.0, 12.0, 29.5)
    elif name[:2] == "S6":
        r, n = name[3:].split("n")
        par = params(power=0.0, radius=float(r))
        have = n == "30"
        counts = (30.0, 29.0)
        cur_patch = (np.ones((h, w), bool), 0.25)
    cur_geo = scene_geometry(w, h, cam, box_cur)
    kind_cur = np.zeros((h, w), np.int64)
    if cur_patch:
        *cur_geo, kind_cur = apply_patches(cur_geo, rng, *cur_patch)
        if name[:2] == "S5":           # antilag wants holes in its windows, not rejected histories: keep only them
            base = scene_geometry(w, h, cam, box_cur)
            cur_geo = [np.where(kind_cur == 5, g, b) for g, b in zip(cur_geo, base)]
    motion = np.zeros((h, w, 4), np.uint16)
    moved = np.array([box_prev[0] - box_cur[0], 0.0, box_prev[1] - box_cur[1]])   # where the point was minus where it is
    motion[..., :3] = np.where((cur_geo[2] == 2)[..., None], to_half(moved), 0)
    cur = make_planes(rng, cur_geo, motion, y_range)
    prev = hist = None
    kind_prev = np.zeros((h, w), np.int64)
    if have:
        if name[:2] in ("S5", "S6"):   # static: the frame before showed the same geometry
            prev_geo = [g.copy() for g in cur_geo]
        else:
            prev_geo = scene_geometry(w, h, prev_cam, box_prev)
            if prev_patch:
                *prev_geo, kind_prev = apply_patches(prev_geo, rng, *prev_patch)
        prev = make_planes(rng, prev_geo, None, y_range)
        if name[:2] == "S5":           # history luminance far above, far below, inside the window's range, and black
            pick = rng.integers(0, 4, (h, w))
            hist_scale = np.where(pick == 0, 8.0, np.where(pick == 1, 1.0 / 16.0, 1.0))
            hist = history(rng, prev_geo, counts, (0.0, 0.2), hist_scale)
            hist[pick == 3, :3] = 0.0
        else:
            hist = history(rng, prev_geo, counts, y_range)
    for p in (cur, prev):
        if p:
            for a in p.values():
                a.setflags(write=False)
    if hist is not None:
        hist.setflags(write=False)
    return dict(cur=cur, prev=prev, cam=cam, prev_cam=prev_cam, hist=hist, params=par, have_history=have, frame_index=frame_index,
                patch_prev=kind_prev, patch_cur=kind_cur)
