"""tests/image_witness.py held against the C oracle on the CPU, on exactly the inputs tests/test_gpu_image_passes.py uploads, and the
conditions those inputs have to meet. What comes out of here is the margin the GPU tests use: the witness and the oracle's float32
evaluation agree to one half-precision step per channel outside the band |o| < 2^-12 for all nine transfer functions, bin for bin on the
histogram, and to EXPOSURE_ORACLE_DEV on the adapted average."""
import ctypes as C

import numpy as np
import pytest

import image_witness as W
import oracle_lib as O


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_tone_map(den, alb, avg, conv, tf):
    h, w = alb.shape
    out = np.zeros((h, w, 4), np.uint16)
    O.lib().orc_tone_map(_p(np.ascontiguousarray(den)), _p(np.ascontiguousarray(alb)), w, h, avg, (C.c_float * 9)(*[float(v) for v in conv]), tf, _p(out))
    return out


def oracle_histogram(den, min_log, max_log):
    h, w = den.shape[:2]
    hist = np.zeros(256, np.uint32)
    O.lib().orc_exposure_histogram(_p(np.ascontiguousarray(den)), w, h, min_log, max_log - min_log, _p(hist))
    return hist


# ------------------------------------------------------------------ the witness's own arithmetic, by hand
def test_unpack_pack_and_half_helpers():
    h = W.to_half(np.array([[0.5, 0.125, -0.25, 3.0], [np.nan, 0.0, 0.0, 0.0], [1.0, np.nan, 0.0, 0.0]]))
    rgb, hd = W.unpack_radiance(h)
    assert np.array_equal(rgb[0], [0.875, 0.25, 0.625]) and hd[0] == 3.0
    assert np.array_equal(rgb[1], [0.0, 0.0, 0.0])          # a NaN channel is 0 after max(., 0)
    assert np.array_equal(rgb[2], [0.0, 1.0, 0.0])
    back = W.pack_radiance(rgb[:1], hd[:1])
    assert np.array_equal(back, h[:1])
    assert W.pack_radiance(np.zeros(3), 1e-9)[3] == W.to_half(W.lit(1e-7)) == 2 and W.pack_radiance(np.zeros(3), 0.0)[3] == 0
    u = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7BFF, 0x7C00, 0xFC00], np.uint16)
    assert W.half_ordinal(u).tolist() == [0, 0, 1, -1, 0x7BFF, 0x7C00, -0x7C00]
    assert W.half_is_nan(np.array([0x7E00, 0x7C00, 0xFE01], np.uint16)).tolist() == [True, False, True]
    assert np.array_equal(W.accumulate(np.array([[1.0], [2.0], [6.0]]))[:, 0], [1.0, 1.5, 3.0])


def test_histogram_and_average_by_hand():
    den = np.zeros((4, 4), np.uint16)
    den[:, 0] = W.to_half([0.001, 0.5, np.inf, 0.0049])
    pos, below = W.histogram_position(den, -6.0, 14.5)
    assert below.tolist() == [True, False, False, True]
    assert np.isclose(pos[1], (np.log2(0.5) + 6.0) / 14.5 * 254.0 + 1.0, rtol=1e-7) and pos[2] == 255.0   # (the three float32 weights sum to 1 + 3e-8)
    hist = W.histogram(den, -6.0, 14.5)
    assert hist[0] == 2 and hist[int(pos[1])] == 1 and hist[255] == 1 and hist.sum() == 4
    # all pixels below the floor: the average heads for 2^(min - range / 254)
    floor_hist = np.zeros(256, np.uint32); floor_hist[0] = 51
    assert np.isclose(W.exposure_average(floor_hist, 51, -6.0, 14.5, 1.0, 0.0), 2.0 ** (-6.0 - 14.5 / 254.0), rtol=1e-12)
    assert np.isclose(W.exposure_average(floor_hist, 51, -6.0, 14.5, 0.2, 0.37), 0.37 + (2.0 ** (-6.0 - 14.5 / 254.0) - W.lit(0.37)) * W.lit(0.2), rtol=1e-7)


def test_transfer_functions_by_hand():
    # continuity at the knees, the published anchor points, NaN under a negative base
    for tf, knee in ((1, 0.0031308), (4, 0.0030186), (5, 0.0181), (7, 1.0 / 12.0)):
        lo, hi = W.oetf(tf, knee * (1 - 1e-6)), W.oetf(tf, knee * (1 + 1e-6))
        assert abs(hi - lo) < 2e-5, (tf, lo, hi)
    assert np.isclose(W.oetf(1, 1.0), 1.0, atol=1e-6) and np.isclose(W.oetf(5, 1.0), 1.0, atol=1e-6) and np.isclose(W.oetf(8, 1.0), 1.0)
    assert np.isclose(W.oetf(7, 1.0), 1.0, atol=1e-6) and np.isclose(W.oetf(7, 1.0 / 12.0 - 1e-9), 0.5, atol=1e-6)
    assert np.isclose(W.oetf(3, 52.37), 1.0, atol=1e-6) and np.isclose(W.oetf(6, 1.0), 1.0, atol=1e-6)
    assert np.isclose(W.oetf(2, -0.5), -W.oetf(1, 0.5)) and W.oetf(0, -0.25) == -0.25
    for tf in (3, 6, 7, 8):
        assert np.isnan(W.oetf(tf, -0.01))
    assert W.oetf(1, -0.01) == W.lit(12.92) * -0.01 and W.oetf(5, -0.01) == -0.045
    # mid grey through the whole chain by hand: grey albedo, identity conversion
    den = W.to_half(np.array([[0.18, 0.0, 0.0, 0.0]]))
    o, out = W.tone_map(den, W.grey_albedo(1023), 0.18, np.eye(3).reshape(9), 0)
    v = W.half_value(den)[0, 0] / W.lit(0.18)
    fit = (v * (v + W.lit(0.0245786)) - W.lit(0.000090537)) / (v * (W.lit(0.983729) * v + W.lit(0.4329510)) + W.lit(0.238081))
    assert np.allclose(o[0], fit, rtol=2e-4)       # the matrices' rows sum to 1 within their five digits
    assert np.array_equal(o, out)


# ------------------------------------------------------------------ B4: conditions on the inputs (not tolerances)
@pytest.mark.parametrize("kind,w,h", sorted({c[:3] for c in W.tone_cases()}))
def test_tone_inputs_meet_their_conditions(kind, w, h):
    t = W.tone_inputs(kind, w, h)
    o = t["o"]
    share = float((np.abs(o) < W.BAND).mean())
    print(f"tone inputs {kind} {w}x{h}: {share:.3%} of the channels inside the band")
    assert share <= W.BAND_SHARE_CAP
    assert not W.near_knee(o).any()
    if kind == "sweep":
        y = t["den"].reshape(-1, 4)[:, 0]
        assert set(range(0x7C00)) <= set(y.tolist())                       # every non-negative finite half is there
        assert np.all(np.diff(o.reshape(-1, 3)[:0x7C00], axis=0)[t["alb"].reshape(-1)[1:0x7C00] == t["alb"].reshape(-1)[:0x7C00 - 1]] >= 0)
        for knee in W.KNEES:                                                # the ramp passes every knee but the negative one
            if knee > 0:
                assert o.reshape(-1, 3)[:0x7C00].min() < knee < o.reshape(-1, 3)[:0x7C00].max()
    if w * h >= 16:
        assert t["special"].sum() == len(W.SPECIAL_TEXELS)
    if kind != "sweep" and w * h > 1000:
        a = t["alb"]
        for shift in (0, 10, 20):
            assert ((a >> shift) & 1023 == 0).any() and ((a >> shift) & 1023 == 1023).any()


@pytest.mark.parametrize("case", W.HIST_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_histogram_inputs_meet_their_conditions(case):
    kind, w, h, mn, mx, _, _ = case
    den = W.histogram_inputs(kind, w, h, mn, mx)
    assert W.mid_bin_ok(den, mn, mx - mn).all()
    # the same, spelled as the conditions read: fraction in [0.1, 0.9] unless clamped or below the floor; nothing next to the floor
    pos, below = W.histogram_position(den, mn, mx - mn)
    frac = np.mod(pos, 1.0)
    assert np.all(below | (pos == 1.0) | (pos == 255.0) | ((frac >= 0.1) & (frac <= 0.9)))
    assert np.all(np.abs(W.luminance(den) - W.LUM_FLOOR) > 1e-5)
    hist = W.histogram(den, mn, mx - mn)
    if kind == "bins" and w * h >= 256:
        assert np.all(hist >= 1)                  # one pixel per bin at least
    if kind == "floor":
        assert hist[0] == w * h
    if kind == "top":
        assert hist[255] == w * h


# ------------------------------------------------------------------ B1 - B3: the witness against the oracle
@pytest.mark.parametrize("kind,w,h,tf", W.tone_cases())
def test_tone_map_against_oracle(kind, w, h, tf):
    t = W.tone_inputs(kind, w, h)
    got = oracle_tone_map(t["den"], t["alb"], t["avg"], t["conv"], tf)
    worst, share = W.check_tone_map_output(got, t["o"], tf)
    print(f"oracle vs witness {kind} {w}x{h} tf {tf}: worst {worst} half steps outside the band, {share:.3%} inside")


@pytest.mark.parametrize("case", W.HIST_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_histogram_against_oracle(case):
    kind, w, h, mn, mx, _, _ = case
    den = W.histogram_inputs(kind, w, h, mn, mx)
    assert np.array_equal(W.histogram(den, mn, mx - mn), oracle_histogram(den, mn, mx))


def test_exposure_average_against_oracle():
    worst = 0.0
    for kind, w, h, mn, mx, tc, avg0 in W.HIST_CASES:
        hist = W.histogram(W.histogram_inputs(kind, w, h, mn, mx), mn, mx - mn)
        avg = avg0
        for call in range(2):   # the second call starts from the first's result, as the device's second call does
            scratch = hist.copy()
            got = float(O.lib().orc_exposure_average(_p(scratch), w, h, mn, mx - mn, tc, avg))
            want = W.exposure_average(hist, w * h, mn, mx - mn, tc, avg)
            dev = abs(got - want) / abs(want)
            print(f"exposure average {kind} {w}x{h} [{mn}, {mx}] tc {tc} from {avg}: witness {want:.9g} oracle {got:.9g} dev {dev:.2e}")
            worst = max(worst, dev)
            assert not scratch.any()
            avg = got
    print("worst relative deviation:", worst)
    assert worst <= W.EXPOSURE_ORACLE_DEV


def _pack32(rgb, hitdist):
    """nrd.glsl:127-147 in float32, one rounding per operation, dot products left to right"""
    F = np.float32
    r, g, b = (np.asarray(rgb[..., k], F) for k in range(3))
    y = ((r * F(0.25)).astype(F) + (g * F(0.5)).astype(F)).astype(F) + (b * F(0.25)).astype(F)
    co = ((r * F(0.5)).astype(F) + (g * F(0.0)).astype(F)).astype(F) + (b * F(-0.5)).astype(F)
    cg = ((r * F(-0.25)).astype(F) + (g * F(0.5)).astype(F)).astype(F) + (b * F(-0.25)).astype(F)
    hd = np.asarray(hitdist, F)
    hd = np.where(hd != 0, np.fmax(hd, F(1e-7)), hd).astype(F)
    with np.errstate(over="ignore"):
        return np.stack([y, co, cg, hd], axis=-1).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("w,h,frames", [s + (W.ACCUM_FRAMES,) for s in W.SIZES[:3]] + [W.SIZES[3] + (2,)])
def test_accumulate_inputs_and_bounds_in_float32(w, h, frames):
    """the bounds of the GPU test -- 2 f 2^-24 M on the mean, one half step on the packed mean -- held against a float32 restatement of
    the pass (acc += (r - acc) / (f + 1), then the pack), on the inputs the GPU test uploads"""
    t = W.accumulate_inputs(w, h, frames)
    assert np.isinf(t["depth"][t["miss"]]).all() and np.isfinite(t["depth"][~t["miss"]]).all()
    s32 = t["samples"].astype(np.float32)
    acc = np.zeros(s32.shape[1:], np.float32)
    worst = 0.0
    for f in range(1, frames + 1):
        acc = acc + (s32[f - 1] - acc) * (np.float32(1.0) / np.float32(f))
        full = np.concatenate([acc, np.full(acc.shape[:2] + (1,), f, np.float32)], axis=-1)
        den = np.where(t["miss"][..., None], t["denoised"][f - 1], _pack32(acc, W.half_value(t["illuminance"][f - 1][..., 3])))
        worst = max(worst, W.check_accumulate(full, den, t, f))
    print(f"accumulate {w}x{h}: float32 running mean within {worst:.3f} x 2^-24 M of the float64 mean")
    assert worst <= 2.0 * frames
