"""The numpy witness of the image passes that end a frame: the N-frame mean (k_accumulate), the auto exposure histogram and its average
(auto_exposure.comp:20-74, auto_exposure_avg.comp:19-53) and the tone map with its nine output transfer functions (tone_map.comp:39-220,
headers/color.glsl:1-23, headers/nrd.glsl:97-147). A helper module, not a test: tests/test_image_witness.py holds the C oracle to it on the
CPU, tests/test_gpu_image_passes.py the kernels on synthetic planes. Written from the shader text; binds neither library and shares no code
with oracle/ or csrc/.

Evaluation is float64 throughout. Every literal of the shaders is the float32 value of that literal, widened; a parameter that reaches the
shader as a float32 (the average luminance, the log range, the time coefficient, the conversion matrix) is rounded to float32 first.
Semantics fixed where GLSL leaves them open: max(x, 0) ignores a NaN operand (np.fmax, as fmaxf does), a comparison with NaN is false, and
pow, sqrt and log of a negative argument are NaN.

The module also makes the INPUTS both test files use, from fixed seeds, so that the CPU tests measure their margins on exactly what the GPU
tests upload. The inputs are built so that the witness and a correct float32 implementation cannot disagree about a branch:
  * tone map: no channel's pre-OETF value lies within a relative 2^-10 of a knee of a transfer function (a pixel that does is redrawn, or,
    in the sweep, gets the next grey albedo code), and few channels lie in the band |o| < 2^-12 where the ACES fit's numerator cancels;
  * histogram: every pixel is clearly below the luminance floor, clearly clamped to bin 1 or bin 255, or between 0.1 and 0.9 of the way
    through its bin (mid_bin_ok)."""
import functools

import numpy as np

F = np.float32


def lit(x):
    """a shader literal: its float32 value, as a float64"""
    return float(F(x))


SIZES = ((1, 1), (17, 3), (250, 131), (1024, 520))
BAND = 2.0 ** -12                      # |o| below this: the ACES fit's numerator cancels, relative error is unbounded
KNEE_GUARD = 2.0 ** -10                # no input within this relative distance of a knee
KNEES = (lit(0.0031308), -lit(0.0031308), lit(0.0030186), lit(0.0181), float(F(1.0) / F(12.0)))
BAND_SHARE_CAP = 0.05
LUM_FLOOR = lit(0.005)
FLOOR_GUARD = 1e-5
BIN_GUARD = 0.1                        # mid-bin inputs: fraction of the bin position in [0.1, 0.9]
# worst relative deviation of exposure_average from the C oracle's float32 evaluation over HIST_CASES, both calls of each
# (tests/test_image_witness.py::test_exposure_average_against_oracle measures it and holds it to this figure: 2.61e-7, at 1024x520 with
# one pixel per bin. It is float32's own: the weighted sum over the pixel count is a quotient near 128 whose rounding, 2^-24 x 128 bins,
# is 3e-7 of the luminance once scaled by range / 254 x ln 2, and the exp2 argument near 8 rounds by as much again.)
EXPOSURE_ORACLE_DEV = 2.7e-7
EXPOSURE_TOLERANCE = max(16.0 * EXPOSURE_ORACLE_DEV, 2.0 ** -21)

# GLSL mat3 constructors list COLUMNS; row i of the arrays below is output component i (color.glsl:8-23)
SRGB_TO_ACESCG = np.array([[0.6031065, 0.32633433, 0.047995567], [0.07011794, 0.9199162, 0.012763573],
                           [0.022178888, 0.11607823, 0.94101846]], F).astype(np.float64)
ACESCG_TO_SRGB = np.array([[1.7312546, -0.6040432, -0.08010775], [-0.131619, 1.1348418, -0.008679431],
                           [-0.024568284, -0.12575036, 1.0656371]], F).astype(np.float64)
# tone_map.comp:49-67: `v *= M` is v * M, component j the dot product with the j-th vec3 listed
RGB_TO_RRT = np.array([[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]], F).astype(np.float64)
ODT_TO_RGB = np.array([[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07602]], F).astype(np.float64)
LUMA = np.array([0.299, 0.587, 0.114], F).astype(np.float64)


# ------------------------------------------------------------------ fp16 bit patterns
def to_half(x):
    """float64 -> fp16 bit patterns, one rounding to nearest even (overflow to infinity)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def half_value(u):
    return np.ascontiguousarray(u, np.uint16).view(np.float16).astype(np.float64)


def half_is_nan(u):
    return (np.asarray(u, np.uint16) & 0x7FFF) > 0x7C00


def half_ordinal(u):
    """fp16 bit patterns on one integer line: consecutive representable values differ by 1, +0 and -0 are both 0, the infinities are
    the step after the largest finite values. NaN patterns have no place on it: mask them first."""
    v = np.asarray(u, np.uint16).astype(np.int32)
    mag = v & 0x7FFF
    return np.where(v & 0x8000, -mag, mag)


def half_steps(a, b):
    return np.abs(half_ordinal(a) - half_ordinal(b))


# ------------------------------------------------------------------ nrd.glsl:97-147
def unpack_radiance(half4):
    """(..., 4) fp16 bit patterns (Y, Co, Cg, hit distance) -> (rgb (..., 3), hit distance (...)), float64"""
    f = half_value(half4)
    with np.errstate(invalid="ignore"):
        t = f[..., 0] - f[..., 2]
        rgb = np.stack([t + f[..., 1], f[..., 0] + f[..., 2], t - f[..., 1]], axis=-1)
    return np.fmax(rgb, 0.0), f[..., 3]


def pack_radiance(rgb, hitdist):
    """REBLUR_FrontEnd_PackRadianceAndNormHitDist stored to an RGBA16F image: (..., 4) fp16 bit patterns"""
    rgb, hd = np.asarray(rgb, np.float64), np.asarray(hitdist, np.float64)
    hd = np.where(hd != 0, np.fmax(hd, lit(1e-7)), hd)
    y = rgb[..., 0] * 0.25 + rgb[..., 1] * 0.5 + rgb[..., 2] * 0.25
    co = rgb[..., 0] * 0.5 + rgb[..., 2] * -0.5
    cg = rgb[..., 0] * -0.25 + rgb[..., 1] * 0.5 + rgb[..., 2] * -0.25
    return to_half(np.stack([y, co, cg, hd], axis=-1))


# ------------------------------------------------------------------ the N-frame mean
def accumulate(samples):
    """samples (frames, ..., 3) -> (frames, ..., 3): entry f - 1 is the plain mean of the first f samples"""
    s = np.asarray(samples, np.float64)
    n = np.arange(1, s.shape[0] + 1, dtype=np.float64).reshape((-1,) + (1,) * (s.ndim - 1))
    return np.cumsum(s, axis=0) / n


# ------------------------------------------------------------------ auto_exposure.comp:20-74
def luminance(half4):
    rgb, _ = unpack_radiance(half4)
    with np.errstate(invalid="ignore"):
        return rgb @ LUMA


def histogram_position(half4, min_log, log_range):
    """-> (position, below): the real-valued bin position clamp((log2(lum) - min) / range, 0, 1) * 254 + 1 -- the bin is its floor -- and
    whether lum < 0.005, which sends the pixel to bin 0 whatever its position"""
    lum = luminance(half4)
    mn, rg = lit(min_log), lit(log_range)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.log2(lum) - mn) * (1.0 / rg)
    return np.clip(t, 0.0, 1.0) * 254.0 + 1.0, lum < LUM_FLOOR


def histogram(half4, min_log, log_range):
    pos, below = histogram_position(half4, min_log, log_range)
    bins = np.where(below, 0, np.floor(pos)).astype(np.int64)
    return np.bincount(bins.reshape(-1), minlength=256).astype(np.uint32)


def mid_bin_ok(half4, min_log, log_range):
    """the input condition of the histogram tests, per pixel: no float32 implementation can put the pixel into another bin"""
    lum = luminance(half4)
    mn, rg = lit(min_log), lit(log_range)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.log2(lum) - mn) * (1.0 / rg)
    frac = np.mod(np.clip(t, 0.0, 1.0) * 254.0 + 1.0, 1.0)
    clear_of_floor = np.abs(lum - LUM_FLOOR) > FLOOR_GUARD
    below = lum < LUM_FLOOR
    clamped = (t <= -BIN_GUARD / 254.0) | (t >= 1.0 + BIN_GUARD / 254.0)
    inside = (t > 0.0) & (t < 1.0) & (frac >= BIN_GUARD) & (frac <= 1.0 - BIN_GUARD)
    return clear_of_floor & (below | clamped | inside)


# ------------------------------------------------------------------ auto_exposure_avg.comp:19-53
def exposure_average(hist, n_pixels, min_log, log_range, time_coeff, avg_before):
    weighted = int(sum(int(c) * i for i, c in enumerate(np.asarray(hist).reshape(256)))) & 0xFFFFFFFF   # uint arithmetic
    log_avg = weighted / max(float(n_pixels), 1.0) - 1.0
    lum = 2.0 ** ((log_avg / 254.0) * lit(log_range) + lit(min_log))
    last = lit(avg_before)
    return last + (lum - last) * lit(time_coeff)


# ------------------------------------------------------------------ tone_map.comp:39-220
def albedo_linear(albedo):
    """A2B10G10R10 texels -> linear rgb (color.glsl:1-5): x is the low ten bits"""
    a = np.asarray(albedo, np.uint32)
    c = np.stack([a & 1023, (a >> 10) & 1023, (a >> 20) & 1023], axis=-1).astype(np.float64) / 1023.0
    return np.where(c < lit(0.04045), c / lit(12.92), np.power(np.abs(c + lit(0.055)) / lit(1.055), lit(2.4)))


def tone_map_linear(half4, albedo, avg, conv):
    """the pre-OETF value `o` per channel (..., 3): radiance x albedo x exposure -> display primaries -> ACES fit"""
    rgb, _ = unpack_radiance(half4)
    conv = np.asarray(conv, F).astype(np.float64).reshape(3, 3).T   # nine constants, column-major
    exposure = 1.0 / lit(avg)                                        # 1 / (9.6 avg) * 9.6
    with np.errstate(invalid="ignore", over="ignore"):
        s = rgb @ ACESCG_TO_SRGB.T
        m = ((s * albedo_linear(albedo)) @ SRGB_TO_ACESCG.T) * exposure
        v = (m @ conv.T) @ RGB_TO_RRT.T
        a = v * (v + lit(0.0245786)) - lit(0.000090537)
        b = v * (lit(0.983729) * v + lit(0.4329510)) + lit(0.238081)
        return (a / b) @ ODT_TO_RGB.T


def oetf(tf, c):
    """SwapchainOETF (tone_map.comp:72-161) of transfer function 0..8"""
    c = np.asarray(c, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        def srgb_upper(x):
            return lit(1.055) * np.power(x, 1.0 / lit(2.4)) - lit(0.055)
        if tf == 1:
            return np.where(c <= lit(0.0031308), lit(12.92) * c, srgb_upper(c))
        if tf == 2:
            return np.where(c <= -lit(0.0031308), -lit(1.055) * np.power(-c, 1.0 / lit(2.4)) + lit(0.055),
                            np.where(c <= lit(0.0031308), lit(12.92) * c, srgb_upper(c)))
        if tf == 3:
            return np.power(c / lit(52.37), 1.0 / lit(2.6))
        if tf == 4:
            return np.where(c < lit(0.0030186), lit(12.92) * c, srgb_upper(c))
        if tf == 5:
            return np.where(c < lit(0.0181), lit(4.5) * c, lit(1.0993) * np.power(c, lit(0.45)) - (lit(1.0993) - 1.0))
        if tf == 6:
            m1, m2 = 2610.0 / 16384.0, (2523.0 / 4096.0) * 128.0
            c2, c3 = (2413.0 / 4096.0) * 32.0, (2392.0 / 4096.0) * 32.0
            c1 = c3 - c2 + 1.0
            lm = np.power(c, m1)
            return np.power((c1 + c2 * lm) / (1.0 + c3 * lm), m2)
        if tf == 7:
            a, cc = lit(0.17883277), lit(0.55991073)
            return np.where(c < KNEES[4], np.sqrt(3.0 * c), a * np.log(12.0 * c - (1.0 - 4.0 * a)) + cc)
        if tf == 8:
            return np.power(c, 256.0 / 563.0)
        if tf == 0:
            return c.copy()
    raise ValueError("transfer function must be 0..8")


def tone_map(half4, albedo, avg, conv, tf):
    """-> (o, oetf(tf, o)), each (..., 3) float64"""
    o = tone_map_linear(half4, albedo, avg, conv)
    return o, oetf(tf, o)


def near_knee(o, guard=KNEE_GUARD):
    """per pixel: some channel lies within a relative `guard` of a knee of some transfer function"""
    hit = np.zeros(o.shape[:-1], bool)
    for k in KNEES:
        hit |= (np.abs(o - k) <= guard * abs(k)).any(axis=-1)
    return hit


def band_limit(tf):
    """what a finite output may reach in magnitude where |o| < BAND: every transfer function is monotone there and largest at +BAND"""
    return float(oetf(tf, np.float64(BAND)))


def check_tone_map_output(got, o, tf):
    """The per-channel comparison both test files make. got: (..., 4) fp16 bit patterns; o: the witness's pre-OETF values.
    -> (worst deviation in half steps outside the band, share of channels inside the band). Raises AssertionError."""
    got = np.asarray(got, np.uint16)
    want = oetf(tf, o)
    assert np.all(got[..., 3] == 0x3C00), "alpha is not 1.0"
    rgb = got[..., :3]
    # a NaN `o` is outside the band: it is NaN on every side
    inside = np.abs(o) < BAND
    want_half = to_half(want)
    got_nan, want_nan = half_is_nan(rgb), np.isnan(want)
    out = ~inside
    assert np.array_equal(got_nan[out], want_nan[out]), f"NaN positions differ at {np.argwhere(out & (got_nan != want_nan))[:5].tolist()}"
    cmp = out & ~want_nan
    steps = half_steps(rgb[cmp], want_half[cmp])
    worst = int(steps.max()) if steps.size else 0
    if worst > 1:
        at = np.argwhere(cmp)[np.argmax(steps)]
        raise AssertionError(f"tf {tf}: {worst} half steps at {at.tolist()}: got {half_value(rgb[tuple(at)])}, witness {want[tuple(at)]}, o {o[tuple(at)]}")
    # inside the band: NaN, or no larger than the transfer function at the band's edge plus one step
    fin = inside & ~got_nan
    limit = half_ordinal(to_half(band_limit(tf))) + 1
    assert np.all(np.abs(half_ordinal(rgb[fin])) <= limit), f"tf {tf}: a value inside the band exceeds oetf(2^-12) + 1 step"
    share = float(inside.mean())
    assert share <= BAND_SHARE_CAP, f"tf {tf}: {share:.3%} of the channels lie inside the band"
    return worst, share


# ------------------------------------------------------------------ inputs
def default_conversion():
    """ACES AP1 -> BT.709 as dust_amd.api.color_space_conversion() gives it (imported late: the witness functions need nothing of the package)"""
    from dust_amd import api
    return np.asarray(api.color_space_conversion(), np.float32)


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def random_radiance(rng, n, log2_lo, log2_hi, chroma=0.3, hitdist=100.0):
    """n packed texels: luminance log-uniform over 2^lo .. 2^hi, chroma up to +-chroma Y (every channel stays positive for chroma < 0.5)"""
    y = 2.0 ** rng.uniform(log2_lo, log2_hi, n)
    co, cg = y * rng.uniform(-chroma, chroma, n), y * rng.uniform(-chroma, chroma, n)
    return to_half(np.stack([y, co, cg, rng.uniform(0.0, hitdist, n)], axis=1))


def random_albedo(rng, n):
    """30 random bits per texel (and two of alpha, which nothing reads); each channel is code point 0 in a tenth of the texels and
    code point 1023 in another tenth"""
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for shift in (0, 10, 20):
        pick = rng.uniform(size=n)
        a = np.where(pick < 0.1, a & ~np.uint32(1023 << shift), a)
        a = np.where(pick > 0.9, a | np.uint32(1023 << shift), a)
    return a.astype(np.uint32)


def grey_albedo(code):
    code = np.asarray(code, np.uint32)
    return (code | (code << 10) | (code << 20) | np.uint32(3 << 30)).astype(np.uint32)


# texels no ray tracer hands over on purpose: the witness says what each becomes
SPECIAL_TEXELS = np.array([[0x7E00, 0, 0, 0],            # Y NaN: every channel NaN, max(., 0) makes it black
                           [0x7C00, 0, 0, 0],            # Y +inf: inf - inf in the first matrix, NaN out
                           [0xBC00, 0, 0, 0],            # Y -1: clamped to black
                           [0xFBFF, 0, 0, 0x3C00],       # Y -65504
                           [0x8000, 0, 0, 0],            # Y -0
                           [0x3C00, 0x7E00, 0, 0],       # Co NaN: red and blue black, green survives
                           [0x3800, 0, 0xB800, 0],       # Cg = -Y: green exactly 0
                           [0x0000, 0, 0, 0]], np.uint16)  # black


def special_positions(n):
    return np.unique(np.linspace(2, n - 2, len(SPECIAL_TEXELS)).astype(np.int64)) if n >= 16 else np.zeros(0, np.int64)


TONE_AVG = 0.37
SWEEP_AVG = 0.006   # the sweep's zero crossing of the ACES fit falls among the subnormal halves, where values are sparse: see tone_inputs
TONE_KINDS = ("sweep", "random", "identity")


@functools.lru_cache(maxsize=None)
def tone_inputs(kind, w, h):
    """-> dict(den (h, w, 4) uint16, alb (h, w) uint32, avg, conv (9,) float32, o (h, w, 3) float64: the witness's pre-OETF values)
    sweep (250x131 only): every non-negative finite half once as Y, Co = Cg = 0, grey albedo -- a monotone ramp through every segment of
      every transfer function. The band |o| < 2^-12 spans two octaves of Y wherever it falls (4.03x between the fit's -2^-12 and
      +2^-12), 2059 normal halves: 6.3 % of the frame. The average luminance is therefore chosen so that the band falls on Y below
      2^-15, where halves are subnormal and 385 of them span it. The 1006 texels left over are random colours and the special texels.
    random: luminance log-uniform over 2^-6 .. 2^8, chroma up to +-0.3 Y, random albedo with code points 0 and 1023, the default
      conversion, the special texels (frames of 16 pixels and more).
    identity: the same recipe from another seed, through the identity conversion."""
    n = w * h
    rng = np.random.default_rng([{"sweep": 11, "random": 12, "identity": 13}[kind], w, h])
    conv = np.eye(3, dtype=np.float32).reshape(9) if kind == "identity" else default_conversion()
    if kind == "sweep":
        assert n >= 0x7C00 + 64
        avg = SWEEP_AVG
        den = random_radiance(rng, n, -6.0, 8.0)
        den[:0x7C00] = 0
        den[:0x7C00, 0] = np.arange(0x7C00, dtype=np.uint16)
        code = np.full(n, 1023, np.uint32)
        sp = 0x7C00 + special_positions(n - 0x7C00)
    else:
        avg = TONE_AVG
        den = random_radiance(rng, n, -6.0, 8.0)
        alb = random_albedo(rng, n)
        sp = special_positions(n)
    den[sp] = SPECIAL_TEXELS[:len(sp)]
    special = np.zeros(n, bool)
    special[sp] = True
    for _ in range(64):   # the knee condition: move whatever lies next to a knee (with twice the guard the tests assert)
        if kind == "sweep":
            alb = grey_albedo(code)
        o = tone_map_linear(den, alb, avg, conv)
        bad = near_knee(o, 2.0 * KNEE_GUARD)
        if not bad.any():
            break
        if kind == "sweep":
            code[bad] -= 1
        else:
            k = int((bad & ~special).sum())
            assert not (bad & special).any()
            den[bad] = random_radiance(rng, k, -6.0, 8.0)
            alb[bad] = random_albedo(rng, k)
    else:
        raise AssertionError("could not move the inputs away from the knees")
    return _frozen(den=den.reshape(h, w, 4), alb=alb.reshape(h, w), avg=avg, conv=conv, o=o.reshape(h, w, 3), special=special.reshape(h, w))


def tone_cases():
    """(kind, w, h, tf): every transfer function at the three small sizes, one at the size that needs a second grid-stride trip"""
    cases = []
    for (w, h), kinds in (((1, 1), ("random",)), ((17, 3), ("random",)), ((250, 131), TONE_KINDS)):
        cases += [(kind, w, h, tf) for kind in kinds for tf in range(9)]
    return cases + [("random", 1024, 520, 1)]


# (kind, w, h, min_log, max_log, time coefficient, starting average). A starting average far above the frame's luminance is paired with
# the small time coefficient only: avg + (lum - avg) * 1.0 cancels, and what is left of a float32 result is noise of relative size
# 2^-24 avg / lum on every side, which says nothing about the histogram.
HIST_CASES = (
    ("floor", 17, 3, -6.0, 8.5, 0.2, 0.37), ("floor", 1, 1, -6.0, 8.5, 1.0, 0.0),
    ("top", 17, 3, -6.0, 8.5, 1.0, 50.0), ("top", 250, 131, -6.0, 8.5, 0.2, 0.0),
    ("bins", 17, 3, -3.0, 5.25, 1.0, 0.0), ("bins", 250, 131, -6.0, 8.5, 0.2, 0.37), ("bins", 1024, 520, -6.0, 8.5, 1.0, 0.0),
    ("random", 1, 1, -6.0, 8.5, 0.2, 0.0), ("random", 1, 1, -6.0, 8.5, 0.2, 50.0), ("random", 17, 3, -6.0, 8.5, 0.2, 50.0),
    ("random", 17, 3, -6.0, 8.5, 1.0, 0.0), ("random", 250, 131, -3.0, 5.25, 0.2, 0.37), ("random", 250, 131, -10.0, 2.0, 1.0, 0.0),
    ("random", 1024, 520, -6.0, 8.5, 0.2, 0.37),
)


@functools.lru_cache(maxsize=None)
def histogram_inputs(kind, w, h, min_log, max_log):
    """-> (h, w, 4) uint16 texels, every one of which satisfies mid_bin_ok.
    floor: all below luminance 0.005 (bin 0). top: all +inf (bin 255). bins: texel i aims at the middle of bin i mod 256 -- one pixel
    per bin where the frame has 256 pixels -- and the rest are random. random: colours over more than the whole range, kept where they
    satisfy the condition; one texel in 32 is NaN (black after max(., 0): bin 0)."""
    n, log_range = w * h, max_log - min_log
    rng = np.random.default_rng([{"floor": 21, "top": 22, "bins": 23, "random": 24}[kind], w, h, int(min_log * 4) + 100])
    den = np.zeros((n, 4), np.uint16)
    if kind == "floor":
        den[:, 0] = to_half(2.0 ** rng.uniform(-20.0, -8.0, n))
    elif kind == "top":
        den[:, 0] = 0x7C00
    else:
        filled = 0
        while filled < n:
            cand = random_radiance(rng, 2 * (n - filled) + 16, max(min_log - 4.0, -20.0), min(max_log + 2.0, 15.9))
            cand = cand[mid_bin_ok(cand, min_log, log_range)][:n - filled]
            den[filled:filled + len(cand)] = cand
            filled += len(cand)
        nan = np.flatnonzero(rng.uniform(size=n) < 1.0 / 32.0)
        den[nan] = np.array([0x7E00, 0x7E00, 0xFE00, 0x7E00], np.uint16)
        if kind == "bins":
            m = min(n, 256)
            b = np.arange(m, dtype=np.float64)
            lum = 2.0 ** ((b + 0.5 - 1.0) / 254.0 * lit(log_range) + lit(min_log))
            lum[0] = 0.001
            den[:m] = 0
            den[:m, 0] = to_half(lum)
    assert mid_bin_ok(den, min_log, log_range).all()
    return _frozen(den=den.reshape(h, w, 4))["den"]


ACCUM_FRAMES = 5


@functools.lru_cache(maxsize=None)
def accumulate_inputs(w, h, frames=ACCUM_FRAMES):
    """-> dict(depth (h, w) float32: +inf on a checkerboard of miss pixels; illuminance, denoised (frames, h, w, 4) uint16; samples
    (frames, h, w, 3) float64: what the witness says the kernel averages -- the unpacked illuminance at hit pixels, the unpacked
    denoised plane (where miss.rmiss left the sky) at miss pixels.
    Samples are finite, over the whole fp16 range, subnormals included, with chroma that cannot cancel (below); a tenth of the hit
    texels are black in every frame and another tenth have negative Y (black after the clamp) in some. The hit distance is 0, the smallest subnormal (below NRD_FP16_MIN), or
    anything up to the largest half. Hit pixels of the denoised plane carry NaN: the pass has to replace them."""
    n = w * h
    rng = np.random.default_rng([31, w, h])
    yy, xx = np.mgrid[0:h, 0:w]
    miss = ((xx + yy) & 1) == 1
    depth = np.where(miss, np.inf, rng.uniform(0.5, 500.0, (h, w))).astype(np.float32)
    black = rng.uniform(size=n) < 0.1
    # Chroma: each pixel keeps the sign of its Co and of its Cg through all frames, a magnitude of 0.05 .. 0.3 Y, or is grey throughout.
    # The pass packs its mean as float32 dot products, and Cg = (-0.25 r + 0.5 g) - 0.25 b is rounded at the size of g before the last
    # term cancels: 2^-25 g absolute, more than a half step of Cg once |Cg| < 2^-13 g. A mean whose chroma is 0.05 of its luminance or
    # exactly 0 keeps the witness's float64 pack and any float32 pack within the one step of the double rounding.
    sign = rng.choice([-1.0, 1.0], (n, 2)) * (rng.uniform(size=(n, 1)) >= 0.1)
    ill = np.zeros((frames, n, 4), np.uint16)
    den = np.zeros((frames, n, 4), np.uint16)
    for f in range(frames):
        y = 2.0 ** rng.uniform(-24.0, 15.99, n)
        chroma = sign * rng.uniform(0.05, 0.3, (n, 2)) * y[:, None]
        t = to_half(np.stack([y, chroma[:, 0], chroma[:, 1], y], axis=1))
        t[black] = 0
        neg = rng.uniform(size=n) < 0.1
        t[neg, 0] |= 0x8000
        pick = rng.uniform(size=n)
        t[:, 3] = np.where(pick < 0.2, 0, np.where(pick < 0.4, 1, to_half(2.0 ** rng.uniform(-20.0, 15.99, n))))
        ill[f] = t
        sky = random_radiance(rng, n, -3.0, 4.0)
        sky[:, 3] = 0x7C00
        den[f] = np.where(miss.reshape(n, 1), sky, np.uint16(0x7E00))
    ill, den = ill.reshape(frames, h, w, 4), den.reshape(frames, h, w, 4)
    samples = np.where(miss[None, :, :, None], unpack_radiance(den)[0], unpack_radiance(ill)[0])
    assert np.isfinite(samples).all()
    return _frozen(depth=depth, miss=miss, illuminance=ill, denoised=den, samples=samples)


def check_accumulate(acc, den_after, inputs, f, rows=None):
    """The D3 comparison after frame f (1-based) of a run over inputs' frames 0 .. f - 1, restricted to rows [rows[0], rows[1]).
    acc: (h, w, 4) float32 ACCUM as read back; den_after: (h, w, 4) uint16 DENOISED as read back.
    -> the largest error of the mean in units of 2^-24 M. Raises AssertionError."""
    r0, r1 = rows if rows else (0, acc.shape[0])
    sl = slice(r0, r1)
    s = inputs["samples"][:f, sl]
    miss = inputs["miss"][sl]
    a = np.asarray(acc[sl], np.float32)
    assert np.all(a[..., 3] == np.float32(f)), "frame count"
    assert np.isfinite(a).all(), "the accumulator still holds what it was pre-filled with"
    mean = accumulate(s)[-1]
    big = np.abs(s).max(axis=(0, -1))            # M: the pixel's largest sample magnitude so far
    err = np.abs(a[..., :3].astype(np.float64) - mean).max(axis=-1)
    assert np.all(err[big == 0] == 0), "a pixel whose samples are all 0 is exactly 0"
    bound = 2.0 * f * 2.0 ** -24 * big
    assert np.all(err <= bound), f"mean off by {float((err / np.maximum(bound, 1e-300)).max()):.3f} of its bound"
    # the denoised plane: untouched on miss pixels, the packed accumulator on hit pixels
    d = np.asarray(den_after[sl], np.uint16)
    assert np.array_equal(d[miss], inputs["denoised"][f - 1, sl][miss]), "a miss pixel's denoised texel changed"
    hit = ~miss
    hitdist = half_value(inputs["illuminance"][f - 1, sl][..., 3])
    want = pack_radiance(a[..., :3].astype(np.float64), hitdist)
    assert not half_is_nan(d[hit]).any()
    assert np.all(half_steps(d[hit][:, :3], want[hit][:, :3]) <= 1), "denoised is not the packed accumulator"
    assert np.array_equal(d[hit][:, 3], want[hit][:, 3]), "hit distance"
    nz = big > 0
    return float((err[nz] / (2.0 ** -24 * big[nz])).max()) if nz.any() else 0.0
