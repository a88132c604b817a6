"""The image passes that end every frame -- k_accumulate, k_exposure_histogram, k_exposure_average, k_tone_map (dust_amd/csrc/kernels.hip)
-- driven with synthetic planes and checked pixel by pixel against the float64 witness (tests/image_witness.py). No rays: the planes
are written with hipMemcpy (tests/device_planes.py), the adaptation state with Pipeline.exposure(set_to=...), and an empty scene with
PASS_ACCUMULATE alone runs k_accumulate and nothing else. tests/test_image_witness.py holds the witness to the C oracle on the same
inputs and checks the conditions the inputs meet.

Frame sizes: 1x1 (one thread of one workgroup works), 17x3 (less than a workgroup, odd pitch), 250x131 (room for every non-negative
finite half; nothing a multiple of anything), 1024x520 (532 480 pixels: the second grid-stride trip of the 2048x256 and 1024x256 launches).

Tolerances.
  Tone map: one half-precision step per channel from the fp16 rounding of the witness wherever |o| >= 2^-12 (o: the value before the
    transfer function), NaN exactly where the witness is NaN. The float32 chain is three orders of magnitude finer than a half step; the
    one step is the double rounding. Inside the band the ACES fit's numerator cancels: NaN, or at most oetf(2^-12) plus a step. The
    inputs keep at most 5 % of the channels in the band (measured: sweep 1.2 %, random 2.4 %, identity 2.6 %).
  Exposure: EXPOSURE_ORACLE_DEV = 2.7e-7 is the worst relative deviation of the C oracle's float32 evaluation from the witness over
    HIST_CASES (measured 2.61e-7); the device gets max(16 x that, 2^-21) = 4.32e-6, 16 x because its log2 and exp2 are 1-ulp hardware
    instructions where glibc's are nearly correctly rounded. Sensitivity: one pixel of 51 in the next bin moves the average by
    1 / 51 / 254 x 14.5 x ln 2 = 0.08 %, 180 times the tolerance; a multiplier of 255 for 254 moves every pixel by up to a bin. (A single
    pixel of 32 750 would move it by 1.2e-6: the large frames test the reduction, the small ones the binning.)
  Accumulate: 2 f 2^-24 M from the float64 mean after f frames, M the pixel's largest sample so far: each step rounds three times,
    each time by at most 2^-24 M. A float32 restatement measures 1.1 x 2^-24 M after five frames."""
import numpy as np
import pytest

import device_planes as D
import image_witness as W
import parity_util as P
from dust_amd import _lib as L
from dust_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(device=0)


@pytest.fixture(scope="module")
def pipes(ctx):
    """one pipeline per frame size for the passes that keep no state of their own between calls"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = api.StandardPipeline(ctx, w, h)
        return made[(w, h)]
    return get


def _ids(c):
    return "-".join(str(v) for v in c)


# ------------------------------------------------------------------ D1: tone map, per pixel
@pytest.mark.parametrize("kind,w,h,tf", W.tone_cases())
def test_tone_map_per_pixel(pipes, kind, w, h, tf):
    t = W.tone_inputs(kind, w, h)
    pipe = pipes(w, h)
    D.upload(pipe, L.PLANE_DENOISED, t["den"])
    D.upload(pipe, L.PLANE_ALBEDO, t["alb"])
    D.upload(pipe, L.PLANE_OUTPUT, np.full((h, w, 4), 0xFFFF, np.uint16))   # a texel the pass does not write shows
    avg = pipe.exposure(set_to=t["avg"])
    pipe.tone_map(transfer_function=tf, conversion=t["conv"], time_coefficient=0.0)
    assert pipe.exposure() == avg == np.float32(t["avg"])   # time coefficient 0: the pixel check does not depend on the histogram
    got = D.download(pipe, L.PLANE_OUTPUT)
    assert np.array_equal(got, pipe.read_plane(L.PLANE_OUTPUT))
    worst, share = W.check_tone_map_output(got, t["o"], tf)
    print(f"tone map {kind} {w}x{h} tf {tf}: worst {worst} half steps outside the band, {share:.3%} inside")
    # the inputs are the pass's to read only
    assert np.array_equal(D.download(pipe, L.PLANE_DENOISED), t["den"]) and np.array_equal(D.download(pipe, L.PLANE_ALBEDO), t["alb"])


# ------------------------------------------------------------------ D2: histogram and average, through the adapted average
@pytest.mark.parametrize("case", W.HIST_CASES, ids=_ids)
def test_exposure_histogram_and_average(pipes, case):
    kind, w, h, mn, mx, tc, avg0 = case
    den = W.histogram_inputs(kind, w, h, mn, mx)
    hist = W.histogram(den, mn, mx - mn)
    pipe = pipes(w, h)
    D.upload(pipe, L.PLANE_DENOISED, den)
    avg = pipe.exposure(set_to=avg0)
    for call in (1, 2):   # k_exposure_average clears the histogram: the second call follows from the first's result, not from doubled counts
        pipe.tone_map(transfer_function=0, min_log=mn, max_log=mx, time_coefficient=tc)
        got = pipe.exposure()
        want = W.exposure_average(hist, w * h, mn, mx - mn, tc, avg)
        dev = abs(got - want) / abs(want)
        print(f"exposure {_ids(case)} call {call}: device {got:.9g} witness {want:.9g} dev {dev:.2e} (tolerance {W.EXPOSURE_TOLERANCE:.2e})")
        assert dev <= W.EXPOSURE_TOLERANCE, (call, got, want, dev)
        avg = got
    if kind == "floor":   # every pixel in bin 0: the luminance the average heads for is 2^(min - range / 254)
        assert np.isclose(W.exposure_average(hist, w * h, mn, mx - mn, 1.0, 0.0), 2.0 ** (mn - (mx - mn) / 254.0), rtol=1e-12)


# ------------------------------------------------------------------ D3: the N-frame mean
def _accumulate_setup(ctx, w, h, frames=W.ACCUM_FRAMES):
    t = W.accumulate_inputs(w, h, frames)
    pipe = api.StandardPipeline(ctx, w, h)   # a fresh one: the frame count is the pipeline's
    scene = D.empty_scene(ctx)
    return t, pipe, scene, P.camera_for((30.0, 20.0, -40.0)), P.sky_state()


def _accumulate_frame(pipe, scene, cam, sky, t, k, frame_index, rows=(0, 0)):
    """inputs' frame k (0-based) through one PASS_ACCUMULATE step -> (ACCUM, DENOISED) as read back"""
    D.upload(pipe, L.PLANE_ILLUMINANCE, t["illuminance"][k])
    D.upload(pipe, L.PLANE_DENOISED, t["denoised"][k])
    pipe.render(scene, cam, sky, L.PASS_ACCUMULATE, frame_index=frame_index, rows=rows)
    return D.download(pipe, L.PLANE_ACCUM), D.download(pipe, L.PLANE_DENOISED)


@pytest.mark.parametrize("w,h", W.SIZES[:3])
def test_accumulate_running_mean(ctx, w, h):
    t, pipe, scene, cam, sky = _accumulate_setup(ctx, w, h)
    nan_fill = np.full((h, w, 4), np.nan, np.float32)
    D.upload(pipe, L.PLANE_DEPTH, t["depth"])
    D.upload(pipe, L.PLANE_ACCUM, nan_fill)
    worst = 0.0
    for f in range(1, W.ACCUM_FRAMES + 1):
        acc, den = _accumulate_frame(pipe, scene, cam, sky, t, f - 1, f)
        worst = max(worst, W.check_accumulate(acc, den, t, f))
    print(f"accumulate {w}x{h}: worst error of the mean {worst:.3f} x 2^-24 M over {W.ACCUM_FRAMES} frames")
    # clear() restarts the count (and zeroes the planes: they are written again)
    pipe.clear()
    D.upload(pipe, L.PLANE_DEPTH, t["depth"])
    D.upload(pipe, L.PLANE_ACCUM, nan_fill)
    acc, den = _accumulate_frame(pipe, scene, cam, sky, t, 0, 6)
    W.check_accumulate(acc, den, t, 1)


@pytest.mark.parametrize("w,h,rows", [(17, 3, (1, 2)), (1024, 520, (130, 391))])
def test_accumulate_row_band(ctx, w, h, rows):
    t, pipe, scene, cam, sky = _accumulate_setup(ctx, w, h, frames=2)
    rng = np.random.default_rng([41, w, h])
    before = rng.uniform(-4.0, 4.0, (h, w, 4)).astype(np.float32)
    before[::2, ::3] = np.nan
    D.upload(pipe, L.PLANE_DEPTH, t["depth"])
    D.upload(pipe, L.PLANE_ACCUM, before)
    outside = np.ones(h, bool)
    outside[rows[0]:rows[1]] = False
    for f in (1, 2):
        acc, den = _accumulate_frame(pipe, scene, cam, sky, t, f - 1, f, rows=rows)
        assert np.array_equal(acc[outside].view(np.uint32), before[outside].view(np.uint32))         # byte for byte, the NaNs included
        assert np.array_equal(den[outside], t["denoised"][f - 1][outside])
        W.check_accumulate(acc, den, t, f, rows=rows)


def test_accumulate_second_grid_stride_trip(ctx):
    w, h = W.SIZES[3]
    t, pipe, scene, cam, sky = _accumulate_setup(ctx, w, h, frames=2)
    D.upload(pipe, L.PLANE_DEPTH, t["depth"])
    D.upload(pipe, L.PLANE_ACCUM, np.full((h, w, 4), np.nan, np.float32))
    acc, den = _accumulate_frame(pipe, scene, cam, sky, t, 0, 1)
    worst = W.check_accumulate(acc, den, t, 1)
    print(f"accumulate {w}x{h}: one whole-frame step, worst error {worst:.3f} x 2^-24 M")


# ------------------------------------------------------------------ D4: error paths
def test_tone_map_argument_checks(pipes):
    pipe = pipes(17, 3)
    with pytest.raises(L.DustError) as e:
        pipe.tone_map(transfer_function=9)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    for mn, mx in ((2.0, 2.0), (3.0, -3.0)):
        with pytest.raises(L.DustError) as e:
            pipe.tone_map(min_log=mn, max_log=mx)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
