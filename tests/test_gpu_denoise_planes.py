"""k_denoise_temporal and k_denoise_spatial (dust_amd/csrc/denoise.hip) on synthetic planes, pixel by pixel. No rays: the planes of the
cases of tests/denoise_witness.py are written with hipMemcpy (tests/device_planes.py) and PASS_DENOISE on an empty scene runs the two
kernels and nothing else. While PLANE_ACCUM is not bound it is the buffer the next frame reads its radiance history from, so the history
and the frame counts are whatever the test uploads; the history's geometry is what the previous pass wrote from the previous planes.

Two judges. oracle/denoise.c, value for value at every pixel: the record of the ray-traced sequences says the device and the oracle
agree exactly, and these planes hold them to it on the branches that sequence does not reach. And the float64 witness, through the same
check functions and the same bound (denoise_witness.DENOISE_ORACLE_DEV, one half step on the packed plane) that
tests/test_denoise_witness.py holds the oracle to: written from the filter's description, it is the judge of a misreading the kernels
and the oracle could share."""
import numpy as np
import pytest

import denoise_witness as W
import device_planes as D
import oracle_lib as O
import parity_util as P
from dust_amd import _lib as L
from dust_amd import api

pytestmark = pytest.mark.gpu
INPUT_PLANES = (("illuminance", L.PLANE_ILLUMINANCE), ("normal", L.PLANE_NORMAL), ("depth", L.PLANE_DEPTH), ("motion", L.PLANE_MOTION),
                ("voxel_id", L.PLANE_VOXEL_ID))


@pytest.fixture(scope="module")
def ctx():
    return api.Context(device=0)


@pytest.fixture(scope="module")
def world(ctx):
    return D.empty_scene(ctx), P.sky_state()


def make_pipe(ctx, w, h, par):
    pipe = api.StandardPipeline(ctx, w, h)
    pipe.set_denoiser(max_accumulated_frames=par["max_frames"], disocclusion_threshold=par["disocclusion"], antilag_sigma_scale=par["sigma"],
                      antilag_power=par["power"], max_blur_radius=par["radius"])
    return pipe


def put(pipe, planes):
    for key, plane in INPUT_PLANES + (("denoised", L.PLANE_DENOISED),):
        D.upload(pipe, plane, planes[key])


def denoise(pipe, world, cam, frame_index):
    pipe.render(world[0], cam, world[1], L.PASS_DENOISE, frame_index=frame_index)
    return D.download(pipe, L.PLANE_ACCUM), D.download(pipe, L.PLANE_DENOISED)


def same_values(a, b):
    """value for value: +0 equals -0, NaN equals NaN"""
    if a.dtype == np.uint16:
        a, b = a.view(np.float16), b.view(np.float16)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def assert_equals_oracle(what, acc, den, want_acc, want_den, other="the oracle's"):
    for name, got, want in (("accumulation", acc, want_acc), ("denoised", den, want_den)):
        same = same_values(got, want)
        if not same.all():
            y, x, c = np.argwhere(~same)[0]
            raise AssertionError(f"{what}: the {name} plane differs from {other} at {int((~same).any(axis=-1).sum())} pixels, first at "
                                 f"(x {x}, y {y}) channel {c}: device {got.view(np.float16)[y, x] if got.dtype == np.uint16 else got[y, x]}, "
                                 f"expected {want.view(np.float16)[y, x] if want.dtype == np.uint16 else want[y, x]}")


def run_case(ctx, world, inp):
    """the device through the case's steps -> (pipeline, accumulation, denoised)"""
    h, w = inp["cur"]["depth"].shape
    pipe = make_pipe(ctx, w, h, inp["params"])
    if inp["have_history"]:
        put(pipe, inp["prev"])
        denoise(pipe, world, inp["prev_cam"], inp["frame_index"] - 1)   # leaves the previous planes' geometry as the history's
        D.upload(pipe, L.PLANE_ACCUM, inp["hist"])                       # ... and this is its radiance and its frame counts
    put(pipe, inp["cur"])
    acc, den = denoise(pipe, world, inp["cam"], inp["frame_index"])
    return pipe, acc, den


def check_case(what, inp, acc, den):
    want_den, want_acc = O.denoise_steps(inp)
    assert_equals_oracle(what, acc, den, want_acc, want_den)
    t = W.temporal(inp["prev"], inp["hist"], inp["cur"], inp["cam"], inp["prev_cam"], inp["params"], inp["have_history"])
    s = W.spatial(acc, inp["cur"], inp["cam"], inp["params"], inp["frame_index"])   # on the accumulation as it stands on the device
    dev = W.check_temporal(acc, t, W.DENOISE_ORACLE_DEV, what=what)
    half = W.check_spatial(den, s, what=what)
    miss = ~t.hit
    assert np.all(acc[miss] == 0.0) and np.all(den[miss] == 0xFFFF), f"{what}: a miss pixel was written"
    print(f"{what}: device == oracle; against the witness {dev:.3e} M (bound {W.DENOISE_ORACLE_DEV:.1e}), {half} half steps")


@pytest.mark.parametrize("case", W.cases(), ids=lambda c: "-".join(map(str, c)))
def test_denoise_case_per_pixel(ctx, world, case):
    inp = W.case_inputs(*case)
    pipe, acc, den = run_case(ctx, world, inp)
    check_case(str(case), inp, acc, den)
    for key, plane in INPUT_PLANES:   # the inputs are the pass's to read only
        assert np.array_equal(D.download(pipe, plane).view(np.uint8), np.ascontiguousarray(inp["cur"][key]).view(np.uint8)), key
    if case[0] == "S0":   # restart_denoiser: the next frame is a first frame again, whatever history there is
        D.upload(pipe, L.PLANE_DENOISED, inp["cur"]["denoised"])
        again = denoise(pipe, world, inp["cam"], inp["frame_index"])     # with history: the count grows
        hit = np.isfinite(inp["cur"]["depth"])
        assert (again[0][hit][:, 3] > 1.0).mean() > 0.5
        D.upload(pipe, L.PLANE_DENOISED, inp["cur"]["denoised"])
        pipe.restart_denoiser()
        acc2, den2 = denoise(pipe, world, inp["cam"], inp["frame_index"])
        check_case(str(case) + " after restart_denoiser", inp, acc2, den2)


def _three_frames(inp):
    """S2's two frames and a third (the previous planes seen again): (planes, camera, frame index)"""
    f = inp["frame_index"]
    return ((inp["prev"], inp["prev_cam"], f - 1), (inp["cur"], inp["cam"], f), (inp["prev"], inp["prev_cam"], f + 1))


@pytest.mark.parametrize("w,h", W.CASES["S2"][1])
def test_bound_accumulation_plane(ctx, world, w, h):
    """denoise_pass with PLANE_ACCUM bound to caller memory keeps the history in a pair of its own and copies the result out: the same
    values as the pipeline that trades buffers, in the plane and in the caller's memory; binding or releasing starts the history over"""
    inp = W.case_inputs("S2", w, h)
    frames = _three_frames(inp)
    own = make_pipe(ctx, w, h, inp["params"])
    bound = make_pipe(ctx, w, h, inp["params"])
    late = make_pipe(ctx, w, h, inp["params"])       # binds between frames 2 and 3
    freed = make_pipe(ctx, w, h, inp["params"])      # releases between frames 2 and 3
    mem = {k: D.DeviceMemory(np.full((h, w, 4), np.nan, np.float32)) for k in ("bound", "late", "freed")}
    bound.bind_plane(L.PLANE_ACCUM, mem["bound"].ptr, w * h * 16)
    freed.bind_plane(L.PLANE_ACCUM, mem["freed"].ptr, w * h * 16)
    for k, (planes, cam, f) in enumerate(frames):
        if k == 2:
            late.bind_plane(L.PLANE_ACCUM, mem["late"].ptr, w * h * 16)
            freed.bind_plane(L.PLANE_ACCUM, 0, 0)
        out = {}
        for name, pipe in (("own", own), ("bound", bound), ("late", late), ("freed", freed)):
            put(pipe, planes)
            out[name] = denoise(pipe, world, cam, f)
        hit = np.isfinite(planes["depth"])
        assert_equals_oracle(f"bound plane, frame {k + 1}", out["bound"][0], out["bound"][1], out["own"][0], out["own"][1], other="the unbound pipeline's")
        assert same_values(mem["bound"].read(bound), out["own"][0]).all(), "the caller's memory does not hold the accumulation"
        if k == 1:   # the history is in use: the second frame found some of the first
            assert (out["own"][0][hit][:, 3] > 1.0).mean() > 0.3
            for name in ("late", "freed"):
                assert_equals_oracle(f"{name}, frame 2", out[name][0], out[name][1], out["own"][0], out["own"][1], other="the unbound pipeline's")
        if k == 2:
            assert (out["own"][0][hit][:, 3] > 1.0).mean() > 0.3
            for name in ("late", "freed"):
                assert np.all(out[name][0][hit][:, 3] == 1.0), f"{name}: history survived the plane changing hands"
            assert same_values(mem["late"].read(late), out["late"][0]).all()
    for pipe in (bound, late):   # the memory outlives its use: release the planes, then free
        pipe.bind_plane(L.PLANE_ACCUM, 0, 0)
        pipe.exposure()
    for m in mem.values():
        m.free()
