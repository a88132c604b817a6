"""The device's sky, sun, albedo modulation, hash keys and hash insert -- the inlined bodies the frame kernels use, through
dust_hip_device_eval 15..19 -- against the independent numpy witness (radiance_witness.py), row by row. Every radiance value ends in an
fp16 texel or a LogLuv word, so the bound is half an fp16 step, 2^-12 of a reference magnitude: a smaller deviation cannot move a stored half
by more than a rounding tie. A quarter of the frame tests' 1e-3, and per row: no row hides behind a bright one.
tests/test_radiance_witness.py holds the C oracle to the same witness with the same checks on the CPU."""
import numpy as np
import pytest

import parity_util as P
import radiance_witness as W
from dust_amd import api
from test_gpu_golden import words
from test_radiance_witness import HALF_STEP, STATES, check_sky, check_sun, check_windows, key_rows, named_state

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    return api.Context(device=0)


def with_state(state, dirs):
    """the rows of fns 15 and 16: the 56 floats of the sky state in rows 0..18 (the last word padding), then one direction per row"""
    head = np.zeros(57, F)
    head[:56] = state
    return words(np.concatenate([head.reshape(19, 3), np.asarray(dirs, F)]))


def radiance(ctx, fn, state, dirs):
    out = ctx.device_eval(fn, with_state(state, dirs), 3)
    assert not out[:19].any(), "the state's rows give zero"
    return out[19:].view(F)


@pytest.mark.parametrize("name", STATES + ("packaged",))
def test_device_sky_matches_witness(ctx, name):
    """uniform, sun-centred (the sun's own direction and its float32 neighbours among them), horizon (y = +0 and -0), zenith, nadir and
    antisolar rows: each within half an fp16 step of its own largest channel, NaN exactly where the float32 cos_gamma leaves [-1, 1]"""
    state = P.sky_state() if name == "packaged" else named_state(name)
    dirs = W.sky_directions(state, np.random.default_rng(41), 27000)
    wit = W.sky_radiance(state, dirs)
    assert (np.abs(wit).max(axis=1) > 0).sum() > 26000
    check_sky(radiance(ctx, 15, state, dirs), wit, f"device sky {name}")


def test_device_sky_of_a_sun_below_the_horizon_is_zero(ctx):
    state = np.array(named_state("hazy_noon"), F)
    state[49] = -state[49]
    dirs = W.sky_directions(state, np.random.default_rng(42), 3000)
    assert not W.sky_radiance(state, dirs).any()
    assert not radiance(ctx, 15, state, dirs).view(np.uint32).any()


@pytest.mark.parametrize("name", STATES + ("grazing",))
def test_device_sun_matches_witness(ctx, name):
    """across the disk the shader draws and past its edge, behind the viewer, and (the grazing sun) inside the disk under the horizon"""
    state = named_state(name)
    dirs = W.sun_directions(state, np.random.default_rng(43), 24000)
    wit, sc2 = W.sun_radiance(state, dirs)
    cg = W.cos_gamma32(state, dirs)
    below = (dirs[:, 1] < 0) & (sc2 > 0) & (cg >= 0)
    assert (cg < 0).sum() > 1000 and (below.sum() > 100) == (name == "grazing")
    check_sun(radiance(ctx, 16, state, dirs), wit, sc2, W.sun_centre(state), f"device sun {name}")


def test_device_albedo_modulation_matches_witness(ctx):
    """all 1024 codes of each field with the other two at 0, 512 and 1023, then random rows with radiance over seven decades"""
    rng = np.random.default_rng(44)
    code = np.arange(1024, dtype=np.uint32)
    packed = []
    for other in (0, 512, 1023):
        o = np.full(1024, other, np.uint32)
        packed += [W.pack_albedo(code, o, o), W.pack_albedo(o, code, o, 1), W.pack_albedo(o, o, code, 3)]
    packed = np.concatenate(packed + [rng.integers(0, 1 << 32, 10000, dtype=np.uint64).astype(np.uint32)])
    r = (10.0 ** rng.uniform(-4, 3, (len(packed), 3))).astype(F)
    out = ctx.device_eval(17, words(r, packed), 6).view(F).astype(np.float64)
    alb, mod = W.modulate_by_avg_albedo(r, packed)
    dev = np.abs(out[:, :3] - alb)
    zero = alb == 0
    assert zero.sum() > 3 * 1024 and (out[:, :3][zero] == 0).all(), "code 0 is exactly black"
    first = packed[:1024] >> 22
    assert first[41] == 41 and alb[41, 0] == (41 / 1023) / float(F(12.92)) and alb[42, 0] > (42 / 1023) / 12.92   # both sides of the 0.04045 branch
    worst = float((dev[~zero] / alb[~zero]).max())
    bound = HALF_STEP * np.abs(mod).max(axis=1) + 2.0 ** -20 * np.abs(r).max(axis=1)   # (the second term: rows whose sRGB mix cancels)
    worst_mod = float((np.abs(out[:, 3:] - mod).max(axis=1) / bound).max())
    print(f"device albedo: worst deviation {worst:.3g} of the linearised value; modulated colour at {worst_mod:.3g} of its bound")
    assert worst <= HALF_STEP and worst_mod <= 1.0


def test_device_hash_keys_match_witness(ctx):
    """negative coordinates, INT32_MIN / INT32_MAX (what the float -> int conversion saturates to), faces 0..5, capacities 1 .. 1 << 26"""
    pos, face, cap = key_rows(np.random.default_rng(45), 20000)
    out = ctx.device_eval(18, words(pos.view(np.uint32), face, cap), 2)
    assert np.array_equal(out[:, 0], W.key_fingerprint(pos, face))
    assert np.array_equal(out[:, 1], W.key_location(pos, face, cap))


def test_device_hash_insert_matches_witness(ctx):
    """hash_insert_window on a register window (what the deterministic apply runs), every branch: empty slots, the fingerprint in each
    slot, eviction among equal and among distinct stamps, counts around the cap of 403, stamps and frame_index around the 16-bit wrap"""
    rng = np.random.default_rng(46)
    win, fp, value, frame = W.insert_cases(rng, rng.integers(1, 1 << 32, 6, dtype=np.uint64))
    want, flagged = zip(*(W.hash_insert(win[i], fp[i], value[i], frame[i]) for i in range(len(win))))
    got = ctx.device_eval(19, words(win, fp, value, frame), 9)
    check_windows(got, want, np.array(flagged), "device insert")
    meta = np.asarray(want, np.uint32).reshape(-1, 3, 3)[:, :, 2]
    assert (meta >> 16).max() == 65535 and 404 in (meta >> 16) and 405 not in (meta >> 16)
    moved = (np.asarray(want, np.uint32) != win).reshape(-1, 3, 3).any(axis=2)
    assert moved.sum(axis=1).max() == 1 and all(moved[:, k].sum() > 100 for k in range(3))   # one entry a row, each slot often
