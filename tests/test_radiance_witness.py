"""The C oracle's sky, sun, hash keys and hash insert (oracle/shade.c) against the independent numpy witness (radiance_witness.py), with
the bounds and on the inputs tests/test_gpu_radiance_functions.py holds the device functions to: half an fp16 step per row for radiance,
exact integers, LogLuv fields exact off the quantisation steps. With it these oracle rows have two witnesses."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import parity_util as P
import radiance_witness as W

F = np.float32
HALF_STEP = 2.0 ** -12   # half an fp16 step (11 significant bits), relative: what every radiance value here is stored to
STATES = ("default", "low_sun", "hazy_noon", "turbid10")
KEY_CAPACITIES = (1, 16, 97, 1 << 14, 1 << 26)


def named_state(name):
    """One of the four states of tests/golden/sky_states.json (its "default" is not the packaged default sun, which is P.sky_state()).
    "grazing" is low_sun with the sun turned down to 2 degrees above the horizon: the disk the shader draws reaches 3.9 degrees
    (sin^2 gamma < sin R), so only there do directions inside the disk point below the horizon; the lowest named sun stands at 10."""
    with open(os.path.join(P.ROOT, "tests", "golden", "sky_states.json")) as f:
        s = np.asarray(json.load(f)["low_sun" if name == "grazing" else name]["state"], F)
    if name == "grazing":
        flat = s[[48, 50]].astype(np.float64) / np.hypot(s[48], s[50])
        s[48:51] = W.normalize32([[flat[0] * np.cos(np.radians(2.0)), np.sin(np.radians(2.0)), flat[1] * np.cos(np.radians(2.0))]])[0]
    return s


def oracle_rows(fn, state, dirs):
    sky = O.sky_from(state)
    d = np.ascontiguousarray(dirs, F)
    out = np.zeros_like(d)
    fp = C.POINTER(C.c_float)
    di, oi = d.ctypes.data, out.ctypes.data
    for i in range(len(d)):
        fn(C.byref(sky), C.cast(di + 12 * i, fp), C.cast(oi + 12 * i, fp))
    return out


def check_sky(got, wit, what):
    """NaN exactly where the witness has it; elsewhere each row within half an fp16 step of its own largest channel. Returns the worst ratio."""
    nan = np.isnan(wit).any(axis=1)
    assert np.array_equal(np.isnan(got).all(axis=1), nan) and not np.isnan(got[~nan]).any(), f"{what}: NaN rows differ"
    scale = np.abs(wit[~nan]).max(axis=1)
    dev = np.abs(got[~nan].astype(np.float64) - wit[~nan]).max(axis=1)
    zero = scale == 0
    assert (dev[zero] == 0).all(), f"{what}: rows the witness has at zero"
    worst = float((dev[~zero] / scale[~zero]).max(initial=0.0))
    print(f"{what}: worst deviation {worst:.3g} of the row's largest channel, {int(nan.sum())} NaN rows of {len(wit)}")
    assert worst <= HALF_STEP, f"{what}: {worst:.3g}"
    return worst


def check_sun(got, wit, sc2, centre, what):
    """Off the limb (sc2 >= 2^-8) each row within half an fp16 step of its own largest channel; on it within 2^-6 of the disk centre's.
    Zero and non-zero agree wherever |sc2| > 2^-20; the limb is at most 1 % of the disk. Returns (worst off the limb, worst on it)."""
    got = got.astype(np.float64)
    lit = sc2 > 0
    limb = lit & (sc2 < F(2.0 ** -8))
    assert lit.sum() > 1000 and limb.sum() <= 0.01 * lit.sum(), f"{what}: {int(limb.sum())} limb rows of {int(lit.sum())}"
    sure = np.abs(sc2) > F(2.0 ** -20)
    assert np.array_equal((got != 0).any(axis=1)[sure], (wit != 0).any(axis=1)[sure]), f"{what}: zero rows differ"
    dev = np.abs(got - wit).max(axis=1)
    off = ~limb & (wit != 0).any(axis=1)
    worst = float((dev[off] / np.abs(wit[off]).max(axis=1)).max())
    rest = ~limb & ~off & sure
    assert (dev[rest] == 0).all(), f"{what}: dark rows"
    worst_limb = float((dev[limb | ~sure] / np.abs(centre).max()).max(initial=0.0))
    print(f"{what}: worst deviation {worst:.3g} of the row's largest channel off the limb, {worst_limb:.3g} of the centre on it "
          f"({int(limb.sum())} limb rows of {int(lit.sum())} lit)")
    assert worst <= HALF_STEP and worst_limb <= 2.0 ** -6, f"{what}: {worst:.3g}, {worst_limb:.3g}"
    return worst, worst_limb


@pytest.mark.parametrize("name", STATES)
def test_oracle_sky_matches_witness(name):
    state = named_state(name)
    dirs = W.sky_directions(state, np.random.default_rng(31), 21000)
    wit = W.sky_radiance(state, dirs)
    assert np.isfinite(wit).all(axis=1).sum() > 20000 and (np.abs(wit).max(axis=1) > 0).sum() > 20000
    check_sky(oracle_rows(O.lib().orc_sky_radiance, state, dirs), wit, f"oracle sky {name}")


def test_oracle_sky_of_a_sun_below_the_horizon_is_zero():
    state = np.array(named_state("hazy_noon"), F)
    state[49] = -state[49]
    dirs = W.sky_directions(state, np.random.default_rng(32), 3000)
    assert not W.sky_radiance(state, dirs).any()
    assert not oracle_rows(O.lib().orc_sky_radiance, state, dirs).any()


@pytest.mark.parametrize("name", STATES + ("grazing",))
def test_oracle_sun_matches_witness(name):
    state = named_state(name)
    dirs = W.sun_directions(state, np.random.default_rng(33), 21000)
    wit, sc2 = W.sun_radiance(state, dirs)
    cg = W.cos_gamma32(state, dirs)
    below = (dirs[:, 1] < 0) & (sc2 > 0) & (cg >= 0)   # inside the disk and under the horizon
    assert (cg < 0).sum() > 1000 and (below.sum() > 100) == (name == "grazing")
    check_sun(oracle_rows(O.lib().orc_sun_radiance, state, dirs), wit, sc2, W.sun_centre(state), f"oracle sun {name}")


def test_witness_sun_centre_and_albedo_anchors():
    """what the witness must give whatever its code: the disk's centre is the darkening polynomial at 1, the albedo curve is the sRGB
    one (0 -> 0, 1023 -> 1 to the float32 literals' rounding, continuous across the 0.04045 branch between codes 41 and 42), white albedo leaves a colour alone"""
    state = named_state("default")
    sun = np.asarray(state, F)[48:51][None]
    rgb, sc2 = W.sun_radiance(state, sun)
    assert sc2[0] > 0.999 and np.allclose(rgb[0], W.sun_centre(state), rtol=1e-3)
    lin = W.srgb_to_linear(np.arange(1024))
    assert lin[0] == 0 and abs(lin[1023] - 1) < 2e-7 and (np.diff(lin) > 0).all()
    assert 41 / 1023 < 0.04045 < 42 / 1023 and abs((lin[42] - lin[41]) - (lin[41] - lin[40])) < 2e-6
    assert 0.21404 < lin[512] < 0.21586   # the curve's well-known values at 0.5 and 128 / 255, either side of 512 / 1023
    r = np.array([[0.3, 2.0, 0.07]], F)
    alb, out = W.modulate_by_avg_albedo(r, W.pack_albedo([1023], [1023], [1023], [3]))
    assert np.allclose(alb, 1) and np.allclose(out, r, rtol=2e-6)


def key_rows(rng, n):
    pos = rng.integers(-(1 << 31), 1 << 31, (n, 3))
    pos[: n // 2] = rng.integers(-300, 300, (n // 2, 3))
    edge = np.array([-(1 << 31), (1 << 31) - 1, 0, -1, 1])
    pos[n // 2: n // 2 + 500] = edge[rng.integers(0, 5, (500, 3))]
    return pos.astype(np.int32), rng.integers(0, 6, n).astype(np.uint32), np.array(KEY_CAPACITIES, np.uint32)[rng.integers(0, 5, n)]


def test_oracle_hash_keys_match_witness():
    pos, face, cap = key_rows(np.random.default_rng(34), 20000)
    fp, loc = W.key_fingerprint(pos, face), W.key_location(pos, face, cap)
    l = O.lib()
    for i in range(len(pos)):
        p = (C.c_int32 * 3)(*pos[i].tolist())
        assert l.orc_hash_fingerprint(p, int(face[i])) == fp[i] and l.orc_hash_location(p, int(face[i]), int(cap[i])) == loc[i], i
    assert fp.min() >= 1 and (loc < cap).all()


def check_windows(got, want, flagged, what):
    """fingerprints and meta words exact; L, u, v within one step, exact off the steps the witness flags; at most 2 % flagged"""
    got, want = np.asarray(got, np.uint32).reshape(-1, 3, 3), np.asarray(want, np.uint32).reshape(-1, 3, 3)
    assert np.array_equal(got[:, :, 0], want[:, :, 0]), f"{what}: fingerprints"
    assert np.array_equal(got[:, :, 2], want[:, :, 2]), f"{what}: stamps and counts"
    d = np.abs(W.logluv_fields(got[:, :, 1]) - W.logluv_fields(want[:, :, 1])).max(axis=(1, 2))
    assert flagged.mean() <= 0.02, f"{what}: {flagged.mean():.3%} of the rows sit on a quantisation step"
    print(f"{what}: {int((d > 0).sum())} of {len(d)} rows differ by a step, {int(flagged.sum())} flagged")
    assert d.max() <= 1 and (d[~flagged] == 0).all(), f"{what}: {np.flatnonzero((d > 0) & ~flagged)[:5]}"


def test_oracle_hash_insert_matches_witness():
    rng = np.random.default_rng(35)
    keys = [(tuple(int(v) for v in rng.integers(-50, 50, 3)), int(rng.integers(0, 6))) for _ in range(6)]
    fps = W.key_fingerprint([k[0] for k in keys], [k[1] for k in keys])
    win, fp, value, frame = W.insert_cases(rng, fps)
    want, flagged = zip(*(W.hash_insert(win[i], fp[i], value[i], frame[i]) for i in range(len(win))))
    by_fp = {int(f): k for f, k in zip(fps, keys)}
    gi = O.GI(1, 1)   # capacity 1: every key probes entries 0, 1, 2 of the capacity + 2 the table holds
    table = gi.l.orc_gi_hash_ptr(gi.h)
    got = np.zeros_like(win)
    for i in range(len(win)):
        C.memmove(table, win[i].ctypes.data, 36)
        pos, face = by_fp[int(fp[i])]
        gi.insert(pos, face, value[i], int(frame[i]))
        C.memmove(got[i].ctypes.data, table, 36)
    check_windows(got, want, np.array(flagged), "oracle insert")
    meta = np.asarray(want, np.uint32).reshape(-1, 3, 3)[:, :, 2]
    assert (meta >> 16).max() == 65535 and 404 in (meta >> 16) and 405 not in (meta >> 16)
