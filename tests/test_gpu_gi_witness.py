"""The final gather and the surfel pass of dust_amd/csrc/gi.hip against the float64 witness of tests/gi_witness.py, each pass ALONE through the
public frame path from a state the test chooses (StandardPipeline.write_gi, tests/device_planes.py): render with PASS_FINAL_GATHER only,
then with PASS_SURFEL | PASS_GI_ORDERED only, on the packet kernels, the ray streams (DUST_HIP_RAY_STREAM=1) and the serial apply
(DUST_HIP_DEBUG=16). Texels per pixel, hash and pool entry by entry, the same checks tests/test_gi_witness.py makes of the C oracle; the
device's integer state is the oracle's bit for bit. The witness of a case is computed once, from the planes the device's own camera-ray
and AO passes left, and shared by the three configurations (they read the same planes)."""
import hashlib

import numpy as np
import pytest

import device_planes as DP
import gi_oracle as GO
import gi_witness as G
import parity_util as P
from dust_amd import _lib as L
from dust_amd import api, scenes

pytestmark = pytest.mark.gpu
CONFIGS = {"packets": {}, "streams": {"DUST_HIP_RAY_STREAM": "1"}, "serial-apply": {"DUST_HIP_DEBUG": "16"}}
SWITCHES = ("DUST_HIP_RAY_STREAM", "DUST_HIP_DEBUG", "DUST_HIP_NO_SURFEL_SORT")
DEVICE_BOUNDS = (G.GI_DEVICE_T_DEV, G.GI_DEVICE_RADIANCE_DEV)
_prepared = {}


@pytest.fixture(scope="module")
def ctx():
    return api.Context(device=0)


@pytest.fixture(scope="module")
def device_scenes(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = DP.empty_scene(ctx) if name == "empty" else P.hip_scene_with_history(ctx, *G.scene_inputs(name))
        return made[name]
    return get


def pipeline(ctx, monkeypatch, config, w, h, capacity, pool_size):
    """a pipeline made under the configuration's switches (they are read when it is created)"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in config.items():
        monkeypatch.setenv(k, v)
    pipe = api.StandardPipeline(ctx, w, h)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    n0, n5 = G.noise()
    pipe.set_noise(0, n0)
    pipe.set_noise(5, n5)
    pipe.configure_gi(capacity, pool_size)
    return pipe


def prepared(name, depth, normal, illuminance):
    key = (name, hashlib.sha1(depth.tobytes() + normal.tobytes() + illuminance.tobytes()).hexdigest())
    if key not in _prepared:
        _prepared[key] = G.prepare_gather(name, depth, normal, illuminance)
    return _prepared[key]


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", sorted(G.GATHER_CASES))
def test_final_gather_against_witness(ctx, device_scenes, monkeypatch, name, config):
    c = G.gather_inputs(name)
    scene = device_scenes(c["scene"])
    pipe = pipeline(ctx, monkeypatch, CONFIGS[config], c["w"], c["h"], c["capacity"], c["pool_size"])
    frame = dict(frame_index=c["frame_index"], rand=c["rand"])
    pipe.render(scene, c["cam"], c["sky"], GO.FRAME, **frame)
    ctx.sync()
    depth, normal, ill0 = (pipe.read_plane(p) for p in (L.PLANE_DEPTH, L.PLANE_NORMAL, L.PLANE_ILLUMINANCE))
    before, wit, removed = prepared(name, depth, normal, ill0)
    cond = G.assert_gather_conditions(name, wit)
    DP.upload(pipe, L.PLANE_ILLUMINANCE, before)
    pipe.write_gi(c["table"], c["pool"])
    pipe.render(scene, c["cam"], c["sky"], L.PASS_FINAL_GATHER, **frame)
    ctx.sync()
    after = pipe.read_plane(L.PLANE_ILLUMINANCE)
    table, pool = pipe.read_gi()
    what = f"{name} {config}"
    worst = G.check_gather_texels(before, after, wit, what, bounds=DEVICE_BOUNDS)
    worst.update(G.check_gather_state(table, c["pool"], pool, wit, what))
    if name in G.STATE_LEVEL:
        assert worst["slots_compared"] == c["pool_size"] and not wit.maybe_stamped
    print(what, worst, cond, "removed", removed)
    orc = GO.gather(name)
    # what decides the gather's rays -- depth, normal, hit distance -- is the oracle's bit for bit (the parity suite holds the two passes
    # before it to that), so the integer state after it is the oracle's too, and so is every hit distance
    hit = np.isfinite(depth)
    assert orc.depth.tobytes() == depth.tobytes() and (orc.normal[hit] == normal[hit]).all() and orc.before[..., 3].tobytes() == before[..., 3].tobytes(), what
    assert G.words_of(orc.hash).tobytes() == np.ascontiguousarray(table, np.uint32).tobytes(), what
    assert orc.pool.tobytes() == pool.tobytes(), what
    assert orc.after[..., 3].tobytes() == after[..., 3].tobytes(), what


def run_surfel_pass(ctx, device_scenes, monkeypatch, config, scene, c, pool_size):
    pipe = pipeline(ctx, monkeypatch, config, 16, 16, c["capacity"], pool_size)
    pipe.write_gi(c["table"], c["pool"])
    pipe.render(device_scenes(scene), scenes.camera_for((1.0, 2.0, 3.0)), c["sky"], L.PASS_SURFEL | L.PASS_GI_ORDERED, frame_index=c["frame_index"], rand=c["rand"])
    ctx.sync()
    return pipe.read_gi()


def hold_state(table, pool, ap, want_pool, orc, what):
    print(what, G.check_hash(table, ap, what))
    G.check_pool(pool, want_pool, what)
    got, ref = np.ascontiguousarray(table, np.uint32), G.words_of(orc.hash)
    assert (got[:, 0] == ref[:, 0]).all() and (got[:, 2] == ref[:, 2]).all() and pool.tobytes() == orc.pool.tobytes(), what


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", sorted(G.SURFEL_CASES))
def test_surfel_pass_against_witness(ctx, device_scenes, monkeypatch, name, config):
    c = G.surfel_inputs(name)
    tr, ap, want_pool = G.surfel_witness(name)
    cond = G.surfel_conditions(tr)
    assert all(cond[k] >= least for k, least in G.SURFEL_MINIMA.items()) and cond["undecided"] == 0, cond
    assert G.flagged_share([ap]) <= G.FLAGGED_CAP
    table, pool = run_surfel_pass(ctx, device_scenes, monkeypatch, CONFIGS[config], "T", c, c["pool_size"])
    hold_state(table, pool, ap, want_pool, GO.surfel(name), f"{name} {config}")


APPLY_RUNS = [(cap, config) for cap in G.APPLY_CAPACITIES for config in sorted(CONFIGS)] + [(1 << 14, "unsorted")]


@pytest.mark.parametrize("capacity,config", APPLY_RUNS)
def test_apply_alone_against_witness(ctx, device_scenes, monkeypatch, capacity, config):
    """the empty scene: every live surfel inserts the sky, nothing depends on a ray. `unsorted`: the pool traced in pool order"""
    c = G.apply_inputs(capacity)
    tr, ap, want_pool = G.apply_witness(capacity)
    rq = np.nonzero(tr.request & tr.live)[0]
    G.assert_apply_conditions(capacity, G.apply_conditions(ap, rq, tr.key[rq], tr.face[rq]))
    assert G.flagged_share([G.apply_witness(k)[1] for k in G.APPLY_CAPACITIES]) <= G.FLAGGED_CAP
    switches = {"DUST_HIP_NO_SURFEL_SORT": "1"} if config == "unsorted" else CONFIGS[config]
    table, pool = run_surfel_pass(ctx, device_scenes, monkeypatch, switches, "empty", c, G.APPLY_POOL)
    hold_state(table, pool, ap, want_pool, GO.apply(capacity), f"apply {capacity} {config}")
