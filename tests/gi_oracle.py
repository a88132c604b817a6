"""The C oracle's final gather and surfel pass run on the cases of tests/gi_witness.py, each from the seeded state, one pass at a time. A
helper module, not a test: tests/test_gi_witness.py holds these runs to the witness, tests/test_gpu_gi_witness.py the kernels to both."""
import functools
from types import SimpleNamespace

import gi_witness as G
import oracle_lib as O
import parity_util as P
from dust_amd import _lib as L

MODES = {"hier": O.ORC_MODE_HIER, "brute": O.ORC_MODE_BRUTE}
FRAME = L.PASS_PRIMARY | L.PASS_AMBIENT_OCCLUSION


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "empty":
        s = O.Scene()
        s.commit()
        return s
    return P.oracle_scene_with_history(*G.scene_inputs(name))


@functools.lru_cache(maxsize=None)
def gather(name, mode="hier"):
    """-> namespace(before, after: the illuminance plane around the gather; wit: the witness's gather on the planes the oracle's gather read;
    hash, pool: the state after it; removed; depth, normal)"""
    c = G.gather_inputs(name)
    g = P.render_oracle(scene(c["scene"]), c["cam"], c["sky"], c["w"], c["h"], FRAME, c["noise5"], c["rand"], mode=MODES[mode])
    ill, wit, removed = G.prepare_gather(name, g.depth, g.normal, g.illuminance)
    g.illuminance[:] = ill
    gi = O.GI(c["capacity"], c["pool_size"])
    gi.write(c["table"], c["pool"])
    P.render_oracle(scene(c["scene"]), c["cam"], c["sky"], c["w"], c["h"], L.PASS_FINAL_GATHER, c["noise5"], c["rand"], mode=MODES[mode],
                    noise0=c["noise0"], gi=gi, frame_index=c["frame_index"], g=g)
    return SimpleNamespace(before=ill, after=g.illuminance.copy(), wit=wit, hash=gi.hash(), pool=gi.pool(), removed=removed,
                           depth=g.depth.copy(), normal=g.normal.copy())


def _surfel_pass(scene_name, c, mode, pool_size):
    from dust_amd import scenes
    gi = O.GI(c["capacity"], pool_size)
    gi.write(c["table"], c["pool"])
    P.render_oracle(scene(scene_name), scenes.camera_for((1.0, 2.0, 3.0)), c["sky"], 8, 8, L.PASS_SURFEL, c["noise5"], c["rand"], mode=MODES[mode],
                    noise0=c["noise0"], gi=gi, frame_index=c["frame_index"])
    return SimpleNamespace(hash=gi.hash(), pool=gi.pool(), superseded=gi.last_superseded())


@functools.lru_cache(maxsize=None)
def surfel(name, mode="hier"):
    c = G.surfel_inputs(name)
    return _surfel_pass("T", c, mode, c["pool_size"])


@functools.lru_cache(maxsize=None)
def apply(capacity, mode="hier"):
    return _surfel_pass("empty", G.apply_inputs(capacity), mode, G.APPLY_POOL)
