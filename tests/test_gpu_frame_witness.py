"""The camera-ray pass (k_primary*, primary_shade) and the sun-shadow + AO pass (ao_packet) against the float64 voxel ray caster of
tests/frame_witness.py, per pixel, through the public frame path: every case of the CPU test through StandardPipeline.render, and one
of them as three same-view frames of one render_frames launch (the kept G-buffer of primary_shade and store_primary_texels, each member's
own noise slice and rand). The device planes are held to the oracle's bit for bit where the parity suite demands it, and to the witness
directly; the AO stage is checked from the device's own depth and normal texels."""
import functools

import numpy as np
import pytest

import frame_witness as W
import oracle_lib as O
import parity_util as P
from dust_amd import _lib as L
from dust_amd import api

pytestmark = pytest.mark.gpu
PASSES = L.PASS_PRIMARY | L.PASS_AMBIENT_OCCLUSION


@pytest.fixture(scope="module")
def ctx():
    return api.Context(device=0)


@functools.lru_cache(maxsize=None)
def oracle_frame(name, frame_index, rand):
    c = W.case_inputs(name)
    return P.render_oracle(P.oracle_scene_with_history(*W.scene_of(name)), c["cam"], c["sky"], c["w"], c["h"], PASSES,
                           c["noise5"][frame_index % W.NOISE_LAYERS], rand, mode=O.ORC_MODE_HIER)


def pipeline(ctx, c):
    pipe = api.StandardPipeline(ctx, c["w"], c["h"])
    pipe.set_noise(5, c["noise5"])
    return pipe


def hold_to_oracle_and_witness(name, hip, frame_index, rand, what):
    c = W.case_inputs(name)
    P.assert_parity(P.compare_gbuffers(oracle_frame(name, frame_index, rand), hip))
    worst = W.check_primary(hip, W.primary_witness(name), c["w"], what)
    aw = W.ambient_occlusion(W.witness_scene(name), c["cam"], c["sky"], c["w"], c["h"], hip["depth"], hip["normal"],
                             c["noise5"][frame_index % W.NOISE_LAYERS], rand)
    worst.update(W.check_ao(hip["illuminance"], aw, c["w"], what))
    cond = W.input_conditions(W.primary_witness(name), aw)
    for k in ("ao_undecided", "sun_undecided"):
        assert cond[k] <= W.UNDECIDED_CAP, (k, cond)
    for k in ("ao_hit", "ao_miss", "lit_open", "lit_shadowed", "unlit"):
        assert cond[k] >= W.MINIMA[k], (k, cond)
    print(what, worst)


@pytest.mark.parametrize("name", W.frame_cases())
def test_frame_against_witness(ctx, name):
    c = W.case_inputs(name)
    scene = P.hip_scene_with_history(ctx, *W.scene_of(name))
    pipe = pipeline(ctx, c)
    pipe.render(scene, c["cam"], c["sky"], PASSES, frame_index=c["frame_index"], rand=c["rand"])
    ctx.sync()
    hold_to_oracle_and_witness(name, P.read_hip_gbuffer(pipe), c["frame_index"], c["rand"], f"{name} render")


def test_view_run_members_against_witness(ctx):
    """three frames of one view in one launch: every member carries the view's G-buffer and its own sun-shadow and AO texels"""
    name = W.RUN_CASE
    c = W.case_inputs(name)
    scene = P.hip_scene_with_history(ctx, *W.scene_of(name))
    pipes = [pipeline(ctx, c) for _ in W.RUN_MEMBERS]
    api.StandardPipeline.render_frames(pipes, scene, c["cam"], c["sky"], PASSES, [f for f, _ in W.RUN_MEMBERS], [r for _, r in W.RUN_MEMBERS])
    ctx.sync()
    texels = []
    for pipe, (frame_index, rand) in zip(pipes, W.RUN_MEMBERS):
        hip = P.read_hip_gbuffer(pipe)
        hold_to_oracle_and_witness(name, hip, frame_index, rand, f"{name} member frame {frame_index}")
        texels.append(hip["illuminance"][..., 3].tobytes())
    assert len(set(texels)) == len(texels)      # (the members' AO rays differ: no member got another's slice or rand)
