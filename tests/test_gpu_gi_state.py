"""GI state across the transitions of the sharded surfel pass (include/dust_hip.h, multi-GPU steps 6a / 6b): reconfiguring the GI
buffers after a sharded trace, cancelling a pending trace (configure_gi, clear), refused exchanges, a second trace, a trace without
DUST_PASS_GI_ORDERED and write_gi while a trace is pending. Every case ends on the same check: the pipelines under test equal, bit for
bit (hash, surfel pool as u32 words, PLANE_ILLUMINANCE), a FRESH pipeline configured directly to the final sizes and driven through the
same frames with the unsharded PASS_SURFEL | PASS_GI_ORDERED.

The ranks of a sharded trace are pipelines on the one GPU: each renders the whole frame's pixel passes (their GI state is identical, so
is their final gather), then traces its share of the pool; a loopback group (api.Comm.local) or, for a world of one,
StandardPipeline.gi_surfel_finish completes the pass."""
import numpy as np
import pytest

import parity_util as P
from dust_amd import _lib as L, api, synth

pytestmark = pytest.mark.gpu

W, H = 192, 104
PIX = L.PASS_PRIMARY | L.PASS_AMBIENT_OCCLUSION | L.PASS_FINAL_GATHER
SURF = L.PASS_SURFEL | L.PASS_GI_ORDERED
SMALL, LARGE = (4093, 776), (16384, 8197)


def stage_slots(pool):
    """the staging slots the first sharded trace of a pipeline allocates for a pool of this size (capi.cpp run_surfel_pass)"""
    return ((pool + 63) // 64 + 64) * 64


class Rig:
    def __init__(self):
        self.ctx = api.Context(device=0)
        data, _ = synth.castle_scene(scale=0.15)
        self.scene = P.hip_scene(self.ctx, P.SceneDesc.from_vox(data))
        self.n0, self.n5 = synth.stbn_scalar(layers=4), synth.stbn_unitvec3_cosine(layers=4)
        self.cam, self.sky = P.camera_for((122.0 * 0.15, 300.61 * 0.15, 54.45 * 0.15)), api.sky_struct(P.sky_state())

    def pipe(self, sizes):
        p = api.StandardPipeline(self.ctx, W, H)
        p.set_noise(0, self.n0)
        p.set_noise(5, self.n5)
        p.configure_gi(*sizes)
        return p

    def render(self, p, passes, f, **kw):
        p.render(self.scene, self.cam, self.sky, passes, f, synth.frame_rand(11, f), **kw)

    def frame(self, p, f):
        """the reference: one unsharded ordered frame"""
        self.render(p, PIX | SURF, f)

    def trace(self, ranks, f):
        """step 6a on every rank (after the whole frame's pixel passes)"""
        for p in ranks:
            self.render(p, PIX, f)
        for r, p in enumerate(ranks):
            self.render(p, SURF | L.PASS_GI_SHARDED, f, surfel_shard=(r, len(ranks)))

    def complete(self, ranks, comms, f):
        """step 6b"""
        if comms is None:
            ranks[0].gi_surfel_finish(f)
        else:
            for c, p in zip(comms, ranks):
                c.gi_surfel_exchange(p, f)

    def sharded_frame(self, ranks, comms, f):
        self.trace(ranks, f)
        self.complete(ranks, comms, f)


def group(rig, sizes, world):
    ranks = [rig.pipe(sizes) for _ in range(world)]
    return ranks, (api.Comm.local(rig.ctx, world) if world > 1 else None)


def refused(status, fn, *args, **kw):
    with pytest.raises(L.DustError) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)


def refused_completion(rig, ranks, comms, f, status=L.ERR_NOT_READY):
    """step 6b is refused: on a loopback group by the call that completes it (the others only join), with no communicator at once"""
    if comms is not None:
        for c, p in zip(comms[:-1], ranks[:-1]):
            c.gi_surfel_exchange(p, f)
        refused(status, comms[-1].gi_surfel_exchange, ranks[-1], f)
    for p in ranks:
        refused(status, p.gi_surfel_finish, f)


def assert_same_gi(ranks, ref, min_used=50):
    h_ref, s_ref = ref.read_gi()
    ill_ref = ref.read_plane(L.PLANE_ILLUMINANCE)
    assert int((h_ref[:, 0] != 0).sum()) > min_used and int((s_ref["direction"] < 6).sum()) > min_used
    for r, p in enumerate(ranks):
        h, s = p.read_gi()
        assert h.shape == h_ref.shape and s.shape == s_ref.shape
        assert np.array_equal(h, h_ref), f"rank {r}: hash differs in {int((h != h_ref).any(axis=1).sum())} entries"
        assert np.array_equal(s.view(np.uint32), s_ref.view(np.uint32)), f"rank {r}: surfel pool differs"
        assert np.array_equal(p.read_plane(L.PLANE_ILLUMINANCE).view(np.uint16), ill_ref.view(np.uint16)), f"rank {r}: illuminance differs"


@pytest.mark.parametrize("first,then", [(SMALL, LARGE), (LARGE, SMALL)], ids=["grow", "shrink"])
@pytest.mark.parametrize("world", [3, 1])
def test_configure_gi_after_a_sharded_trace(first, then, world):
    """Two sharded frames, configure_gi to other sizes, three more: the staging arrays of the first trace were sized for the first pool,
    the later traces need them sized for the second (grow: 8197 slots against 77 x 64 = 4928 staged), and the result is the fresh
    pipeline's."""
    if first == SMALL:
        assert then[1] > stage_slots(first[1])   # the later traces cross the first staging allocation
    rig = Rig()
    ranks, comms = group(rig, first, world)
    ref0 = rig.pipe(first)
    for f in (1, 2):
        rig.sharded_frame(ranks, comms, f)
        rig.frame(ref0, f)
    assert_same_gi(ranks, ref0)
    for p in ranks:
        p.configure_gi(*then)
    ref = rig.pipe(then)
    for f in (3, 4, 5):
        rig.sharded_frame(ranks, comms, f)
        rig.frame(ref, f)
    assert_same_gi(ranks, ref)


@pytest.mark.parametrize("world", [3, 1])
def test_configure_gi_between_trace_and_exchange_cancels_the_trace(world):
    """configure_gi after step 6a: the trace's permutation lived in the buffers just re-made -- the completion is refused with
    NOT_READY ("nothing pending") instead of running against them, and the next frames are the fresh pipeline's."""
    rig = Rig()
    ranks, comms = group(rig, SMALL, world)
    for f in (1, 2):
        rig.sharded_frame(ranks, comms, f)
    rig.trace(ranks, 3)
    for p in ranks:
        p.configure_gi(*LARGE)
    refused_completion(rig, ranks, comms, 3)
    ref = rig.pipe(LARGE)
    for f in (4, 5):
        rig.sharded_frame(ranks, comms, f)
        rig.frame(ref, f)
    assert_same_gi(ranks, ref)


@pytest.mark.parametrize("world", [3, 1])
def test_clear_between_trace_and_exchange_cancels_the_trace(world):
    """clear() after step 6a drops the trace (NOT_READY for its completion) and keeps the hash and the pool: the frame's surfel pass
    run again, then one more frame, equal the pipeline that never traced it sharded."""
    rig = Rig()
    ranks, comms = group(rig, SMALL, world)
    ref = rig.pipe(SMALL)
    for f in (1, 2):
        rig.sharded_frame(ranks, comms, f)
        rig.frame(ref, f)
    rig.trace(ranks, 3)
    for p in ranks:
        p.clear()
    refused_completion(rig, ranks, comms, 3)
    for r, p in enumerate(ranks):   # the surfel pass of frame 3 again, sharded and completed
        rig.render(p, SURF | L.PASS_GI_SHARDED, 3, surfel_shard=(r, world))
    rig.complete(ranks, comms, 3)
    rig.render(ref, PIX, 3)
    ref.clear()
    rig.render(ref, SURF, 3)
    rig.sharded_frame(ranks, comms, 4)
    rig.frame(ref, 4)
    assert_same_gi(ranks, ref)


def test_refused_exchange_leaves_the_trace_pending():
    """Step 6b refused -- the ranks' pipelines handed to each other's communicators, or the ranks disagreeing about the frame --
    is INVALID_ARGUMENT and leaves every rank's trace pending: the correct exchange then completes the frame."""
    rig = Rig()
    world = 3
    ranks, comms = group(rig, SMALL, world)
    ref = rig.pipe(SMALL)
    for f in (1, 2):
        rig.sharded_frame(ranks, comms, f)
        rig.frame(ref, f)
    rig.trace(ranks, 3)
    rig.frame(ref, 3)
    for r in range(world - 1):
        comms[r].gi_surfel_exchange(ranks[(r + 1) % world], 3)
    refused(L.ERR_INVALID_ARGUMENT, comms[world - 1].gi_surfel_exchange, ranks[0], 3)   # a trace made for another rank
    for r in range(world - 1):
        comms[r].gi_surfel_exchange(ranks[r], 3)
    refused(L.ERR_INVALID_ARGUMENT, comms[world - 1].gi_surfel_exchange, ranks[world - 1], 4)   # another frame
    two = api.Comm.local(rig.ctx, 2)
    two[0].gi_surfel_exchange(ranks[0], 3)
    refused(L.ERR_INVALID_ARGUMENT, two[1].gi_surfel_exchange, ranks[1], 3)   # a communicator of another world size
    rig.complete(ranks, comms, 3)
    rig.sharded_frame(ranks, comms, 4)
    rig.frame(ref, 4)
    assert_same_gi(ranks, ref)


@pytest.mark.parametrize("world", [3, 1])
def test_second_trace_before_the_exchange_is_refused(world):
    """A pending trace refuses the pipeline's next GI pass -- a second sharded trace, an unsharded surfel pass, a final gather -- with
    NOT_READY and is still completed correctly afterwards."""
    rig = Rig()
    ranks, comms = group(rig, SMALL, world)
    ref = rig.pipe(SMALL)
    for f in (1, 2):
        rig.sharded_frame(ranks, comms, f)
        rig.frame(ref, f)
    rig.trace(ranks, 3)
    rig.frame(ref, 3)
    refused(L.ERR_NOT_READY, rig.render, ranks[0], SURF | L.PASS_GI_SHARDED, 3, surfel_shard=(0, world))
    refused(L.ERR_NOT_READY, rig.render, ranks[0], SURF | L.PASS_GI_SHARDED, 4, surfel_shard=(0, world))
    refused(L.ERR_NOT_READY, rig.render, ranks[0], SURF, 3)
    refused(L.ERR_NOT_READY, rig.render, ranks[0], PIX, 4)
    rig.complete(ranks, comms, 3)
    rig.sharded_frame(ranks, comms, 4)
    rig.frame(ref, 4)
    assert_same_gi(ranks, ref)


def test_sharded_trace_without_the_ordered_apply_is_refused():
    """Step 6a asks for DUST_PASS_GI_ORDERED (its completion applies in surfel order whatever the frame asked for): without it the call
    is INVALID_ARGUMENT, nothing is left pending, and the frame's unsharded surfel pass that follows is unaffected."""
    rig = Rig()
    p, ref = rig.pipe(SMALL), rig.pipe(SMALL)
    for f in (1, 2):
        rig.frame(p, f)
        rig.frame(ref, f)
    rig.render(p, PIX, 3)
    for world in (1, 3):
        refused(L.ERR_INVALID_ARGUMENT, rig.render, p, L.PASS_SURFEL | L.PASS_GI_SHARDED, 3, surfel_shard=(0, world))
    refused(L.ERR_NOT_READY, p.gi_surfel_finish, 3)
    rig.render(p, SURF, 3)
    rig.render(ref, PIX, 3)
    rig.render(ref, SURF, 3)
    rig.frame(p, 4)
    rig.frame(ref, 4)
    assert_same_gi([p], ref)


@pytest.mark.parametrize("world", [3, 1])
def test_write_gi_while_a_trace_is_pending_is_refused(world):
    """write_gi between 6a and 6b is NOT_READY (the completion would overwrite the pool it restores and stamp the hash over it);
    read_gi works; the trace completes as if nothing had been asked, and write_gi works again afterwards."""
    rig = Rig()
    ranks, comms = group(rig, SMALL, world)
    ref = rig.pipe(SMALL)
    for f in (1, 2):
        rig.sharded_frame(ranks, comms, f)
        rig.frame(ref, f)
    saved = ranks[0].read_gi()
    rig.trace(ranks, 3)
    rig.frame(ref, 3)
    h, s = ranks[0].read_gi()
    assert h.shape == saved[0].shape and s.shape == saved[1].shape
    for p in ranks:
        refused(L.ERR_NOT_READY, p.write_gi, *saved)
    rig.complete(ranks, comms, 3)
    rig.sharded_frame(ranks, comms, 4)
    rig.frame(ref, 4)
    assert_same_gi(ranks, ref)
    ranks[0].write_gi(*saved)   # (nothing pending: restored)
    h, s = ranks[0].read_gi()
    assert np.array_equal(h, saved[0]) and np.array_equal(s.view(np.uint32), saved[1].view(np.uint32))
