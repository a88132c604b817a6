"""The C oracle's final gather and surfel pass (orc_pass_final_gather, orc_pass_surfel; both traversal modes) against the float64 witness of
tests/gi_witness.py: per pixel on the texels, entry by entry on the hash and the pool, each pass alone from a seeded state; the
conditions the cases must meet for that to mean something; and the witness itself against rays worked out by hand. CPU only."""
import numpy as np
import pytest

import gi_oracle as GO
import gi_witness as G
import oracle_lib as O
import radiance_witness as RW

F = np.float32


# ------------------------------------------------------------------ the witness against rays worked out by hand
def _bricks(origins, instances=((0.0, 0.0, 0.0),), albedo=(0x11111111,)):
    """bricks with one voxel each at the given origins, placed once per entry of `instances` (a translation) with that avg_albedo"""
    models = []
    for a in albedo:
        b = np.zeros(len(origins), O.BLOCK_DTYPE)
        for k, o in enumerate(origins):
            b["x"][k], b["y"][k], b["z"][k] = o
        b["mask"], b["material_ptr"], b["avg_albedo"] = 1 << 21, np.arange(len(origins)), a
        models.append((b, np.ones(len(origins), np.uint8)))
    inst = []
    for k, t in enumerate(instances):
        m = np.zeros((3, 4), F)
        m[:, :3], m[:, 3] = np.eye(3), t
        inst.append((k % len(models), m.reshape(12), None))
    return G.make_scene(models, np.zeros((256, 4), np.uint8), inst)


def test_brick_entered_just_before_and_just_after_eight():
    """a brick [4, 8] x [8, 12] x [12, 16]: a gather ray along +x that enters it at t = 7.99 goes through it, at t = 8.01 it hits; a surfel
    ray (tmin 0.1) hits both times; a second brick behind the first is what the first ray finds"""
    sc = _bricks([(4, 8, 12)])
    o = np.array([[4.0 - 7.99, 9.5, 13.25], [4.0 - 8.01, 9.5, 13.25]])
    d = np.array([[1.0, 0.0, 0.0]] * 2)
    g = G.rough_trace(sc, o, d, G.GATHER_TMIN, 10000.0)
    assert g.hit.tolist() == [False, True] and not g.undecided.any() and abs(g.t[1] - 8.01) < 1e-12 and g.reach[1] == 1.0
    s = G.rough_trace(sc, o, d, G.SURFEL_TMIN, G.SURFEL_TMAX)
    assert s.hit.tolist() == [True, True] and np.allclose(s.t, [7.99, 8.01], atol=1e-12)
    two = _bricks([(4, 8, 12), (20, 8, 12)])
    g2 = G.rough_trace(two, o, d, G.GATHER_TMIN, 10000.0)
    assert g2.hit.all() and g2.block.tolist() == [1, 0] and abs(g2.t[0] - 23.99) < 1e-12
    near = G.rough_trace(sc, np.array([[4.0 - 8.00001, 9.5, 13.25]]), d[:1], G.GATHER_TMIN, 10000.0)   # 1e-5 behind tmin: inside the band
    assert near.undecided[0]


def test_ray_that_starts_inside_a_brick():
    """the brick a ray starts in is entered before any tmin: it does not exist for the ray, whatever lies behind it does"""
    sc = _bricks([(4, 8, 12), (4, 8, 32)])
    o, d = np.array([[5.5, 9.5, 13.0]]), np.array([[0.0, 0.0, 1.0]])
    for tmin in (G.SURFEL_TMIN, G.GATHER_TMIN):
        r = G.rough_trace(sc, o, d, tmin, 10000.0)
        assert r.hit[0] and r.block[0] == 1 and r.t[0] == 19.0 and not r.undecided[0]
    assert not G.rough_trace(_bricks([(4, 8, 12)]), o, d, G.SURFEL_TMIN, 10000.0).hit[0]
    assert G.rough_trace(sc, o, d, G.SURFEL_TMIN, 10000.0, any_hit=True).hit[0]


def test_corner_graze_is_undecided_and_a_clear_pass_is_not():
    """a ray through the brick's edge x = 4, y = 12 cannot be decided; 1e-3 outside it is a miss, 1e-3 inside a hit whose interval is short"""
    sc = _bricks([(4, 8, 12)])
    d = np.array([[1.0, 1.0, 0.0]] * 3) / np.sqrt(2.0)
    o = np.array([[0.0, 8.0, 13.0], [0.0, 8.0 - 1e-3, 13.0], [0.0, 8.0 + 1e-3, 13.0]])       # the first passes through (4, 12) exactly
    r = G.rough_trace(sc, o, d, G.SURFEL_TMIN, 10000.0)
    assert r.undecided.tolist() == [True, False, False] and r.hit[1:].tolist() == [True, False]
    b = G.brick_surfel(sc, r, o, d)
    assert b.face[1] == 0 and not b.undecided[1]          # entered through the -x face: offset (-2, 2 - 1e-3, -1), x is the largest
    # a ray that enters at the corner (4, 8) and runs along the diagonal: a clear hit whose face cannot be decided
    o2 = np.array([[0.0, 4.0 + 1e-5, 13.0]])
    r2 = G.rough_trace(sc, o2, d[:1], G.SURFEL_TMIN, 10000.0)
    assert r2.undecided[0] or G.brick_surfel(sc, r2, o2, d[:1]).undecided[0]


def test_two_coincident_bricks_tie_to_the_lower_instance():
    sc = _bricks([(4, 8, 12)], instances=((1.0, 1.0, 1.0), (1.0, 1.0, 1.0)), albedo=(0x12345678, 0x87654321))
    o, d = np.array([[-10.0, 11.0, 15.5]]), np.array([[1.0, 0.0, 0.0]])
    r = G.rough_trace(sc, o, d, G.GATHER_TMIN, 10000.0)
    assert r.hit[0] and r.tie[0] and r.inst[0] == 0 and r.t[0] == 15.0 and not r.undecided[0]
    b = G.brick_surfel(sc, r, o, d)
    assert b.albedo[0] == 0x12345678 and b.face[0] == 0 and b.key[0].tolist() == [1, 2, 3] and b.pos32[0].tolist() == [7.0, 11.0, 15.0]
    # a third instance a hair in front wins outright; a hair behind it is a near tie the band cannot decide
    apart = _bricks([(4, 8, 12)], instances=((1.0, 1.0, 1.0), (1.0 - 1e-3, 1.0, 1.0)), albedo=(1, 2))
    assert G.rough_trace(apart, o, d, G.GATHER_TMIN, 10000.0).inst[0] == 1
    close = _bricks([(4, 8, 12)], instances=((1.0, 1.0, 1.0), (1.0 + 2e-5, 1.0, 1.0)), albedo=(1, 2))
    assert G.rough_trace(close, o, d, G.GATHER_TMIN, 10000.0).undecided[0]


def test_hash_get_by_hand():
    """three probes, no wrap, the stop at the first empty entry, the stamp"""
    cap = 8
    pos, face = np.array([[3, -7, 11]]), np.array([5])
    fp, loc = int(RW.key_fingerprint(pos, face)[0]), int(RW.key_location(pos, face, cap)[0])
    word = RW.logluv_encode(np.array([1.0, 2.0, 3.0], F))[0]
    for probe in range(3):
        t = np.zeros((cap + 2, 3), np.uint32)
        for q in range(probe):
            t[loc + q] = [0x1000 + q, 7, 9 | (3 << 16)]
        t[loc + probe] = [fp, word, 0x1234 | (403 << 16)]
        r = G.hash_get(t, cap, pos, face)
        assert r.found[0] and r.probe[0] == probe and r.slot[0] == loc + probe and r.count[0] == 403
        assert np.allclose(r.radiance[0], RW.logluv_decode(word))
        G.stamp(t, r.slot, 65537)
        assert t[loc + probe, 2] == (1 | (403 << 16)) and (t[:, 0] != 0).sum() == probe + 1
        if probe:
            t[loc + probe - 1, 0] = 0                        # an emptied probe in front of it
            assert not G.hash_get(t, cap, pos, face).found[0] and G.hash_get(t, cap, pos, face, stop_at_empty=False).found[0]
    t = np.zeros((cap + 2, 3), np.uint32)
    t[(loc + 3) % (cap + 2)] = [fp, word, 1 << 16]           # a fourth probe is never made
    t[loc:loc + 3, 0] = 0x77
    assert not G.hash_get(t, cap, pos, face).found[0]


def test_schedule_rule_in_integers_is_the_float32_comparison():
    noise, count = np.meshgrid(np.arange(256), np.concatenate([np.arange(0, 600), [65533, 65534, 65535]]), indexing="ij")
    f32 = (noise.astype(F) / F(255.0)) > (F(1.0) / (count + 2).astype(F))
    assert np.array_equal(G.schedules(noise, count), f32)


def test_clusters_and_supersession_by_hand():
    loc = np.array([0, 0, 0, 2, 5, 9, 10, 12, 14, 20, 22, 24, 25, 40, 41, 42, 43, 44])
    assert G.clusters(loc) == [(0, 4, "slab"), (4, 5, "one"), (5, 9, "slab"), (9, 13, "slab"), (13, 18, "wide")]
    assert G.clusters(np.array([3, 3, 3])) == [(0, 3, "one")] and G.clusters(np.array([0, 2, 4, 6])) == [(0, 4, "wide")]      # 6 - 0 + 3 > 8
    key = np.zeros((12, 3), np.int64)
    face = np.zeros(12, np.int64)
    dead = G.superseded(np.zeros(12, np.int64), key, face)
    assert dead.tolist() == [True] * 4 + [False] * 8
    face[8:] = 1                                               # another key at the same location, 8 places on: nothing is superseded
    assert not G.superseded(np.zeros(12, np.int64), key, face)[:4].any()


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("scene", ["A", "T"])
def test_seeded_hash_holds_what_the_cases_need(scene):
    cen = G.hash_census(scene)
    print(scene, cen)
    assert 0.35 <= cen["present"] / cen["keys"] <= 0.65 and cen["chained"] >= 20 and cen["holes"] >= 10 and cen["overflow"] == 2
    _, t = G.seeded_hash(scene)
    used = t[t[:, 0] != 0]
    assert set(G.COUNTS) <= set((used[:, 2] >> 16).tolist()) and len(set((used[:, 2] & 0xFFFF).tolist())) >= 4


@pytest.mark.parametrize("name", sorted(G.GATHER_CASES))
def test_gather_input_conditions(name):
    """the minima, the undecided share, and what the two rules decide: without the tmin of 8 and without the stop at an empty probe at
    least as many decided rays end differently as the minima count"""
    run = GO.gather(name)
    cond = G.assert_gather_conditions(name, run.wit)
    print(name, cond, "removed", run.removed)
    c, g = G.gather_inputs(name), run.wit
    off = lambda **kw: G.gather(G.witness_scene(c["scene"]), c["cam"], c["sky"], c["w"], c["h"], run.depth, run.normal, run.before, c["noise5"], c["noise0"],
                                c["rand"], c["frame_index"], c["table"], c["capacity"], c["pool_size"], **kw)
    dec = g.live & ~g.undecided
    no_tmin = off(tmin=G.SURFEL_TMIN)
    assert int((dec & ((no_tmin.hit != g.hit) | (no_tmin.t != g.t))).sum()) >= G.GATHER_MINIMA["near"]
    no_stop = off(stop_at_empty=False)
    assert int((dec & (no_stop.found != g.found)).sum()) >= G.GATHER_MINIMA["hole"]


@pytest.mark.parametrize("name", sorted(G.SURFEL_CASES))
def test_surfel_input_conditions(name):
    tr, ap, _ = G.surfel_witness(name)
    cond = G.surfel_conditions(tr)
    print(name, cond, "removed", G.surfel_inputs(name)["removed"])
    for k, least in G.SURFEL_MINIMA.items():
        assert cond[k] >= least, (name, k, cond)
    assert cond["undecided"] == 0 and G.flagged_share([ap]) <= G.FLAGGED_CAP
    dead = G.surfel_inputs(name)["pool"]["direction"] >= 6
    assert dead[9::10].all() and dead.sum() <= 0.13 * len(dead)            # dead slots interleaved


def apply_conditions(capacity):
    tr, ap, _ = G.apply_witness(capacity)
    rq = np.nonzero(tr.request & tr.live)[0]
    return G.apply_conditions(ap, rq, tr.key[rq], tr.face[rq]), tr


@pytest.mark.parametrize("capacity", G.APPLY_CAPACITIES)
def test_apply_input_conditions(capacity):
    cond, tr = apply_conditions(capacity)
    print(capacity, cond, "live", int(tr.live.sum()))
    assert not tr.hit.any() and not tr.undecided.any() and tr.request[tr.live].all()
    assert 1400 <= tr.live.sum() <= 1600 and tr.live[16384:].sum() >= 30
    G.assert_apply_conditions(capacity, cond)


def test_apply_flagged_share():
    assert G.flagged_share([G.apply_witness(c)[1] for c in G.APPLY_CAPACITIES]) <= G.FLAGGED_CAP


# ------------------------------------------------------------------ the oracle against the witness
@pytest.mark.parametrize("mode", sorted(GO.MODES))
@pytest.mark.parametrize("name", sorted(G.GATHER_CASES))
def test_oracle_gather_against_witness(name, mode):
    """texels the gather does not touch bit for bit; hit or miss, hit distance and radiance of every decided pixel; the hash (stamps only)
    and the pool entry by entry"""
    run, c = GO.gather(name, mode), G.gather_inputs(name)
    worst = G.check_gather_texels(run.before, run.after, run.wit, f"{name} {mode}")
    worst.update(G.check_gather_state(run.hash, c["pool"], run.pool, run.wit, f"{name} {mode}"))
    if name in G.STATE_LEVEL:
        assert worst["slots_compared"] == c["pool_size"] and not run.wit.maybe_stamped
    print(name, mode, worst)


@pytest.mark.parametrize("mode", sorted(GO.MODES))
@pytest.mark.parametrize("name", sorted(G.SURFEL_CASES))
def test_oracle_surfel_pass_against_witness(name, mode):
    run = GO.surfel(name, mode)
    _, ap, pool = G.surfel_witness(name)
    print(name, mode, G.check_hash(run.hash, ap, f"{name} {mode}"))
    G.check_pool(run.pool, pool, f"{name} {mode}")
    assert run.superseded == int(ap.superseded.sum())


@pytest.mark.parametrize("capacity", G.APPLY_CAPACITIES)
def test_oracle_apply_against_witness(capacity):
    run = GO.apply(capacity)
    _, ap, pool = G.apply_witness(capacity)
    print(capacity, G.check_hash(run.hash, ap, f"apply {capacity}"))
    G.check_pool(run.pool, pool, f"apply {capacity}")
    assert run.superseded == int(ap.superseded.sum())


def test_recorded_deviations_are_the_measurement():
    """GI_T_DEV and GI_RADIANCE_DEV: each at least what the oracle shows over all gather cases and both modes, and less than twice that"""
    worst = dict(t=0.0, radiance=0.0)
    for name in sorted(G.GATHER_CASES):
        for mode in sorted(GO.MODES):
            run = GO.gather(name, mode)
            got = G.check_gather_texels(run.before, run.after, run.wit, name, bounds=(np.inf, np.inf))
            for k in worst:
                worst[k] = max(worst[k], got[k])
    print(worst)
    for k, (measured, bound) in dict(t=(G.GI_T_DEV_MEASURED, G.GI_T_DEV), radiance=(G.GI_RADIANCE_DEV_MEASURED, G.GI_RADIANCE_DEV)).items():
        assert worst[k] <= bound <= 2.0 * measured, (k, worst[k], measured, bound)
        assert abs(worst[k] - measured) <= 0.005 * measured, (k, worst[k], measured)
    assert G.GI_DEVICE_T_DEV == G.GI_T_DEV and G.GI_DEVICE_RADIANCE_DEV == G.GI_RADIANCE_DEV + G.GI_DEVICE_RADIANCE_EXTRA
