"""The sweep witness (tests/sweep_witness.py) on hand-built scenes with known answers: the header's contract case by case -- a drop onto a
floor, sliding along it, a resting box moving down, starting inside with and without DUST_HIP_SWEEP_IGNORE_START, a grazing edge,
touching at t = 1, +-0 and subnormal delta components, flat and point boxes, and delta = 0 against the box queries' rule. No device."""
import numpy as np
import pytest

from dust_amd import api, scenes
from sweep_witness import SweepWitness, slab_times

F = np.float32


def floor_desc(transform=None):
    """one full brick (4 x 4 x 4 voxels) placed at world x, z in [-2, 2], y in [-4, 0]: a floor whose top is y = 0"""
    blocks = np.zeros(1, api.BLOCK_DTYPE)
    blocks["mask"] = np.uint64(0xFFFFFFFFFFFFFFFF)
    mats = (np.arange(64) % 7 + 1).astype(np.uint8)
    t = np.array([1, 0, 0, -2, 0, 1, 0, -4, 0, 0, 1, -2], F) if transform is None else np.asarray(transform, F)
    return scenes.SceneDesc([(blocks, mats)], np.zeros((256, 4), np.uint8), [(0, t)])


@pytest.fixture(scope="module")
def floor():
    return SweepWitness(floor_desc())


def bit(x, y, z):
    return x << 4 | y << 2 | z


def test_drop_onto_the_floor(floor):
    h = floor.exact((-0.5, 1.0, -0.5), (0.5, 3.0, 0.5), (0.0, -2.0, 0.0))
    assert h["t"] == F(0.5) and h["instance"] == 0 and h["block"] == 0
    assert h["voxel"] == bit(1, 3, 1) and list(h["xyz"]) == [1, 3, 1]      # (the lowest bit of the four voxels under the box)
    assert list(h["normal"]) == [0.0, 1.0, 0.0]
    assert h["palette"] == bit(1, 3, 1) % 7 + 1


def test_sliding_along_the_floor_is_a_miss(floor):
    h = floor.exact((-0.5, 0.0, -0.5), (0.5, 2.0, 0.5), (3.0, 0.0, 1.0))
    assert h["t"] == 1.0 and h["instance"] == 0xFFFFFFFF and h.tobytes()[8:] == bytes(24)


def test_resting_box_moving_down_hits_at_zero_with_normal_up(floor):
    h = floor.exact((-0.5, 0.0, -0.5), (0.5, 2.0, 0.5), (0.0, -1.0, 0.0))
    assert h["t"] == 0.0 and not np.signbit(h["t"]) and list(h["normal"]) == [0.0, 1.0, 0.0]


def test_starting_inside(floor):
    lo, hi, d = (-0.5, -1.5, -0.5), (0.5, -0.5, 0.5), (1.0, 0.0, 0.0)
    h = floor.exact(lo, hi, d)
    assert h["t"] == 0.0 and list(h["normal"]) == [0.0, 0.0, 0.0] and h["instance"] == 0
    g = floor.exact(lo, hi, d, ignore_start=True)      # the voxels ahead, at x in [1, 2]: entered at t = 0.5 through their -x face
    assert g["t"] == F(0.5) and list(g["normal"]) == [-1.0, 0.0, 0.0] and g["xyz"][0] == 3
    # moving out of the floor with IGNORE_START: nothing ahead, a miss
    assert floor.exact(lo, hi, (0.0, 2.0, 0.0), ignore_start=True)["instance"] == 0xFFFFFFFF


def test_grazing_edge_is_not_a_hit(floor):
    # the box's left face reaches x = 2 exactly when its bottom leaves y = 0: T_in == T_out
    assert floor.exact((3.0, -1.0, -0.5), (4.0, 0.0, 0.5), (-2.0, 2.0, 0.0))["instance"] == 0xFFFFFFFF
    # a hair lower it is a hit
    assert floor.exact((3.0, -1.25, -0.5), (4.0, -0.25, 0.5), (-2.0, 2.0, 0.0))["t"] == F(0.5)


def test_touching_at_one_is_not_a_hit(floor):
    assert floor.exact((-0.5, 2.0, -0.5), (0.5, 3.0, 0.5), (0.0, -2.0, 0.0))["instance"] == 0xFFFFFFFF
    assert floor.exact((-0.5, 2.0, -0.5), (0.5, 3.0, 0.5), (0.0, -2.5, 0.0))["t"] == F(0.8)


def test_signed_zero_and_subnormal_delta(floor):
    want = floor.exact((-0.5, 1.0, -0.5), (0.5, 3.0, 0.5), (0.0, -2.0, 0.0))
    for d in ((-0.0, -2.0, 0.0), (0.0, -2.0, -0.0), (1e-45, -2.0, 0.0), (-1e-45, -2.0, 1e-40)):
        h = floor.exact((-0.5, 1.0, -0.5), (0.5, 3.0, 0.5), d)
        assert h.tobytes() == want.tobytes(), d
    # a subnormal component is a moving axis: its slab quotients overflow to +-inf, not NaN
    e, x = slab_times(np.array([1.0], F), np.array([2.0], F), F(-0.5), F(0.5), F(1e-45))
    assert e[0] == np.inf and x[0] == np.inf


def test_flat_and_point_boxes(floor):
    h = floor.exact((0.25, 1.0, 0.25), (0.25, 1.0, 0.25), (0.0, -2.0, 0.0))    # a point: one voxel per resting axis
    assert h["t"] == F(0.5) and h["voxel"] == bit(2, 3, 2) and list(h["normal"]) == [0.0, 1.0, 0.0]
    h = floor.exact((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, -2.0, 0.0))          # on an integer plane: the voxel above it on the axis
    assert h["voxel"] == bit(2, 3, 2)
    h = floor.exact((-1.5, 1.0, 0.25), (1.5, 1.0, 0.25), (0.0, -2.0, 0.0))       # flat in y and z
    assert h["t"] == F(0.5) and h["voxel"] == bit(0, 3, 2)
    # a flat box lying on the floor's top plane moving sideways: a < lo fails for the top voxels, a miss
    assert floor.exact((-1.0, 0.0, -1.0), (1.0, 0.0, 1.0), (1.0, 0.0, 0.0))["instance"] == 0xFFFFFFFF


def test_zero_delta_is_the_box_rule(floor):
    inside = floor.exact((-0.5, -1.5, -0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 0.0))
    assert inside["t"] == 0.0 and inside["instance"] == 0 and list(inside["normal"]) == [0.0, 0.0, 0.0]
    assert floor.exact((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5), (0.0, 0.0, 0.0))["instance"] == 0xFFFFFFFF   # touching
    assert floor.exact((2.0, -1.0, 0.0), (2.0, -1.0, 0.0), (0.0, 0.0, 0.0))["instance"] == 0xFFFFFFFF   # a point on the +x face
    assert floor.exact((-2.0, -1.0, 0.0), (-2.0, -1.0, 0.0), (0.0, 0.0, 0.0))["instance"] == 0          # ... on the -x face
    # IGNORE_START: T_in = -inf with no moving axis, never a hit
    assert floor.exact((-0.5, -1.5, -0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 0.0), ignore_start=True)["instance"] == 0xFFFFFFFF


def test_degenerate_sweeps_miss(floor):
    for lo, hi, d in (((np.nan, 0, 0), (1, 1, 1), (0, -1, 0)), ((0, 0, 0), (1, 1, 1), (0, np.inf, 0)), ((1, 0, 0), (0, 1, 1), (0, -1, 0))):
        assert floor.exact(lo, hi, d)["instance"] == 0xFFFFFFFF


def test_mirrored_and_scaled_instance():
    # mirrored in x and scaled by 2 in y: world x in [-4, 0] (model x = 0 is world [-1, 0]), y in [-8, 0]
    w = SweepWitness(floor_desc([-1, 0, 0, 0, 0, 2, 0, -8, 0, 0, 1, -2]))
    h = w.exact((-0.5, 1.0, -0.5), (-0.25, 2.0, 0.5), (0.0, -4.0, 0.0))
    assert h["t"] == F(0.25) and list(h["xyz"]) == [0, 3, 1] and list(h["normal"]) == [0.0, 1.0, 0.0]
    h = w.exact((1.0, -3.0, 0.1), (2.0, -2.0, 0.2), (-2.0, 0.0, 0.0))           # into the +x face: model x = 0 faces +x
    assert h["t"] == F(0.5) and h["xyz"][0] == 0 and list(h["normal"]) == [1.0, 0.0, 0.0]


def test_tolerance_witness_agrees_on_the_floor(floor):
    # the float64 SAT of the shrunk and grown box brackets the exact answer on an axis-aligned scene
    lo, hi, d = (-0.5, 1.0, -0.5), (0.5, 3.0, 0.5), (0.3, -2.0, 0.1)
    t = floor.exact(lo, hi, d)["t"]
    inner, outer = floor.contact_times(lo, hi, d, -1.0), floor.contact_times(lo, hi, d, 1.0)
    assert min(max(c[3], 0.0) for c in outer) <= t <= min(max(c[3], 0.0) for c in inner)
