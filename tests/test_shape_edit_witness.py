"""The shape-edit witness (tests/shape_edit_witness.py) on hand-built cases whose answers are worked out here, not computed: what
the GPU tests then hold dust_hip_model_edit_shapes to."""
import numpy as np

import shape_edit_witness as W
from shape_edit_witness import BOX, CAPSULE, CARVE, FILL, PAINT, PLACE, SPHERE


def count(s):
    return int(W.coverage(s)[1].sum())


def test_sphere_boundary_is_inclusive():
    """r = 5 around a voxel centre: the integer offsets with x^2 + y^2 + z^2 <= 25 -- 515 of them, 30 at distance exactly 5
    (6 of the (5,0,0) type, 24 of the (3,4,0) type); r = 4.99 loses exactly those"""
    c = (100.5, 100.5, 100.5)
    inside = W.covered_voxels(W.shape(SPHERE, c, radius=5.0))
    assert len(inside) == 515
    assert (103, 104, 100) in inside and (105, 100, 100) in inside and (100, 96, 97) in inside
    assert (103, 104, 101) not in inside and (106, 100, 100) not in inside
    smaller = W.covered_voxels(W.shape(SPHERE, c, radius=4.99))
    assert len(smaller) == 485 and smaller < inside
    assert (103, 104, 100) not in smaller and (105, 100, 100) not in smaller and (104, 102, 102) in smaller   # 16 + 4 + 4 = 24


def test_box_bounds_on_a_centre_are_included():
    got = W.covered_voxels(W.shape(BOX, (10.5, 20.5, 30.5), (12.5, 20.5, 31.5)))
    assert got == {(x, 20, z) for x in (10, 11, 12) for z in (30, 31)}
    # lo == hi on a centre: one layer; between two centres: nothing
    assert W.covered_voxels(W.shape(BOX, (0.0, 7.5, 0.0), (4.0, 7.5, 2.0))) == {(x, 7, z) for x in range(4) for z in range(2)}
    assert count(W.shape(BOX, (0.0, 7.25, 0.0), (4.0, 7.25, 2.0))) == 0
    assert W.covered_voxels(W.shape(BOX, (3.5, 4.5, 5.5), (3.5, 4.5, 5.5))) == {(3, 4, 5)}
    # just short of a centre on either end (the neighbours of 12.5 in float32)
    lo, hi = np.nextafter(np.float32(10.5), np.float32(11)), np.nextafter(np.float32(12.5), np.float32(12))
    assert W.covered_voxels(W.shape(BOX, (lo, 0.0, 0.0), (hi, 1.0, 1.0))) == {(11, 0, 0)}


def test_degenerate_capsule_is_the_sphere():
    for c, r in (((100.5, 100.5, 100.5), 5.0), ((17.3, 40.9, 8.2), 6.7), ((1.0, 2.0, 3.0), 0.9)):
        assert W.covered_voxels(W.shape(CAPSULE, c, c, radius=r)) == W.covered_voxels(W.shape(SPHERE, c, radius=r))
    assert count(W.shape(SPHERE, (100.5, 100.5, 100.5), radius=0.0)) == 1      # the one centre it sits on
    assert count(W.shape(SPHERE, (100.0, 100.5, 100.5), radius=0.0)) == 0


def test_axis_capsule_is_a_cylinder_plus_caps():
    """segment (50.5 .. 58.5, 60.5, 70.5), r = 2: nine slices along the segment, each the 13 offsets with y^2 + z^2 <= 4; beyond
    either end one slice with y^2 + z^2 <= 3 (9 offsets) and one with the axis voxel alone: 9 * 13 + 2 * (9 + 1) = 137"""
    got = W.covered_voxels(W.shape(CAPSULE, (50.5, 60.5, 70.5), (58.5, 60.5, 70.5), radius=2.0))
    assert len(got) == 137
    for x, n in ((47, 0), (48, 1), (49, 9), (50, 13), (54, 13), (58, 13), (59, 9), (60, 1), (61, 0)):
        assert sum(1 for v in got if v[0] == x) == n, x
    assert (54, 62, 70) in got and (54, 62, 71) not in got and (60, 60, 70) in got and (60, 61, 70) not in got
    # the same segment the other way round covers the same voxels
    assert W.covered_voxels(W.shape(CAPSULE, (58.5, 60.5, 70.5), (50.5, 60.5, 70.5), radius=2.0)) == got


def half_solid():
    """a 4^3 region whose lower half (z < 2) is solid in colour 5"""
    return {(x, y, z): 5 for x in range(4) for y in range(4) for z in range(2)}


def test_the_four_ops_on_a_half_solid_region():
    box = dict(a=(0.0, 0.0, 0.0), b=(4.0, 4.0, 4.0))
    region = [(x, y, z) for x in range(4) for y in range(4) for z in range(4)]
    vox, ch = W.apply(half_solid(), W.shapes(W.shape(BOX, op=CARVE, **box)))
    assert ch.tolist() == [32] and vox == {}
    vox, ch = W.apply(half_solid(), W.shapes(W.shape(BOX, op=FILL, palette=5, **box)))
    assert ch.tolist() == [32] and vox == {k: 5 for k in region}            # the solid half already has that colour
    vox, ch = W.apply(half_solid(), W.shapes(W.shape(BOX, op=FILL, palette=9, **box)))
    assert ch.tolist() == [64] and vox == {k: 9 for k in region}
    vox, ch = W.apply(half_solid(), W.shapes(W.shape(BOX, op=PAINT, palette=9, **box)))
    assert ch.tolist() == [32] and vox == {k: 9 for k in half_solid()}
    vox, ch = W.apply(half_solid(), W.shapes(W.shape(BOX, op=PAINT, palette=5, **box)))
    assert ch.tolist() == [0] and vox == half_solid()
    vox, ch = W.apply(half_solid(), W.shapes(W.shape(BOX, op=PLACE, palette=9, **box)))
    assert ch.tolist() == [32] and vox == {k: (5 if k[2] < 2 else 9) for k in region}
    # the three that count nothing
    solid = dict(a=(0.0, 0.0, 0.0), b=(4.0, 4.0, 2.0))
    empty = dict(a=(0.0, 0.0, 2.0), b=(4.0, 4.0, 4.0))
    for s in (W.shape(BOX, op=FILL, palette=5, **solid), W.shape(BOX, op=PLACE, palette=9, **solid), W.shape(BOX, op=CARVE, **empty),
              W.shape(BOX, op=PAINT, palette=9, **empty)):
        vox, ch = W.apply(half_solid(), W.shapes(s))
        assert ch.tolist() == [0] and vox == half_solid()
    # palette 0 and 254 are colours like any other
    vox, ch = W.apply({}, W.shapes(W.shape(BOX, (0, 0, 0), (1, 1, 1), op=FILL, palette=0), W.shape(BOX, (1, 0, 0), (2, 1, 1), op=PLACE, palette=254)))
    assert ch.tolist() == [1, 1] and vox == {(0, 0, 0): 0, (1, 0, 0): 254}


def test_order_matters_and_equals_sequential_application():
    one = W.shape(BOX, (0.0, 0.0, 0.0), (4.0, 2.0, 1.0), op=FILL, palette=1)     # 4 x 2 x 1 = 8 voxels
    two = W.shape(SPHERE, (2.0, 2.0, 0.5), radius=1.0, op=FILL, palette=2)        # the centres (1.5|2.5, 1.5|2.5, 0.5): 4 voxels, 2 in the box
    ball = {(1, 1, 0), (2, 1, 0), (1, 2, 0), (2, 2, 0)}
    assert W.covered_voxels(two) == ball
    ab, ch_ab = W.apply({}, W.shapes(one, two))
    ba, ch_ba = W.apply({}, W.shapes(two, one))
    assert ch_ab.tolist() == [8, 4] and ch_ba.tolist() == [4, 8]
    assert ab != ba
    assert {k for k, v in ab.items() if v == 2} == ball and {k for k, v in ba.items() if v == 2} == {(1, 2, 0), (2, 2, 0)}
    for first, second, both in ((one, two, ab), (two, one, ba)):
        step, _ = W.apply({}, W.shapes(first))
        step, _ = W.apply(step, W.shapes(second))
        assert step == both
    # a carve between two fills: the second fill counts the carved voxels again
    _, ch = W.apply({}, W.shapes(one, W.shape(BOX, (0.0, 0.0, 0.0), (2.0, 2.0, 1.0), op=CARVE), one))
    assert ch.tolist() == [8, 4, 4]


def test_shapes_that_cover_nothing():
    nan, inf = float("nan"), float("inf")
    full = {(x, y, z): 3 for x in range(3) for y in range(3) for z in range(3)}
    nothing = [
        W.shape(BOX, (nan, 0, 0), (3, 3, 3)), W.shape(BOX, (0, 0, 0), (3, inf, 3)), W.shape(BOX, (0, -inf, 0), (3, 3, 3)),
        W.shape(BOX, (2, 0, 0), (1, 3, 3)), W.shape(BOX, (0, 0, 2.5), (3, 3, 1.5)),
        W.shape(SPHERE, (1.5, nan, 1.5), radius=2), W.shape(SPHERE, (1.5, 1.5, 1.5), radius=nan), W.shape(SPHERE, (1.5, 1.5, 1.5), radius=inf),
        W.shape(SPHERE, (1.5, 1.5, 1.5), radius=-1.0), W.shape(SPHERE, (1.5, 1.5, 1.5), radius=-1e-30),
        W.shape(SPHERE, (65537.0, 1.5, 1.5), radius=65536.0), W.shape(SPHERE, (1.5, -65540.0, 1.5), radius=65536.0),
        W.shape(SPHERE, (1.5, 1.5, 1.5), radius=65537.0), W.shape(SPHERE, (1.5, 1.5, 1.5), radius=1e30),
        W.shape(CAPSULE, (1.5, 1.5, 1.5), (1.5, inf, 1.5), radius=1), W.shape(CAPSULE, (inf, 1.5, 1.5), (1.5, 1.5, 1.5), radius=1),
        W.shape(CAPSULE, (1.5, 1.5, 1.5), (1.5, 1.5, 1.5), radius=nan), W.shape(CAPSULE, (1.5, 1.5, 1.5), (2.5, 1.5, 1.5), radius=-0.5),
        W.shape(CAPSULE, (1.5, 1.5, 1.5), (1e5, 1.5, 1.5), radius=1), W.shape(CAPSULE, (1.5, -1e5, 1.5), (1.5, 1.5, 1.5), radius=1),
        W.shape(CAPSULE, (1.5, 1.5, 1.5), (2.5, 1.5, 1.5), radius=70000.0),
    ]
    for s in nothing:
        assert W.covers_nothing(s), s
        assert count(s) == 0
    vox, ch = W.apply(full, W.shapes(*nothing))      # (not an error: changed is 0 for each)
    assert vox == full and not ch.any() and len(ch) == len(nothing)
    # exactly at the limit is still a shape; a field the kind ignores is ignored; radius -0 is a radius of 0
    reg, m = W.coverage(W.shape(SPHERE, (65536.0, 0.5, 0.5), radius=65536.0))
    assert reg == (slice(0, 256),) * 3 and m[0, 0, 0] and m[1, 255, 255] and not m[0, 255, 255]
    assert count(W.shape(CAPSULE, (-65536.0, 0.5, 0.5), (65536.0, 0.5, 0.5), radius=0.0)) == 256
    assert count(W.shape(BOX, (0, 0, 0), (3, 3, 3), radius=nan)) == 27 and count(W.shape(BOX, (0, 0, 0), (3, 3, 3), radius=-1.0)) == 27
    assert count(W.shape(SPHERE, (1.5, 1.5, 1.5), (nan, inf, 1e30), radius=1.0)) == 7
    assert count(W.shape(SPHERE, (1.5, 1.5, 1.5), radius=-0.0)) == 1
    assert count(W.shape(BOX, (-1e30, -1e30, -1e30), (1e30, 1e30, 1e30))) == 256 ** 3


def test_shapes_are_clipped_to_the_tree():
    assert W.covered_voxels(W.shape(BOX, (-5.0, -5.0, -5.0), (1.5, 1.5, 1.5))) == {(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)}
    assert W.covered_voxels(W.shape(BOX, (254.5, 254.5, 254.5), (1e30, 300.0, 256.0))) == {(x, y, z) for x in (254, 255) for y in (254, 255) for z in (254, 255)}
    assert count(W.shape(BOX, (256.0, 0.0, 0.0), (300.0, 10.0, 10.0))) == 0 and count(W.shape(BOX, (-9.0, 0.0, 0.0), (0.25, 10.0, 10.0))) == 0
    assert W.covered_voxels(W.shape(SPHERE, (-0.5, 0.5, 0.5), radius=1.0)) == {(0, 0, 0)}
    assert W.covered_voxels(W.shape(SPHERE, (256.5, 255.5, 0.5), radius=1.0)) == {(255, 255, 0)}
    assert count(W.shape(SPHERE, (0.0, 0.0, 0.0), radius=2.0)) == 4      # centres (.5,.5,.5) and the three (1.5,.5,.5): 0.75 and 2.75 <= 4 < 4.75
    assert W.covered_voxels(W.shape(CAPSULE, (-5.5, 3.5, 3.5), (2.5, 3.5, 3.5), radius=0.0)) == {(0, 3, 3), (1, 3, 3), (2, 3, 3)}
    assert count(W.shape(SPHERE, (128.0, 128.0, 128.0), radius=1000.0)) == 256 ** 3
    vox, ch = W.apply({(0, 0, 0): 1, (255, 255, 255): 2}, W.shapes(W.shape(BOX, (-1e30,) * 3, (1e30,) * 3, op=CARVE), W.shape(BOX, (-1.0,) * 3, (2.0,) * 3, op=FILL, palette=7)))
    assert ch.tolist() == [2, 8] and len(vox) == 8 and set(vox.values()) == {7}


def test_the_shape_limit_and_the_refusals():
    ok = np.zeros(W.MAX_SHAPES, W.SHAPE_DTYPE)
    assert W.MAX_SHAPES == 65536 and not W.refused(ok) and W.refused(np.zeros(W.MAX_SHAPES + 1, W.SHAPE_DTYPE))
    assert W.refused(W.shapes(W.shape(3, (0, 0, 0)))) and W.refused(W.shapes(W.shape(BOX, (0, 0, 0), op=4)))
    assert W.refused(W.shapes(W.shape(BOX, (0, 0, 0), op=FILL, palette=255))) and W.refused(W.shapes(W.shape(BOX, (0, 0, 0), op=PLACE, palette=-1)))
    assert not W.refused(W.shapes(W.shape(BOX, (0, 0, 0), op=CARVE, palette=999)))    # CARVE ignores the palette
    assert not W.refused(W.shapes(W.shape(BOX, (0, 0, 0), op=PAINT, palette=254)))
    assert W.SHAPE_DTYPE.itemsize == 48
