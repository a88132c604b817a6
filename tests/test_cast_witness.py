"""tests/cast_witness.py (whole arrays, one placement at a time) against an independent reading of the header: a plain Python loop over
placements and, inside it, over the piece's voxels one by one, with the formulas of include/dust_hip.h written out. Small random pieces in
small trees (the witness takes the extent from the grid), all 48 orientations, all 27 steps, WALLS on and off, offsets that begin outside
the tree."""
import itertools

import numpy as np
import pytest

import cast_witness as W
from stamp_witness import all_orientations

EXTENT = 12


def by_the_header(dst, src, cast):
    """every placement 0..max_steps, every voxel: no clipping, no intervals"""
    extent = dst.shape[0]
    orient = int(cast["orient"])
    p = [(orient >> (2 * r)) & 3 for r in range(3)]
    g = [(orient >> (6 + r)) & 1 for r in range(3)]
    lo = [int(v) for v in cast["src_lo"]]
    hi = [int(v) for v in cast["src_hi"]]
    off = [int(v) for v in cast["offset"]]
    step = [int(v) for v in cast["step"]]
    max_steps = int(cast["max_steps"])
    walls = int(cast["flags"]) & W.WALLS
    piece = [(x, y, z) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1) if src[x, y, z]]
    for k in range(max_steps + 1):
        hit = []
        for s in piece:
            u = [hi[p[r]] - s[p[r]] if g[r] else s[p[r]] - lo[p[r]] for r in range(3)]
            d = [off[r] + k * step[r] + u[r] for r in range(3)]
            inside = all(0 <= v < extent for v in d)
            if (inside and dst[d[0], d[1], d[2]]) or (not inside and walls):
                hit.append((s[0] << 16 | s[1] << 8 | s[2], tuple(d), inside))
        if hit:
            key, contact, _ = min(hit)
            flags = W.HIT | (W.OVERLAP if k == 0 else 0) | (0 if all(h[2] for h in hit) else W.HIT_WALL)
            return (k - 1 if k else 0, flags, len(hit), len(piece), contact, key)
    return (max_steps, 0, 0, len(piece), (0, 0, 0), W.NO_KEY)


def as_tuple(h):
    return (int(h["steps"]), int(h["flags"]), int(h["contacts"]), int(h["voxels"]), tuple(int(v) for v in h["contact"]), int(h["src_key"]))


def grids(seed, fill=0.08):
    rng = np.random.default_rng(seed)
    dst = (rng.random((EXTENT,) * 3) < fill).astype(np.uint8) * 3
    src = (rng.random((EXTENT,) * 3) < 0.5).astype(np.uint8) * 5
    return rng, dst, src


STEPS = list(itertools.product((-1, 0, 1), repeat=3))


@pytest.mark.parametrize("walls", [0, W.WALLS])
def test_every_orientation_and_step_matches_the_header(walls):
    """48 orientations x 27 steps, the offsets drawn so that pieces begin inside, straddling the tree's faces and wholly outside it"""
    rng, dst, src = grids(7 + walls)
    orients = all_orientations()
    assert len(orients) == 48 and len(STEPS) == 27
    seen = {"miss": 0, "hit": 0, "overlap": 0, "wall": 0, "many": 0, "outside_start": 0}
    for orient in orients:
        for step in STEPS:
            lo = rng.integers(0, 6, 3)
            hi = lo + rng.integers(0, 4, 3)
            offset = rng.integers(0, EXTENT - 4, 3) if rng.random() < 0.5 else rng.integers(-8, EXTENT + 4, 3)
            c = W.records([offset], step, int(rng.integers(0, 30)), orient, walls, lo, hi)[0]
            want = by_the_header(dst, src, c)
            got = as_tuple(W.cast(dst, src, [c])[0])
            assert got == want, (orient, step, c)
            seen["miss"] += want[1] == 0
            seen["hit"] += want[1] & W.HIT and not want[1] & W.OVERLAP
            seen["overlap"] += bool(want[1] & W.OVERLAP)
            seen["wall"] += bool(want[1] & W.HIT_WALL)
            seen["many"] += want[2] > 1
            seen["outside_start"] += any(o + 3 < 0 or o >= EXTENT for o in offset)
    assert min(seen["miss"], seen["hit"], seen["overlap"], seen["many"], seen["outside_start"]) > 40, seen
    assert (seen["wall"] > 50) == bool(walls), seen


def test_degenerate_inputs():
    _, dst, src = grids(3)
    full = dict(src_lo=(0, 0, 0), src_hi=(3, 3, 3))
    # src_lo > src_hi, and an empty piece: no hit, voxels 0, steps = max_steps
    for c in (W.records([(2, 2, 2)], (0, -1, 0), 9, src_lo=(4, 0, 0), src_hi=(3, 5, 5))[0],):
        assert as_tuple(W.cast(dst, src, [c])[0]) == by_the_header(dst, src, c) == (9, 0, 0, 0, (0, 0, 0), W.NO_KEY)
    empty = np.zeros_like(src)
    c = W.records([(2, 2, 2)], (0, -1, 0), 9, flags=W.WALLS, **full)[0]
    assert as_tuple(W.cast(dst, empty, [c])[0]) == by_the_header(dst, empty, c) == (9, 0, 0, 0, (0, 0, 0), W.NO_KEY)
    # a zero step: every placement is placement 0
    solid = np.ones_like(dst)
    c = W.records([(2, 2, 2)], (0, 0, 0), 500, **full)[0]
    assert as_tuple(W.cast(solid, src, [c])[0]) == by_the_header(solid, src, c)
    assert as_tuple(W.cast(empty, src, [c])[0]) == by_the_header(empty, src, c)
    assert int(W.cast(empty, src, [c])[0]["steps"]) == 500


def test_offsets_at_the_int32_limits_answer_at_once():
    """no placement is examined that the piece cannot spend inside the tree; the contact wraps to its low 32 bits as the header says"""
    _, dst, src = grids(5)
    src[0, 0, 0] = 1
    far = [(2 ** 31 - 1, 3, 3), (-2 ** 31, 3, 3), (3, -2 ** 31, 2 ** 31 - 1)]
    for walls in (0, W.WALLS):
        c = W.records(far, (-1, 1, 0), W.MAX_STEPS, flags=walls, src_lo=(0, 0, 0), src_hi=(3, 3, 3))
        hits = W.cast(dst, src, c)
        if not walls:
            assert (hits["flags"] == 0).all() and (hits["steps"] == W.MAX_STEPS).all()
        else:
            assert (hits["flags"] == (W.HIT | W.OVERLAP | W.HIT_WALL)).all() and (hits["src_key"] == 0).all()
            assert hits["contact"].tolist() == [[2 ** 31 - 1, 3, 3], [-2 ** 31, 3, 3], [3, -2 ** 31, 2 ** 31 - 1]]
    wrapped = W.cast(dst, src, W.records([(2 ** 31 - 1, 3, 3)], (1, 0, 0), 5, orient=W.IDENTITY | 1 << 6, flags=W.WALLS, src_lo=(0, 0, 0), src_hi=(3, 0, 0)))[0]
    assert wrapped["src_key"] == 0 and wrapped["contact"].tolist() == [-2 ** 31 + 2, 3, 3]   # u = 3 on a flipped axis: 2^31 + 2, reduced
