"""The relaxation of dust_amd/csrc/flood.hip (k_flood_seed, k_flood_relax and the host's pass loop) ported to numpy and run against the
witness: the worklists, the rule for whom a brick wakes, the step cap and the pass ceiling, with neighbour bricks read fresh and read
as they stood when the pass began (the two extremes of what a wavefront may see of a brick that is being relaxed beside it), the
listed bricks in a shuffled order. It checks the algorithm without a device; tests/test_gpu_flood.py checks the kernels."""
import numpy as np
import pytest

import flood_witness as W

U = W.UNREACHED
LX, LY, LZ = np.arange(64) >> 4, (np.arange(64) >> 2) & 3, np.arange(64) & 3      # a lane's voxel inside its brick


def emulate(grid, seeds, medium=W.EMPTY, palette=0, max_steps=W.MAX_STEPS, region=None, stale=False, rng=None):
    """(field, (passes, brick visits)): the host loop of dust_hip_model_flood around the port of k_flood_relax, a brick at a time"""
    ok = W.passable(grid, medium, palette, region)
    box = W.clip(region, grid.shape)
    field = np.full(grid.shape, U, np.int32)
    if box is None:
        return field.astype(np.uint16), (0, 0)
    blo, bhi = box[0] >> 2, box[1] >> 2
    cur = []
    for s in seeds:
        s = tuple(int(v) for v in s)
        if ok[s]:
            field[s] = 0
            b = tuple(v >> 2 for v in s)
            if b not in cur:
                cur.append(b)
    passes = 0
    first = True
    visits = 0
    while cur and passes < max_steps + 1:
        passes += 1
        nxt = []
        snap = field.copy() if stale else field
        if rng is not None:
            rng.shuffle(cur)
        for (bx, by, bz) in cur:
            visits += 1
            sl = (slice(bx*4, bx*4+4), slice(by*4, by*4+4), slice(bz*4, bz*4+4))
            op = ok[sl].reshape(64)
            v0 = np.where(op, field[sl].reshape(64), U)
            def ext(axis):
                e = np.full(64, U, np.int64)
                for lane in range(64):
                    if not op[lane]:
                        continue
                    l = (LX[lane], LY[lane], LZ[lane])[axis]
                    p = [bx*4+LX[lane], by*4+LY[lane], bz*4+LZ[lane]]
                    if l == 0 and p[axis] > 0:
                        p[axis] -= 1
                        e[lane] = snap[tuple(p)]
                    elif l == 3 and p[axis] < 255:
                        p[axis] += 1
                        e[lane] = snap[tuple(p)]
                return e
            ex, ey, ez = ext(0), ext(1), ext(2)
            e = np.minimum(ex, np.minimum(ey, ez))
            v = v0.copy()
            m = op & (e + 1 <= max_steps)
            v[m] = np.minimum(v[m], e[m] + 1)
            for rnd in range(64):
                c = v.reshape(4, 4, 4)
                n = np.full((4, 4, 4), U, np.int64)
                n[1:] = np.minimum(n[1:], c[:-1])
                n[:-1] = np.minimum(n[:-1], c[1:])
                n[:, 1:] = np.minimum(n[:, 1:], c[:, :-1])
                n[:, :-1] = np.minimum(n[:, :-1], c[:, 1:])
                n[:, :, 1:] = np.minimum(n[:, :, 1:], c[:, :, :-1])
                n[:, :, :-1] = np.minimum(n[:, :, :-1], c[:, :, 1:])
                n = n.reshape(64)
                lower = op & (n + 1 <= max_steps) & (n + 1 < v)
                v = np.where(lower, n + 1, v)
                if not lower.any():
                    break
            else:
                assert False, "65th round wanted"
            dropped = v < v0
            f = field[sl].reshape(64).copy()
            f[dropped] = v[dropped]
            field[sl] = f.reshape(4, 4, 4)
            news = (dropped | (first & (v != U))) & (v + 1 <= max_steps)
            for axis, (ee, L) in enumerate(((ex, LX), (ey, LY), (ez, LZ))):
                for up in (0, 1):
                    if (news & (v + 1 < ee) & (L == (3 if up else 0))).any():
                        b = [bx, by, bz]
                        b[axis] += 1 if up else -1
                        if blo[axis] <= b[axis] <= bhi[axis] and tuple(b) not in nxt:
                            nxt.append(tuple(b))
        cur = nxt
        first = False
    return field.astype(np.uint16), (passes, visits)


def cases():
    grid, empty, solid = W.corridors()
    yield "corridor cut by the region", grid, [empty[0][0]], dict(region=((0, 0, 0), (25, 255, 255)))
    yield "corridor capped", grid, [empty[1][0]], dict(max_steps=12)
    yield "bars", grid, [r[0] for r in solid], dict(medium=W.SOLID)
    grid, path = W.brick_snake()
    yield "snake from both ends", grid, [path[0], path[-1]], dict(medium=W.MATERIAL, palette=8)
    grid, seed, _, _, _ = W.late_shortcut()
    yield "late shortcut", grid, [seed], dict(medium=W.SOLID)
    grid = np.zeros((W.EXTENT,) * 3, np.uint8)
    rng = np.random.default_rng(3)
    grid[5:19, 6:20, 7:21] = np.where(rng.random((14, 14, 14)) < 0.6, 2, 0)
    region = ((5, 6, 7), (18, 19, 20))
    seeds = np.argwhere(grid[5:19, 6:20, 7:21] == 0)[:3] + (5, 6, 7)
    yield "random fill", grid, seeds, dict(region=region)
    yield "random fill, capped", grid, seeds, dict(region=region, max_steps=7)
    yield "random fill, solid", grid, np.argwhere(grid)[:2], dict(medium=W.SOLID, region=region)
    yield "seed on the tree's corner", np.zeros((W.EXTENT,) * 3, np.uint8), [(255, 255, 255)], dict(max_steps=6)
    yield "empty region", grid, seeds, dict(region=((9, 0, 0), (8, 255, 255)))


@pytest.mark.parametrize("case", list(cases()), ids=lambda c: c[0])
def test_port_reaches_the_witness_fixed_point(case):
    _, grid, seeds, query = case
    want = W.steps(grid, seeds, **query)
    for stale in (False, True):
        got, (passes, visits) = emulate(grid, seeds, stale=stale, rng=np.random.default_rng(1), **query)
        assert np.array_equal(got, want), stale
        assert passes <= query.get("max_steps", W.MAX_STEPS) + 1 and visits <= passes * 64 ** 3
