"""tests/census_witness.py against plain Python loops on hand-built cases: the header's membership rule evaluated voxel by voxel with
numpy float32 scalars, and the record and the row built by counting. No device, no library."""
import math

import numpy as np

import census_witness as W
import shape_edit_witness as SW

F = np.float32


def contains(s, x, y, z):
    """the header's rule for one voxel centre, one float32 operation at a time"""
    c = [F(x) + F(0.5), F(y) + F(0.5), F(z) + F(0.5)]
    a, b, kind = [F(v) for v in s["a"]], [F(v) for v in s["b"]], int(s["kind"])
    if kind == SW.BOX:
        return all(a[r] <= c[r] <= b[r] for r in range(3))

    def dot(u, v):
        return F(F(F(u[0] * v[0]) + F(u[1] * v[1])) + F(u[2] * v[2]))
    rr = F(F(s["radius"]) * F(s["radius"]))
    ap = [F(c[r] - a[r]) for r in range(3)]
    if kind == SW.SPHERE:
        return bool(dot(ap, ap) <= rr)
    ab = [F(b[r] - a[r]) for r in range(3)]
    l = dot(ab, ab)
    h = F(0) if l == 0 else min(max(F(dot(ap, ab) / l), F(0)), F(1))
    q = [F(ap[r] - F(ab[r] * h)) for r in range(3)]
    return bool(dot(q, q) <= rr)


def dead(s):
    used = list(s["a"]) + ([] if int(s["kind"]) == SW.SPHERE else list(s["b"])) + ([] if int(s["kind"]) == SW.BOX else [s["radius"]])
    if not all(math.isfinite(float(v)) for v in used):
        return True
    if int(s["kind"]) == SW.BOX:
        return any(float(s["a"][r]) > float(s["b"][r]) for r in range(3))
    return float(s["radius"]) < 0 or any(abs(float(v)) > 65536.0 for v in used)


def loops(grid, s, lo, hi):
    """the census of one shape by visiting every voxel of the box lo..hi (inclusive, inside the tree; the caller picks one that holds the shape)"""
    covered = solid = 0
    row = [0] * 256
    blo, bhi, sums = [255] * 3, [0] * 3, [0] * 3
    if not dead(s):
        for x in range(lo[0], hi[0] + 1):
            for y in range(lo[1], hi[1] + 1):
                for z in range(lo[2], hi[2] + 1):
                    if not contains(s, x, y, z):
                        continue
                    covered += 1
                    row[int(grid[x, y, z])] += 1
                    if grid[x, y, z]:
                        solid += 1
                        for r, v in enumerate((x, y, z)):
                            blo[r], bhi[r], sums[r] = min(blo[r], v), max(bhi[r], v), sums[r] + v
    return covered, solid, blo, bhi, sums, row


def agree(grid, s, lo, hi):
    record, row = W.census_one(grid, s)
    covered, solid, blo, bhi, sums, want_row = loops(grid, s, lo, hi)
    assert (int(record["covered"]), int(record["solid"])) == (covered, solid), s
    assert record["lo"].tolist() == blo and record["hi"].tolist() == bhi and record["sum"].tolist() == sums, s
    assert row.tolist() == want_row and int(record["reserved0"]) == int(record["reserved1"]) == 0
    return record, row


def sample_grid():
    rng = np.random.default_rng(5)
    grid = np.zeros((256,) * 3, np.uint8)
    grid[0:24, 0:24, 0:24] = np.where(rng.random((24,) * 3) < 0.6, rng.integers(1, 256, (24,) * 3), 0)
    grid[244:256, 244:256, 244:256] = np.where(rng.random((12,) * 3) < 0.6, rng.integers(1, 7, (12,) * 3), 0)
    grid[7, 8, 9] = 42
    grid[4:8, 8:12, 12:16] = 3
    grid[5, 9, 13] = 0
    return grid


def test_one_voxel_and_one_brick():
    grid = sample_grid()
    record, row = agree(grid, SW.shape(SW.BOX, (7.0, 8.0, 9.0), (8.0, 9.0, 10.0)), (5, 6, 7), (10, 11, 12))
    assert (int(record["covered"]), int(record["solid"])) == (1, 1) and row[42] == 1 and row.sum() == 1
    assert record["lo"].tolist() == record["hi"].tolist() == record["sum"].tolist() == [7, 8, 9]
    record, row = agree(grid, SW.shape(SW.BOX, (4.0, 8.0, 12.0), (8.0, 12.0, 16.0)), (2, 6, 10), (9, 13, 17))      # exactly a brick
    assert (int(record["covered"]), int(record["solid"])) == (64, 63) and row[3] == 63 and row[0] == 1
    assert record["lo"].tolist() == [4, 8, 12] and record["hi"].tolist() == [7, 11, 15]
    assert record["sum"].tolist() == [16 * (4 + 5 + 6 + 7) - 5, 16 * (8 + 9 + 10 + 11) - 9, 16 * (12 + 13 + 14 + 15) - 13]


def test_radius_zero_on_and_off_a_centre():
    grid = sample_grid()
    record, row = agree(grid, SW.shape(SW.SPHERE, (7.5, 8.5, 9.5), radius=0.0), (5, 6, 7), (10, 11, 12))
    assert (int(record["covered"]), int(record["solid"])) == (1, 1) and row[42] == 1
    record, row = agree(grid, SW.shape(SW.SPHERE, (7.25, 8.5, 9.5), radius=0.0), (5, 6, 7), (10, 11, 12))
    assert record.tobytes() == W.zero_record().tobytes() and not row.any()
    record, row = agree(grid, SW.shape(SW.CAPSULE, (5.5, 9.5, 13.5), (5.5, 9.5, 13.5), radius=0.0), (3, 7, 11), (8, 12, 16))      # a == b on an empty voxel
    assert (int(record["covered"]), int(record["solid"])) == (1, 0) and row[0] == 1
    assert record["lo"].tolist() == [255] * 3 and record["hi"].tolist() == [0] * 3 and record["sum"].tolist() == [0] * 3


def test_half_outside_the_tree():
    grid = sample_grid()
    record, _ = agree(grid, SW.shape(SW.SPHERE, (-1.0, 5.5, 5.5), radius=4.0), (0, 0, 0), (6, 12, 12))
    assert 0 < int(record["covered"]) and record["lo"][0] == 0
    record, _ = agree(grid, SW.shape(SW.BOX, (250.0, 250.0, 250.0), (300.0, 300.0, 300.0)), (245, 245, 245), (255, 255, 255))
    assert int(record["covered"]) == 6 ** 3 and record["hi"].tolist() == [255] * 3
    record, _ = agree(grid, SW.shape(SW.CAPSULE, (252.0, 252.0, 252.0), (262.0, 258.0, 254.0), radius=2.5), (244, 244, 244), (255, 255, 255))
    assert 0 < int(record["solid"]) < int(record["covered"])
    record, row = agree(grid, SW.shape(SW.BOX, (300.0, 10.0, 10.0), (310.0, 20.0, 20.0)), (250, 8, 8), (255, 22, 22))      # wholly outside
    assert record.tobytes() == W.zero_record().tobytes() and not row.any()


def test_shapes_that_cover_nothing():
    grid = sample_grid()
    nan, inf = float("nan"), float("inf")
    for s in (SW.shape(SW.BOX, (nan, 1.0, 1.0), (5.0, 5.0, 5.0)), SW.shape(SW.BOX, (6.0, 1.0, 1.0), (5.0, 5.0, 5.0)),
              SW.shape(SW.SPHERE, (5.0, 5.0, 5.0), radius=nan), SW.shape(SW.SPHERE, (5.0, 5.0, 5.0), radius=-1.0),
              SW.shape(SW.CAPSULE, (5.0, 5.0, 5.0), (9.0, inf, 5.0), radius=1.0), SW.shape(SW.SPHERE, (5.0, 5.0, 5.0), radius=65537.0)):
        record, row = agree(grid, s, (0, 0, 0), (8, 8, 8))
        assert record.tobytes() == W.zero_record().tobytes() and not row.any()
    record, _ = agree(grid, SW.shape(SW.SPHERE, (5.5, 5.5, 5.5), (nan, inf, -inf), radius=1.0), (2, 2, 2), (9, 9, 9))      # a sphere ignores b
    assert int(record["covered"]) == 7


def test_invariants_of_rows_and_records():
    grid = sample_grid()
    rng = np.random.default_rng(6)
    shapes = SW.shapes(*[SW.shape(int(k), p, p + d, radius=float(r), op=int(op), palette=int(pal)) for k, p, d, r, op, pal in
                         zip(rng.integers(0, 3, 40), rng.uniform(-4.0, 26.0, (40, 3)), rng.uniform(0.0, 9.0, (40, 3)), rng.uniform(0.0, 5.0, 40),
                             rng.integers(0, 9, 40), rng.integers(-5, 400, 40))])      # (op and palette are not looked at, valid or not)
    assert not W.refused(shapes)
    records, counts = W.census(grid, shapes)
    assert counts.shape == (40, 256) and counts.dtype == np.uint32 and W.census(grid, shapes, tables=False)[1] is None
    assert np.array_equal(counts.sum(axis=1), records["covered"]) and np.array_equal(counts[:, 1:].sum(axis=1), records["solid"])
    none = records["solid"] == 0
    assert np.all(records["lo"][none] == 255) and np.all(records["hi"][none] == 0) and np.all(records["sum"][none] == 0)
    assert np.all(records["lo"][~none] <= records["hi"][~none]) and np.count_nonzero(~none) > 10
    for r in range(3):
        s = records["solid"][~none].astype(np.uint64)
        assert np.all(records["lo"][~none, r] * s <= records["sum"][~none, r]) and np.all(records["sum"][~none, r] <= records["hi"][~none, r] * s)
    plain = shapes.copy()
    plain["op"], plain["palette"], plain["reserved"] = 0, 0, 0
    again, _ = W.census(grid, plain)
    assert again.tobytes() == records.tobytes()
    # independence: the order does not matter and overlapping shapes each see every voxel
    back, back_counts = W.census(grid, shapes[::-1])
    assert back[::-1].tobytes() == records.tobytes() and np.array_equal(back_counts[::-1], counts)
    bad = shapes[:2].copy()
    bad["kind"][1] = 3
    assert W.refused(bad) and W.refused(np.zeros(W.MAX_TABLES + 1, SW.SHAPE_DTYPE)) and not W.refused(np.zeros(W.MAX_TABLES + 1, SW.SHAPE_DTYPE), tables=False)
