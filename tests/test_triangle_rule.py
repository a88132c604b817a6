"""dust_amd/csrc/triangle_rule.hpp (the text k_edit_triangles and k_fill_columns of triangle.hip run) and the triangle records of
dust_amd/csrc/model_records.hpp (device_triangle, device_fill_triangle, device_fill_mesh, fill_mesh_result) run as native code on a
CPU: tests/cpp/triangle_rule_test.cpp compiled with g++ under AddressSanitizer and UBSan into a program of its own, fed triangles on
stdin and held to the witness (tests/triangle_witness.py) voxel by voxel and column by column. UBSan is the overflow check: the cases
include vertices at +-2^18 and triangles that span the full range."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import triangle_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "triangle_rule_test.cpp")
M = W.MAX_COORD


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("triangle_rule") / "triangle_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def flat(v):
    return " ".join(str(c) for p in v for c in p)


def box_around(v, pad=1):
    """the voxels the vertices' extent touches and `pad` more on every side, unclipped (negative and beyond 255 included)"""
    lo = [(min(p[r] for p in v) - 1) // W.UNIT - pad for r in range(3)]
    hi = [max(p[r] for p in v) // W.UNIT + pad for r in range(3)]
    return lo, hi


def check_surface(exe, cases):
    """cases: [(v, lo, hi)] -- every voxel of lo..hi, against the witness's per-voxel Python-int test"""
    got = run(exe, [f"s {flat(v)} {lo[0]} {lo[1]} {lo[2]} {hi[0]} {hi[1]} {hi[2]}" for v, lo, hi in cases])
    total = 0
    for (v, lo, hi), row in zip(cases, got):
        b_lo, m = W.coverage(v, lo=lo, hi=hi)
        want = np.zeros(tuple(h - l + 1 for l, h in zip(lo, hi)), bool)
        if m is not None:
            for x, y, z in np.argwhere(m):
                at = (x + b_lo[0] - lo[0], y + b_lo[1] - lo[1], z + b_lo[2] - lo[2])
                if all(0 <= a < s for a, s in zip(at, want.shape)):
                    want[at] = True
        assert row[0] == want.size and row[1:] == want.reshape(-1).astype(int).tolist(), (v, lo, hi)
        total += int(want.sum())
    return total


def random_lattice_triangles(rng, n, lo, hi, step):
    """vertices on a lattice of `step` units inside lo..hi voxels: full of triangles that only touch cubes"""
    out = []
    while len(out) < n:
        v = [tuple(int(c) for c in p) for p in rng.integers(lo * W.UNIT // step, hi * W.UNIT // step + 1, (3, 3)) * step]
        if W.normal(v) != (0, 0, 0):
            out.append(v)
    return out


def test_surface_random_lattice_triangles(exe):
    rng = np.random.default_rng(1)
    cases = []
    for step, lo, hi in ((256, 3, 9), (128, 2, 7), (64, -3, 2), (1, 250, 258), (32, -1024, -1016)):
        for v in random_lattice_triangles(rng, 40, lo, hi, step):
            cases.append((v, *box_around(v)))
    assert check_surface(exe, cases) > 2000
    # the witness's vectorised coverage is its per-voxel test
    for v, lo, hi in cases[::9]:
        b_lo, m = W.coverage(v, lo=lo, hi=hi)
        for x, y, z in itertools.product(*(range(l, h + 1) for l, h in zip(lo, hi))):
            at = (x - b_lo[0], y - b_lo[1], z - b_lo[2])
            inside = all(0 <= a < s for a, s in zip(at, m.shape)) and bool(m[at])
            assert W.covers(v, x, y, z) == inside


def test_surface_faces_edges_corners_needles_and_the_range_limit(exe):
    U = W.UNIT
    cases = []
    on_face = [(5 * U, 5 * U, 7 * U), (8 * U, 5 * U, 7 * U), (5 * U, 8 * U, 7 * U)]      # lies exactly on the plane z = 7: both sides
    cases.append((on_face, (4, 4, 5), (9, 9, 9)))
    corner = [(4 * U, 4 * U, 4 * U), (4 * U - 300, 4 * U - 10, 4 * U - 200), (4 * U - 20, 4 * U - 310, 4 * U - 100)]   # touches voxel (4, 4, 4) at its corner only
    cases.append((corner, (1, 1, 1), (6, 6, 6)))
    edge = [(4 * U, 4 * U, 4 * U + 100), (4 * U, 4 * U, 4 * U + 200), (4 * U - 500, 4 * U - 300, 4 * U + 150)]         # an edge of it along a cube edge
    cases.append((edge, (1, 1, 3), (6, 6, 6)))
    sliver = [(10 * U + 1, 3 * U + 7, 2 * U + 5), (40 * U + 1, 9 * U + 7, 5 * U + 5), (40 * U + 2, 9 * U + 7, 5 * U + 5)]   # one unit wide
    cases.append((sliver, *box_around(sliver)))
    needle = [(-3 * U, 17, 33), (20 * U, 17, 34), (20 * U, 18, 33)]
    cases.append((needle, *box_around(needle)))
    far = [(M, M, M), (M - 700, M, M - 3), (M, M - 650, M - 1)]                            # at the range limit
    cases.append((far, *box_around(far)))
    near = [(-M, -M, -M), (-M + 700, -M, -M + 3), (-M, -M + 650, -M + 1)]
    cases.append((near, *box_around(near)))
    whole = [(-M, -M, M), (M, -M, -M), (-M, M, -M)]                                       # spans the full range: the largest intermediates
    cases.append((whole, (-2, -2, -2), (3, 3, 3)))
    cases.append((whole, (250, 250, 250), (257, 257, 257)))
    cases.append((whole, (1020, -1026, -1026), (1025, -1020, -1020)))
    cases.append(([(-M, -M, -M), (M, M, M), (M, -M, M)], (-1026, -1026, -1026), (-1020, -1020, -1020)))
    cases.append(([(-M, -M, -M), (M, M, M), (M, -M, M)], (100, 98, 100), (104, 103, 104)))
    vertical = [(3 * U, 2 * U + 128, 0), (3 * U, 6 * U + 128, 0), (3 * U, 2 * U + 128, 4 * U)]   # n.z == 0, on the plane x = 3
    cases.append((vertical, (1, 1, -1), (5, 8, 5)))
    total = check_surface(exe, cases)
    assert total > 300
    assert W.covers(on_face, 5, 5, 6) and W.covers(on_face, 5, 5, 7) and not W.covers(on_face, 5, 5, 8) and not W.covers(on_face, 5, 5, 5)
    assert W.covers(corner, 4, 4, 4) and W.covers(corner, 3, 3, 3) and not W.covers(corner, 5, 4, 4)
    assert W.covers(edge, 4, 4, 4) and W.covers(edge, 3, 4, 4) and W.covers(edge, 4, 3, 4)
    assert W.covers(vertical, 2, 3, 1) and W.covers(vertical, 3, 3, 1) and not W.covers(vertical, 4, 3, 1)


def test_columns_on_edges_and_vertices_and_crossings_outside_the_tree(exe):
    rng = np.random.default_rng(2)
    U = W.UNIT
    cases = []
    for v in random_lattice_triangles(rng, 60, 0, 6, 128):                    # vertices and edges pass through column centres
        for px, py in itertools.product(range(-128, 7 * U, 128), repeat=2):
            cases.append((v, px, py))
    steep = [(2 * U, 2 * U, -900 * U), (6 * U, 2 * U + 1, 900 * U), (2 * U + 3, 7 * U, 100 * U)]      # crossings far below 0 and above 256
    flat_low, flat_high = [(0, 0, -5), (9 * U, 0, -5), (0, 9 * U, -5)], [(0, 0, M), (9 * U, 0, M), (0, 9 * U, M - 1)]
    on_centres = [(0, 0, 3 * U + 128), (9 * U, 0, 3 * U + 128), (0, 9 * U, 3 * U + 128)]             # the plane passes through centres: not crossed there
    wide = [(-M, -M, M), (M, -M, -M), (-M, M, -M)]
    vertical = [(3 * U, 2 * U, 0), (3 * U, 6 * U, 0), (3 * U, 2 * U, 4 * U)]
    for v in (steep, flat_low, flat_high, on_centres, wide, vertical, [p[::-1] for p in wide][::-1]):
        for px, py in itertools.product(range(128, 8 * U, U), repeat=2):
            cases.append((v, px, py))
    cases += [(wide, 255 * U + 128, 255 * U + 128), (wide, -M, -M), (wide, M, M), ([(-M, -M, -M), (M, -M, -M + 1), (-M, M, M)], 128, 128)]
    got = run(exe, [f"c {flat(v)} {px} {py}" for v, px, py in cases])
    crossed = counts = 0
    for (v, px, py), (c, count) in zip(cases, got):
        assert c == int(W.column_crossed(v, px, py)), (v, px, py)
        assert count == (W.crossing_count(v, px, py) if W.normal(v)[2] != 0 else 0), (v, px, py)
        crossed += c
        counts += 0 < count < 256
    assert crossed > 500 and counts > 500
    assert run(exe, [f"c {flat(flat_low)} 640 640", f"c {flat(flat_high)} 640 640", f"c {flat(on_centres)} 640 640"]) == [[1, 0], [1, 256], [1, 3]]
    # a closed fan around a column centre: whatever the windings, exactly one triangle on each side of it is counted
    hub = (2 * U + 128, 2 * U + 128, U)
    rim = [(0, 0, U), (5 * U, 0, U), (5 * U, 5 * U, U), (0, 5 * U, U)]
    fan = [[hub, rim[k], rim[(k + 1) % 4]] if k % 2 else [rim[(k + 1) % 4], rim[k], hub] for k in range(4)]
    assert sum(row[0] for row in run(exe, [f"c {flat(v)} {hub[0]} {hub[1]}" for v in fan])) == 1


def test_bounds_and_operation_bytes(exe):
    rng = np.random.default_rng(3)
    U = W.UNIT
    cases = random_lattice_triangles(rng, 80, -3, 3, 64) + random_lattice_triangles(rng, 80, 250, 260, 64) + random_lattice_triangles(rng, 40, 0, 255, 1)
    cases += [[(4 * U, 4 * U, 4 * U), (5 * U, 4 * U, 4 * U), (4 * U, 5 * U, 4 * U)],     # on 256 k: voxels 3..5 in x and y, 3 and 4 in z
              [(0, 0, 0), (U, 0, 0), (0, U, 0)], [(256 * U, 0, 0), (256 * U, U, 0), (256 * U, 0, U)],   # touching the tree from outside
              [(256 * U + 1, 0, 0), (256 * U + 1, U, 0), (256 * U + 1, 0, U)], [(-1, 0, 0), (-1, U, 0), (-1, 0, U)],   # wholly outside
              [(M, M, M), (M, 0, 0), (0, M, 0)], [(M + 1, 0, 0), (0, 5, 0), (0, 0, 5)], [(0, -M - 1, 0), (5, 0, 0), (0, 0, 5)],
              [(7, 7, 7), (7, 7, 7), (9, 9, 9)], [(0, 0, 0), (U, U, U), (3 * U, 3 * U, 3 * U)]]                         # zero normal
    ops = [(W.CARVE, 77), (W.FILL, 0), (W.PAINT, 254), (W.PLACE, 9)]
    got = run(exe, [f"t {flat(v)} {ops[i % 4][0]} {ops[i % 4][1]}" for i, v in enumerate(cases)])
    kept = 0
    for i, (v, row) in enumerate(zip(cases, got)):
        bounds = W.voxel_bounds(v) if W.live(v) else None
        if bounds is None:
            assert row == [0], v
            continue
        kept += 1
        op, palette = ops[i % 4]
        bytes_ = {W.CARVE: (0, 0), W.FILL: (palette + 1, palette + 1), W.PAINT: (palette + 1, 0), W.PLACE: (256, palette + 1)}[op]
        assert row == [1] + bounds[0] + bounds[1] + list(bytes_), v
    assert 100 < kept <= len(cases) - 7
    assert got[200] == [1, 3, 3, 3, 5, 5, 4, 0, 0] and got[201][:7] == [1, 0, 0, 0, 1, 1, 0] and got[202][:7] == [1, 255, 0, 0, 255, 1, 1]
    assert got[203] == got[204] == got[206] == got[207] == got[208] == got[209] == [0] and got[205][0] == 1
    # the solid rule's columns: centres inside the extent, clipped to the region; live and crossing
    fills = [(v, (lo, lo + 1), (hi, hi - 2)) for v in cases for lo, hi in ((0, 255), (2, 100))]
    got = run(exe, [f"f {flat(v)} {lo[0]} {lo[1]} {hi[0]} {hi[1]}" for v, lo, hi in fills])
    kept = 0
    for (v, lo, hi), row in zip(fills, got):
        alive = W.live(v)
        crossing = alive and W.normal(v)[2] != 0
        want = None
        if crossing:
            c_lo = [max(-((-(min(p[r] for p in v) - 128)) // U), lo[r]) for r in range(2)]
            c_hi = [min((max(p[r] for p in v) - 128) // U, hi[r]) for r in range(2)]
            if all(l <= h for l, h in zip(c_lo, c_hi)):
                want = c_lo + c_hi
        assert row == [int(want is not None), int(alive), int(crossing)] + (want or []), (v, lo, hi)
        kept += want is not None
    assert kept > 50


def test_refusal_table_and_result_record(exe):
    queries = [(op, palette, flags, r0, r1, lo, hi)
               for op in (0, 1, 2, 3, 4, 0xFFFFFFFF) for palette in (-1, 0, 254, 255) for flags, r0, r1 in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 7))
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((17, 3, 250), (40, 3, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 300, 1)), ((0, 0, 0), (1, 1, 4000)))]
    got = run(exe, ["q " + " ".join(str(v) for v in (op, palette, flags, r0, r1) + lo + hi) for op, palette, flags, r0, r1, lo, hi in queries])
    accepted = 0
    for (op, palette, flags, r0, r1, lo, hi), row in zip(queries, got):
        if W.query_refused(op, palette, flags, (r0, r1)):
            assert row == [0]
            continue
        accepted += 1
        hi = tuple(min(h, 255) for h in hi)
        empty = any(l > h for l, h in zip(lo, hi))
        bytes_ = {W.CARVE: (0, 0), W.FILL: (palette + 1, palette + 1), W.PAINT: (palette + 1, 0), W.PLACE: (256, palette + 1)}[op]
        assert row[:4] == [1, int(empty)] + list(bytes_)
        assert row[4:] == ([] if empty else list(lo) + list(hi) + [l >> 4 for l in lo] + [h >> 4 for h in hi])
    assert 0 < accepted < len(queries)
    got = run(exe, ["r", "r 10 4 250 240 230 9 19 29 7 5", "r 0 0 0 0 0 0 0 0 3 2"])
    zero = W.zero_result()
    assert got[0] == [0, 0, 0, 0, 255, 255, 255, 0, 0, 0, 0, 0] == [int(c) for f in W.RESULT_DTYPE.names for c in np.atleast_1d(zero[f])]
    assert got[1] == [10, 4, 7, 5, 5, 15, 25, 9, 19, 29, 0, 0] and got[2] == [0, 0, 3, 2, 255, 255, 255, 0, 0, 0, 0, 0]
