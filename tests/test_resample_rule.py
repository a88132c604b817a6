"""dust_amd/csrc/resample_rule.hpp (the text k_resample of resample.hip runs) and the resample records of
dust_amd/csrc/model_records.hpp (resample_op_refusal, resample_map_refusal, device_resample, the cell binning) run as native code on a CPU:
tests/cpp/resample_rule_test.cpp compiled with g++ under AddressSanitizer and UBSan into a program of its own, fed maps, voxels and
boxes on stdin. The program checks resample_box_range against loops over the box, that a rejected box holds no voxel of the image and
that no cell with one goes unlisted; here its source coordinates, ranges and cell lists are held to the witness
(tests/resample_witness.py). UBSan is the overflow check: the maps include every entry at +-8.0 with |t| = 2^28 at voxels 0 and 255."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import resample_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "resample_rule_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resample_rule") / "resample_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def fixed(v):
    return int(round(float(v) * W.ONE))


def text(m, t):
    return " ".join(str(int(v)) for v in list(np.asarray(m).reshape(-1)) + list(t))


def random_maps(rng, n):
    """rotations with scales and shears, singular ones, and entries and translations up to their limits"""
    out = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            a = rng.normal(size=(3, 3))
            q, _ = np.linalg.qr(a)
            m = np.rint(q * rng.uniform(0.3, 3.0) * W.ONE).astype(np.int64)
            t = rng.integers(-300 * W.ONE, 300 * W.ONE, 3)
        elif kind == 1:
            m = rng.integers(-W.MAX_M, W.MAX_M + 1, (3, 3))
            t = rng.integers(-W.MAX_T, W.MAX_T + 1, 3)
        elif kind == 2:
            m = rng.integers(-W.ONE, W.ONE + 1, (3, 3))
            m[int(rng.integers(0, 3))] = 0                       # singular
            t = rng.integers(0, 256 * W.ONE, 3)
        else:
            m = np.eye(3, dtype=np.int64) * W.ONE + rng.integers(-3, 4, (3, 3))      # the identity, a few units of 1 / 65536 off
            t = rng.integers(-2 * W.ONE, 2 * W.ONE, 3)
        out.append((m.astype(np.int64), [int(v) for v in t]))
    return out


def boxes(rng):
    """single voxels, 4^3 bricks, 16^3 cells and clipped slivers, at the tree's faces too"""
    out = []
    for _ in range(4):
        p = [int(c) for c in rng.integers(0, 256, 3)]
        out.append((p, p))
    for _ in range(4):
        b = [int(c) * 4 for c in rng.integers(0, 64, 3)]
        out.append((b, [c + 3 for c in b]))
    for cell in ((0, 0, 0), (15, 15, 15), (3, 9, 15)):
        out.append(([c * 16 for c in cell], [c * 16 + 15 for c in cell]))
    for _ in range(5):
        cell = [int(c) * 16 for c in rng.integers(0, 16, 3)]
        lo = [c + int(rng.integers(0, 16)) for c in cell]
        hi = [min(l + int(rng.integers(0, 3)) if rng.random() < 0.6 else c + 15, c + 15) for l, c in zip(lo, cell)]
        out.append((lo, hi))
    return out


def test_source_coordinates_at_the_limits_and_at_random(exe):
    cases = []
    for signs in itertools.product((-1, 1), repeat=4):            # every entry at +-8.0 (one sign per row and one for all of t), |t| = 2^28
        m = np.array([[signs[k] * W.MAX_M] * 3 for k in range(3)], np.int64)
        for mixed in (False, True):
            mm = m.copy()
            if mixed:
                mm[:, 1] *= -1
            for voxel in itertools.product((0, 255), repeat=3):
                cases.append((mm, [signs[3] * W.MAX_T] * 3, voxel))
    rng = np.random.default_rng(21)
    for m, t in random_maps(rng, 40):
        for _ in range(4):
            cases.append((m, t, tuple(int(v) for v in rng.integers(0, 256, 3))))
    cases.append((np.eye(3, dtype=np.int64) * W.ONE, [fixed(-0.75), 0, -1], (0, 0, 0)))     # Q = -32768 and Q = -2 + 65536: floors -1 and 0
    got = run(exe, [f"s {text(m, t)} {v[0]} {v[1]} {v[2]}" for m, t, v in cases])
    assert len(got) == len(cases)
    negative = 0
    for (m, t, v), row in zip(cases, got):
        rec = W.records([m], [t], v, v)[0]
        want = [int(s[0, 0, 0]) for s in W.source_of(rec, list(v), list(v))]
        assert row == want, (m, t, v)
        negative += sum(w < 0 for w in want)
    assert got[-1] == [-1, 0, 0] and negative > 100
    extreme = max(abs(q) for m, t, v in cases[:10] for pair in W.box_range(W.records([m], [t], v, v)[0], list(v), list(v)) for q in pair)
    assert extreme < 1 << 31


def test_box_ranges_and_the_interval_test(exe):
    rng = np.random.default_rng(22)
    cases = []
    for m, t in random_maps(rng, 24):
        for lo, hi in boxes(rng):
            a, b = sorted(int(v) for v in rng.integers(0, 256, 2))
            sl, sh = ((0, 0, 0), (255, 255, 255)) if rng.random() < 0.3 else ((a, 0, a), (b, 255, b))
            cases.append((m, t, lo, hi, sl, sh))
    got = run(exe, [f"b {text(m, t)} " + " ".join(str(v) for v in list(lo) + list(hi) + list(sl) + list(sh)) for m, t, lo, hi, sl, sh in cases])
    assert len(got) == len(cases)
    rejected = held = 0
    for (m, t, lo, hi, sl, sh), row in zip(cases, got):
        rec = W.records([m], [t], lo, hi, W.REPLACE, sl, sh)[0]
        assert row[:6] == [q for pair in W.box_range(rec, lo, hi) for q in pair]
        assert row[6] == int(W.box_can_hold(rec, lo, hi)) and row[7] == int(W.image_of(rec, lo, hi)[0].any())
        assert row[6] or not row[7]
        rejected += not row[6]
        held += row[7]
    assert rejected > 50 and held > 50


def test_records_and_cell_lists(exe):
    rng = np.random.default_rng(23)
    cases = []
    for i, (m, t) in enumerate(random_maps(rng, 28)):
        lo = [int(v) for v in rng.integers(-40, 200, 3)]
        hi = [l + int(v) for l, v in zip(lo, rng.integers(0, 90, 3))]
        a, b = sorted(int(v) for v in rng.integers(0, 256, 2))
        cases.append((m, t, lo, hi, (a, 10, 0), (b, 200, 255), i % 5))
    eye = np.eye(3, dtype=np.int64) * W.ONE
    c, s = fixed(np.cos(np.pi / 4)), fixed(np.sin(np.pi / 4))
    cases += [(eye, [0, 0, 0], [-2 ** 31] * 3, [2 ** 31 - 1] * 3, (0, 0, 0), (255, 255, 255), 2),             # the whole tree, every cell
              (np.array([[c, 0, s], [0, W.ONE, 0], [-s, 0, c]]), [fixed(-50), 0, fixed(128)], [0, 0, 0], [255, 255, 255], (0, 0, 0), (199, 199, 2), 2),  # a thin slab, turned
              (eye, [0, 0, 0], [5, 0, 0], [4, 9, 9], (0, 0, 0), (9, 9, 9), 0), (eye, [0, 0, 0], [0, 0, 0], [9, 9, 9], (0, 6, 0), (9, 5, 9), 0),
              (eye, [0, 0, 0], [256, 0, 0], [300, 9, 9], (0, 0, 0), (255, 255, 255), 0), (eye, [0, 0, 0], [0, 0, -90], [9, 9, -1], (0, 0, 0), (255, 255, 255), 0),
              (eye, [0, 0, 0], [0, 0, 0], [9, 9, 9], (0, 0, 0), (9, 9, 9), 5), (eye * 8 + 1, [0, 0, 0], [0, 0, 0], [9, 9, 9], (0, 0, 0), (9, 9, 9), 0),
              (eye, [0, W.MAX_T + 1, 0], [0, 0, 0], [9, 9, 9], (0, 0, 0), (9, 9, 9), 0), (-eye * 8 - 1, [0, 0, 0], [0, 0, 0], [9, 9, 9], (0, 0, 0), (9, 9, 9), 0),
              (eye, [0, 0, -W.MAX_T - 1], [0, 0, 0], [9, 9, 9], (0, 0, 0), (9, 9, 9), 0),
              (np.zeros((3, 3), np.int64), [fixed(3.5)] * 3, [10, 10, 10], [40, 12, 12], (0, 0, 0), (9, 9, 9), 1),                          # singular: one voxel
              (np.zeros((3, 3), np.int64), [fixed(30.5)] * 3, [10, 10, 10], [40, 12, 12], (0, 0, 0), (9, 9, 9), 1)]                         # ... outside the sub-box
    # live, and listed in no cell: s[0] = 8 x + 4 reads 4..124 in cell 0 and 132..252 in cell 1; 127 lies in the whole box's 4..252 only
    cases.append((eye * np.array([8, 1, 1])[:, None], [0, 0, 0], [0, 0, 0], [31, 15, 15], (127, 0, 0), (127, 15, 15), 2))
    got = run(exe, [f"r {text(m, t)} " + " ".join(str(v) for v in list(lo) + list(hi) + list(sl) + list(sh)) + f" {op}" for m, t, lo, hi, sl, sh, op in cases])
    assert len(got) == len(cases)
    tables = {W.PLACE: 0b00_01_00_00, W.OVERWRITE: 0b01_01_00_00, W.REPLACE: 0b01_01_01_01, W.CARVE: 0b10_00_00_00, W.PAINT: 0b01_00_00_00}
    refused = dead = culled = 0
    for (m, t, lo, hi, sl, sh, op), row in zip(cases, got):
        rec = W.records([m], [t], lo, hi, op, sl, sh)[0]
        if W.refused(rec):
            assert row == [1]
            refused += 1
            continue
        cells, reached = W.cells_listed(rec)
        box = W.clipped_box(rec)
        if box is None or not W.box_can_hold(rec, *box):
            assert row == [0, 0] and not cells, (lo, hi, sl, sh)
            dead += 1
            continue
        pack = lambda v: int(v[0]) | int(v[1]) << 8 | int(v[2]) << 16  # noqa: E731
        assert row[:7] == [0, 1, pack(box[0]), pack(box[1]), pack(sl), pack(sh), tables[op]]
        assert row[7] == len(cells) and row[8:] == cells
        culled += reached - len(cells)
    assert refused == 5 and dead >= 5 and culled > 1000
    assert got[28][7] == 4096 and len(got[29]) - 8 < 2048                        # the whole tree; the turned slab: more than half culled
    assert got[-1][:2] == [0, 1] and got[-1][7:] == [0]                          # a live record without a cell
