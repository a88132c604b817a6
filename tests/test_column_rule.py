"""dust_amd/csrc/column_rule.hpp (column_turn, column_run, column_span, column_cell, column_nibble, the key words) and the columns
records of dust_amd/csrc/model_records.hpp (device_columns, columns_apply_arguments, columns_result) run as native code on a CPU:
tests/cpp/column_rule_test.cpp compiled with g++ under AddressSanitizer and UBSan into a program of its own, fed columns on stdin and
held to the witness (tests/column_witness.py), which sees the same columns as a grid of z columns: the empty and the full column, one
voxel at bit 0 and at bit 255, runs across the word edges 63 | 64, 127 | 128 and 191 | 192, the alternating column with its 128 runs,
layers 0, 1, 127 and 128, random columns at three densities, regions that cut runs at either end, and the validation table."""
import os
import subprocess

import numpy as np
import pytest

import column_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "column_rule_test.cpp")
BYTE = 8                                                                           # the program puts palette index 7 into its cells


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("column_rule") / "column_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def words(column):
    """a 256-entry boolean column in coordinate order -> its four 64-bit words"""
    return [sum(1 << k for k in np.flatnonzero(column[64 * w:64 * w + 64]).tolist()) for w in range(4)]


def check_columns(exe, columns, lo, hi, from_high, layer, where, depth):
    """the rule on every column (rows of a boolean (n, 256) array) against the witness on the same columns stood side by side along y
    (u of the z sides: the map is one row)"""
    grid = (columns.astype(np.uint8) * BYTE)[None, :, :]
    face = W.POS_Z if from_high else W.NEG_Z
    region = ((0, 0, lo), (0, len(columns) - 1, hi))
    got = run(exe, ["c " + " ".join(str(v) for v in words(column) + [lo, hi, int(from_high), layer, where, depth]) for column in columns])
    hit, at, length, gap, runs, _ = W.walk(grid, face, -1, W.clip(grid, region), layer)
    _, cells, _ = W.columns(grid, face, -1, region, layer)
    written = W.turned(W.apply(grid, 100, face, where, depth, -1, region, layer)[0] != grid, W.clip(grid, region), face)
    for j, row in enumerate(got):
        want_at = int(at[0, j]) if hit[0, j] else 256
        assert row[:4] == [want_at, int(length[0, j]), int(gap[0, j]), int(runs[0, j])], (j, lo, hi, from_high, layer, row)
        cell = cells[0, j]
        word = int(cell["at"]) | (int(cell["palette"]) << 8) | (int(cell["length_minus_1"]) << 16) | (int(cell["runs"]) << 24)
        assert row[4] == int(cell["at"]) and row[5] == word, (j, row, cell)
        assert int(cell["palette"]) == (BYTE - 1 if hit[0, j] else 255)
        assert list(range(row[6], row[6] + row[7])) == np.flatnonzero(written[0, j]).tolist(), (j, where, depth, row)
    return int(np.count_nonzero(hit))


def special_columns():
    rows = np.zeros((9, 256), bool)
    rows[1] = True                                                                 # full
    rows[2, 0] = rows[3, 255] = True                                               # one voxel at either end
    rows[4, 60:70] = rows[5, 120:130] = rows[6, 190:200] = True                    # runs across 63 | 64, 127 | 128, 191 | 192
    rows[7, 0::2] = True                                                           # alternating from bit 0: 128 runs
    rows[8, 1::2] = True                                                           # ... from bit 1
    rows[4, 63:65] |= True
    return rows


def test_special_columns_and_layers(exe):
    rows = special_columns()
    hits = {}
    for layer in (0, 1, 127, 128):
        for from_high in (False, True):
            hits[layer, from_high] = check_columns(exe, rows, 0, 255, from_high, layer, W.RUN, 256)
            check_columns(exe, rows, 0, 255, from_high, layer, W.GAP, 256)
            check_columns(exe, rows, 0, 255, from_high, layer, W.GAP, 1)
            check_columns(exe, rows, 0, 255, from_high, layer, W.RUN, 3)
    assert hits[0, False] == hits[0, True] == 8 and hits[1, False] == 2 and hits[127, False] == hits[127, True] == 2 and hits[128, False] == 0
    got = run(exe, ["c " + " ".join(str(v) for v in words(rows[k]) + [0, 255, 0, layer, 0, 1]) for k, layer in ((0, 0), (1, 0), (7, 127), (7, 128), (8, 127), (3, 0))])
    assert got[0][:4] == [256, 0, 0, 0] and got[1][:4] == [0, 256, 0, 1] and got[2][:4] == [254, 1, 1, 128] and got[3][:4] == [256, 0, 0, 128]
    assert got[4][:4] == [255, 1, 1, 128] and got[5][:4] == [255, 1, 255, 1]
    assert got[1][5] == 0 | (7 << 8) | (255 << 16) | (1 << 24) and got[0][5] == 255 << 8 and got[3][5] == (255 << 8) | (128 << 24)


def test_regions_cut_runs_at_either_face(exe):
    rows = special_columns()
    hits = 0
    for lo, hi in ((0, 0), (255, 255), (62, 66), (64, 64), (63, 64), (1, 254), (100, 195), (128, 191), (127, 192), (5, 68), (192, 255)):
        for from_high in (False, True):
            for layer in (0, 1, 2):
                hits += check_columns(exe, rows, lo, hi, from_high, layer, (W.RUN, W.GAP)[layer & 1], (1, 256, 2)[layer])
    assert hits > 100


@pytest.mark.parametrize("density", [0.02, 0.5, 0.98])
def test_random_columns(exe, density):
    rng = np.random.default_rng(int(density * 100))
    rows = rng.random((1200, 256)) < density
    hits = check_columns(exe, rows, 0, 255, False, 0, W.RUN, 2) + check_columns(exe, rows, 0, 255, True, 1, W.GAP, 3)
    hits += check_columns(exe, rows, 37, 201, True, 0, W.GAP, 256) + check_columns(exe, rows, 64, 190, False, 3, W.RUN, 256)
    assert hits > 1200


def test_nibbles_and_key_words(exe):
    rng = np.random.default_rng(5)
    requests, want = [], []
    for _ in range(200):
        word = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        axis = int(rng.integers(0, 3))
        stride = 16 >> (2 * axis)
        other = [int(rng.integers(0, 4)) for _ in range(3)]
        other[axis] = 0
        off = (other[0] << 4) | (other[1] << 2) | other[2]
        requests.append(f"n {word} {off} {stride}")
        want.append([sum(((word >> (off + i * stride)) & 1) << i for i in range(4))])
    assert run(exe, requests) == want and len({w[0] for w in want}) == 16
    # one atomic maximum each: the nearest and the farthest of a set of hit voxels, among equal depths the lowest key
    voxels = [(int(d), int(k)) for d, k in zip(rng.integers(0, 256, 300), rng.integers(0, 1 << 24, 300))]
    voxels += [(0, 0xFFFFFF), (0, 5), (255, 0xFFFFFF), (255, 9), (255, 0), (0, 0)]
    got = run(exe, [f"k {d} {k}" for d, k in voxels])
    for (d, k), row in zip(voxels, got):
        assert row[2] == row[3] == k
    for subset in (slice(0, 300), slice(0, 301), slice(0, 303), slice(0, 306), slice(300, 301), slice(302, 303)):
        part, rows = voxels[subset], got[subset]
        near, far = max(r[0] for r in rows), max(r[1] for r in rows)
        assert (~near) & 0xFFFFFF == min(part)[1] and 0xFFFFFF - (far & 0xFFFFFF) == min(part, key=lambda v: (-v[0], v[1]))[1]


def test_query_validation_table_and_clipping(exe):
    queries = [(face, flags, palette, lo, hi, layer, reserved)
               for face in (0, 1, 2, 3, 4, 8, 16, 32, 48, 64, 128, 0xFFFFFFFF) for flags in (0, 1, 1 << 31) for palette in (-2, -1, 0, 254, 255)
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((17, 3, 250), (40, 3, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 300, 1)), ((3, 2, 1), (30, 20, 4000)))
               for layer, reserved in ((0, 0), (255, 0), (256, 0), (0, 1))]
    got = run(exe, ["q " + " ".join(str(v) for v in (face, flags, palette) + lo + hi + (layer, reserved)) for face, flags, palette, lo, hi, layer, reserved in queries])
    accepted = 0
    for (face, flags, palette, lo, hi, layer, reserved), row in zip(queries, got):
        if W.refused(face, flags, palette, layer, reserved):
            assert row == [0], (face, flags, palette, layer, reserved)
            continue
        accepted += 1
        axis, from_high = W.side(face)
        hi = tuple(min(h, 255) for h in hi)                                        # clipped to the tree
        empty = any(l > h for l, h in zip(lo, hi))
        ua, va = W.U_AXIS[axis], W.V_AXIS[axis]
        nu, nv = (0, 0) if empty else (hi[ua] - lo[ua] + 1, hi[va] - lo[va] + 1)
        assert row[:8] == [1, int(empty), axis, int(from_high), palette + 1, layer, nu, nv]
        if empty:
            assert len(row) == 8
        else:
            assert row[8:] == [lo[axis], hi[axis], lo[ua], hi[ua], lo[va], hi[va], lo[ua] >> 4, lo[va] >> 4, (hi[ua] >> 4) - (lo[ua] >> 4) + 1,
                               (hi[va] >> 4) - (lo[va] >> 4) + 1]
    assert accepted == 6 * 1 * 3 * 5 * 2
    cases = [(where, depth, value) for where in (0, 1, 2, 0xFFFFFFFF) for depth in (0, 1, 256, 257, 0xFFFFFFFF) for value in (-2, -1, 0, 254, 255)]
    got = run(exe, [f"a {where} {depth} {value}" for where, depth, value in cases])
    assert [row[0] for row in got] == [int(not W.refused(W.POS_Y, 0, -1, 0, 0, where, depth, value)) for where, depth, value in cases]
    assert sum(row[0] for row in got) == 2 * 2 * 3


def test_result_record(exe):
    near, far = (~((3 << 24) | 0x010203)) & 0xFFFFFFFF, (200 << 24) | (0xFFFFFF - 0x0A0B0C)
    acc = [10, 200, 30, 777, near, far, 255 - 3, 255 - 0, 255 - 200, 9, 255, 201]
    got = run(exe, ["r", "r 16 20 " + " ".join(str(v) for v in acc), "r 4 5 " + " ".join(["0", "0", "6"] + ["0"] * 9)])
    zero = W.zero_result()
    assert got[0] == [0] * 5 + [W.NO_KEY, W.NO_KEY] + zero["lo"].tolist() + zero["hi"].tolist() + [0]
    assert got[1] == [320, 10, 200, 30, 777, 0x010203, 0x0A0B0C, 3, 0, 200, 9, 255, 201, 0]
    assert got[2] == [20, 0, 0, 6, 0, W.NO_KEY, W.NO_KEY, 255, 255, 255, 0, 0, 0, 0]   # columns and runs, none hit: the keys and bounds of the zero result
