"""dust_amd/csrc/settle_rule.hpp (settle_fall, settle_destination, settle_walk, settle_slide) and the settle records of
dust_amd/csrc/model_records.hpp (device_settle, settle_apply_arguments, settle_slide_direction, settle_result, settle_applied,
settle_at_rest) run as native code on a CPU: tests/cpp/settle_rule_test.cpp compiled with g++ under AddressSanitizer and UBSan into a
program of its own. The fall and the slide are checked inside the program against bit loops -- the empty, the full and the alternating
column, a fixed voxel at every word edge, random columns; random 12^3 worlds for every pair of directions --; the records are fed on
stdin and held to the witness (tests/settle_witness.py)."""
import os
import subprocess

import numpy as np
import pytest

import settle_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "settle_rule_test.cpp")
ACC_WORDS = 14


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("settle_rule") / "settle_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, mode, lines=(), seed=None):
    done = subprocess.run([exe, mode] + ([str(seed)] if seed is not None else []), input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


@pytest.mark.parametrize("seed", [1, 2])
def test_fall_against_the_bit_loop(exe, seed):
    (columns, moved), = run(exe, "fall", seed=seed)
    assert columns == 16 + 4 * 16 + 4000 and moved > 50000


@pytest.mark.parametrize("seed", [3, 4])
def test_slide_against_the_voxel_loop(exe, seed):
    (bricks, slid), = run(exe, "slide", seed=seed)
    assert bricks == 24 * 6 * 4 * 27 and slid > 5000


def test_query_validation_table(exe):
    masks = (W.ALL_LOOSE, W.loose_mask([]), W.loose_mask([3, 200]), (0,) * 7 + (1 << 31,), (0xFFFFFFFF,) * 8, W.loose_mask([(0, 253)]))
    queries = [(toward, flags, reserved, lo, hi, loose)
               for toward in (0, 1, 2, 3, 4, 8, 16, 32, 48, 64, 0xFFFFFFFF) for flags, reserved in ((0, 0), (1, 0), (0, 1), (1 << 31, 0))
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((17, 3, 250), (40, 3, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 300, 1)), ((3, 2, 1), (30, 20, 256)))
               for loose in masks]
    got = run(exe, "records", ["q " + " ".join(str(v) for v in (toward, flags, reserved) + lo + hi + loose) for toward, flags, reserved, lo, hi, loose in queries])
    accepted = 0
    for (toward, flags, reserved, lo, hi, loose), row in zip(queries, got):
        if W.refused(toward, flags, reserved, lo, hi, loose):
            assert row == [0], (toward, flags, reserved, lo, hi, loose)
            continue
        accepted += 1
        axis, from_high = W.side(toward)
        empty = any(l > h for l, h in zip(lo, hi))
        ua, va = W.U_AXIS[axis], W.V_AXIS[axis]
        nu, nv = (0, 0) if empty else (hi[ua] - lo[ua] + 1, hi[va] - lo[va] + 1)
        assert row[:7] == [1, int(empty), int(loose == W.ALL_LOOSE), axis, int(from_high), nu, nv]
        if empty:
            assert len(row) == 7
        else:
            assert row[7:] == [lo[axis], hi[axis], lo[ua], hi[ua], lo[va], hi[va], lo[ua] >> 4, lo[va] >> 4, (hi[ua] >> 4) - (lo[ua] >> 4) + 1,
                               (hi[va] >> 4) - (lo[va] >> 4) + 1] + [c >> 4 for c in lo] + [c >> 4 for c in hi]
    assert accepted == 6 * 1 * 3 * 4
    cases = (0, 1, 255, 256, 257, 0xFFFFFFFF)
    assert [row[0] for row in run(exe, "records", [f"g {g}" for g in cases])] == [int(not W.refused(4, 0, 0, (0,) * 3, (0,) * 3, W.ALL_LOOSE, g)) for g in cases]
    for axis in range(3):                                                            # +u, -u, +v, -v, and round again
        for k, row in enumerate(run(exe, "records", [f"d {axis} {k}" for k in range(9)])):
            d = W.lateral(W.FACES[2 * axis], k)
            assert row == [int(np.flatnonzero(d)[0]), int(sum(d) > 0)]


def test_result_record(exe):
    acc = [1000, 2000, 300, 400, 5000, 60, 0, 77, 255 - 3, 255 - 0, 255 - 200, 9, 255, 201]
    none = [5, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    got = run(exe, "records", ["r", "r 16 20 " + " ".join(str(v) for v in acc), "r 4 5 " + " ".join(str(v) for v in none)])
    assert got[0] == [0] * 7 + [255] * 3 + [0] * 3 + [0, 0]
    assert got[1] == [320, 1000, 2000, 300, 400, 77, 5000, 3, 0, 200, 9, 255, 201, 60, 0]
    assert got[2] == [20, 5, 6, 0, 0, 0, 0, 255, 255, 255, 0, 0, 0, 0, 0]           # nothing would move: the bounds of the zero result


def slot(loose=0, moved=0, fall_sum=0, slid=0, lo=None, hi=None):
    words = [loose, 0, moved, 0, fall_sum, 0, slid, 0] + ([0] * 6 if lo is None else [255 - c for c in lo] + list(hi))
    assert len(words) == ACC_WORDS
    return words


def test_applied_record(exe):
    # the initial fall, then: a generation that slides and falls, one that only slides, two that do nothing, one that falls, then rest
    steps = [slot(loose=500, moved=40, fall_sum=90, lo=(10, 0, 10), hi=(12, 30, 12)),
             slot(slid=7, lo=(9, 20, 10), hi=(13, 21, 12)), slot(moved=5, fall_sum=11, lo=(9, 4, 10), hi=(9, 20, 10)),
             slot(slid=2, lo=(14, 1, 1), hi=(15, 2, 1)), slot(),
             slot(), slot(), slot(), slot(),
             slot(), slot(moved=1, fall_sum=200, lo=(0, 0, 0), hi=(0, 255, 0))]
    words = [w for s in steps for w in s]
    got = run(exe, "records", [f"a 8 {len(words)} " + " ".join(str(w) for w in words), "a 3", f"a 2 {len(words)} " + " ".join(str(w) for w in words), "a 0 14 " + " ".join(
        str(w) for w in steps[0]), f"a 256 {len(words)} " + " ".join(str(w) for w in words)])
    assert got[0][:14] == [5, 40, 500, 9, 6, 301, 0, 0, 0, 15, 255, 12, 0, 0]         # two quiet generations are not rest: AT_REST 0
    assert got[0][14:] == [7, 5, 2, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert got[1] == [0, 0, 0, 0, 0, 0, 255, 255, 255, 0, 0, 0, 0, 0] + [0] * 6       # nothing was looked at: the zero record, the rows cleared
    assert got[2] == [2, 40, 500, 9, 5, 101, 9, 0, 1, 15, 30, 12, 0, 0, 7, 5, 2, 0]
    assert got[3] == [0, 40, 500, 0, 0, 90, 10, 0, 10, 12, 30, 12, 0, 0]
    assert got[4][:14] == [5, 40, 500, 9, 6, 301, 0, 0, 0, 15, 255, 12, 0, 1] and not any(got[4][14 + 10:])  # 251 quiet generations behind it: at rest
    quiet = [w for s in [steps[0]] + [slot()] * 8 for w in s]
    rest = run(exe, "records", [f"a 3 {len(quiet)} " + " ".join(str(w) for w in quiet), f"a 4 {len(quiet)} " + " ".join(str(w) for w in quiet)])
    assert rest[0][13] == 0 and rest[1][13] == 1 and rest[1][0] == 0                  # four in a row, one per direction
