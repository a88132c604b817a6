"""The distance half of dust_amd/csrc/model_records.hpp (device_distance, distance_result) run as native code on a CPU:
tests/cpp/distance_records_test.cpp compiled with g++ under AddressSanitizer and UBSan, held to the witness's limit and to its result
record (tests/distance_witness.py)."""
import os
import subprocess

import numpy as np
import pytest

import distance_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "distance_records_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("distance_records") / "distance_records_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def test_queries_become_kernel_arguments(exe):
    queries = [(t, m, f, p, r) for t in (0, 1, 2) for m in (0, 1) for f in (0, 1) for p in (0, 254) for r in (1, 2, 17, 255)]
    got = run(exe, [f"q {t} {m} {f} {p} {r}" for t, m, f, p, r in queries])
    for (t, m, f, p, r), row in zip(queries, got):
        assert row == [1, t, m, p + 1 if t == W.TO_MATERIAL else 0, r, W.limit_of(m, r), f], (t, m, f, p, r)
    refused = [(3, 0, 0, 0, 5), (0, 2, 0, 0, 5), (0, 0, 2, 0, 5), (0, 0, 3, 0, 5), (0, 0, 1 << 31, 0, 5), (2, 0, 0, -1, 5), (2, 0, 0, 255, 5),
               (0, 0, 0, 0, 0), (0, 0, 0, 0, 256), (0, 0, 0, 0, 0xFFFFFFFF)]
    assert [row[0] for row in run(exe, [f"q {t} {m} {f} {p} {r}" for t, m, f, p, r in refused])] == [0] * len(refused)
    assert run(exe, ["q 0 0 0 255 9", "q 1 1 1 -7 9"]) == [[1, 0, 0, 0, 9, 81, 0], [1, 1, 1, 0, 9, 9, 1]]      # palette is read under TO_MATERIAL only


def test_accumulator_becomes_the_result_record(exe):
    rng = np.random.default_rng(23)
    lines, want = [], []
    for fill, radius in ((0.0, 3), (1.0, 3), (0.002, 2), (0.002, 255), (0.3, 255)):
        grid = (rng.random((256, 16, 16)) < fill).astype(np.uint8)          # (a slice of a tree: the record counts 2^24 voxels, so the rest is added as FAR)
        values = W.field(grid, W.TO_SOLID, W.EUCLIDEAN, radius)
        r = W.result(values)
        rest = (1 << 24) - values.size
        finite = np.argwhere(values != W.FAR)
        best = 0
        if len(finite):      # the device's maximum of value << 32 | (0xFFFFFF - key)
            keys = (finite[:, 0] << 16) | (finite[:, 1] << 8) | finite[:, 2]
            best = int(((values[tuple(finite.T)].astype(np.uint64) << np.uint64(32)) | (0xFFFFFF - keys).astype(np.uint64)).max())
        lines.append(f"r {best} {int(r['targets'])} {int(r['far']) + rest}")
        want.append([int(r["targets"]), int(r["near"]), int(r["far"]) + rest, int(r["largest"]), int(r["largest_key"])])
    assert run(exe, lines) == want
    assert want[0][3:] == [0, W.NO_KEY] and want[1][:2] == [256 * 16 * 16, 0]
    assert run(exe, ["r 0 0 16777216", "r 0 1 16777215"]) == [[0, 0, 1 << 24, 0, W.NO_KEY], [1, 0, (1 << 24) - 1, 0, 0xFFFFFF]]
