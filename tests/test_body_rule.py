"""The device-free half of dust_hip_model_bodies run as native code on a CPU: tests/cpp/body_rule_test.cpp compiled with g++ under
AddressSanitizer and UBSan into a program of its own (no HIP compiler, not linked against the library). It drives body_shift, the
popcount fast path, the per-voxel weighted path, the fold and the emit of dust_amd/csrc/body_rule.hpp -- the one text k_bodies runs --
and device_bodies of dust_amd/csrc/model_records.hpp, and is held to tests/body_witness.py."""
import os
import subprocess

import numpy as np
import pytest

import body_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "body_rule_test.cpp")

BRICK = np.dtype([("mask", "<u8"), ("at", "<u4", 3), ("key", "<u4"), ("w", "<u2", 64)])
BRICK_OUT = np.dtype([("fast", "<u4", 10), ("slow", "<u4", 10), ("unit", "<u4", 10), ("record", W.BODY_DTYPE)])
QUERY_OUT = np.dtype([("refused", "<u4"), ("empty", "<u4"), ("group", "<u4"), ("byte", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3), ("box_lo", "<u4", 3),
                      ("box_hi", "<u4", 3)])
assert (BRICK.itemsize, BRICK_OUT.itemsize, QUERY_OUT.itemsize) == (152, 216, 64)
BITS = np.arange(64)
LOCAL = np.stack([BITS >> 4, (BITS >> 2) & 3, BITS & 3], axis=1)            # voxel bit -> (lx, ly, lz)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("body_rule") / "body_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, tmp_path, bricks=(), folds=0, queries=()):
    """one run of the program (which must end clean under both sanitizers) -> (per brick, all folded, brick 0 folded `folds` times, per query)"""
    bricks = np.zeros(0, BRICK) if len(bricks) == 0 else np.asarray(bricks, BRICK).reshape(-1)
    queries = np.zeros(0, W.QUERY_DTYPE) if len(queries) == 0 else np.asarray(queries, W.QUERY_DTYPE).reshape(-1)
    head = np.array([len(bricks), folds, len(queries), 0], "<u4")
    (tmp_path / "in.bin").write_bytes(head.tobytes() + bricks.tobytes() + queries.tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    data = (tmp_path / "out.bin").read_bytes()
    per = np.frombuffer(data, BRICK_OUT, len(bricks))
    rest = np.frombuffer(data, W.BODY_DTYPE, 2, per.nbytes)
    answers = np.frombuffer(data, QUERY_OUT, len(queries), per.nbytes + rest.nbytes)
    assert per.nbytes + rest.nbytes + answers.nbytes == len(data)
    return per, rest[0], rest[1], answers


def _bits(mask):
    return np.array([(int(mask) >> b) & 1 for b in range(64)], bool)


def _voxels(brick):
    """the witness's view of a brick case: absolute coordinates and weights of the mask's voxels"""
    on = _bits(brick["mask"])
    return LOCAL[on] + 4 * brick["at"].astype(np.int64), brick["w"][on]


def _locals(on, w):
    x, y, z = (LOCAL[on, r].astype(np.int64) for r in range(3))
    w = w[on].astype(np.int64)
    return [int(v.sum()) for v in (w, w * x, w * y, w * z, w * x * x, w * y * y, w * z * z, w * x * y, w * y * z, w * z * x)]


def test_random_bricks_against_the_witness(exe, tmp_path):
    rng = np.random.default_rng(71)
    n = 300
    bricks = np.zeros(n, BRICK)
    # distinct bricks of one grid, so that the fold of all of them is one witness call over it
    codes = rng.choice(64 ** 3, n, replace=False)
    bricks["at"] = np.stack([codes >> 12, (codes >> 6) & 63, codes & 63], axis=1)
    bricks["at"][0] = (63, 63, 63)
    assert len(np.unique(bricks["at"], axis=0)) == n
    density = rng.random(n)
    on = rng.random((n, 64)) < density[:, None]
    on[1], on[2], on[3] = True, False, False
    on[3, 37] = True                                                         # full, empty, one voxel
    bricks["mask"] = (on.astype(np.uint64) << BITS.astype(np.uint64)).sum(axis=1, dtype=np.uint64)
    weights = rng.integers(0, 65536, W.WEIGHTS)
    weights[:3] = 0, 65535, 1
    byte = rng.integers(1, 256, (n, 64))
    byte[:40] = rng.integers(1, 4, (40, 64))                                 # weights 0 and 65535 among them
    bricks["w"] = weights[byte - 1]
    bricks["key"] = rng.integers(0, 1 << 24, n)
    per, folded, _, _ = run(exe, tmp_path, bricks)
    grid = np.zeros((256, 256, 256), np.uint8)
    for b, o, g, got in zip(bricks, on, byte, per):
        assert got["fast"].tolist() == _locals(o, np.ones(64, np.int64)) == got["unit"].tolist()
        assert got["slow"].tolist() == _locals(o, b["w"])
        xyz, w = _voxels(b)
        assert got["record"].tobytes() == W.record_of(b["key"], xyz, w).tobytes()
        grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]] = g[o]
    want = W.bodies(grid, W.ALL, weights)[0].copy()
    want["key"] = 7
    assert folded.tobytes() == want.tobytes()


def test_every_single_voxel_and_every_plane(exe, tmp_path):
    """the fast path's planes and columns one at a time: 64 single voxels, then the 12 planes c = 0..3 of the three axes"""
    planes = [sum(1 << int(b) for b in BITS[LOCAL[:, r] == c]) for r in range(3) for c in range(4)]
    masks = [1 << b for b in range(64)] + planes
    bricks = np.zeros(len(masks), BRICK)
    bricks["mask"], bricks["at"], bricks["w"] = masks, (17, 0, 63), 1
    per, _, _, _ = run(exe, tmp_path, bricks)
    for b, got in zip(bricks, per):
        on = _bits(b["mask"])
        assert got["fast"].tolist() == got["unit"].tolist() == got["slow"].tolist() == _locals(on, np.ones(64, np.int64))
        assert got["record"].tobytes() == W.record_of(0, *_voxels(b)).tobytes()


def test_maximal_brick_folded_two_to_the_eighteen_times(exe, tmp_path):
    """the brick at 252..255 on every axis with all weights 65535: its local moments are the largest a brick can have, and 2^18 of
    them folded -- as many voxels as the tree holds, each with the largest coordinates -- stay exact in 64 bits"""
    brick = np.zeros(1, BRICK)
    brick["mask"], brick["at"], brick["w"], brick["key"] = (1 << 64) - 1, (63, 63, 63), 65535, 0xFFFFFF
    folds = 1 << 18
    per, _, many, _ = run(exe, tmp_path, brick, folds=folds)
    assert per[0]["slow"].tolist() == [65535 * v for v in per[0]["fast"].tolist()] and max(per[0]["slow"].tolist()) == 224 * 65535 < 64 * 65535 * 9 < 1 << 32
    one = W.record_of(0xFFFFFF, *_voxels(brick[0]))
    assert per[0]["record"].tobytes() == one.tobytes()
    assert int(many["key"]) == 9 and int(many["voxels"]) == 1 << 24 and many["lo"].tolist() == [252] * 3 and many["hi"].tolist() == [255] * 3
    assert int(many["mass"]) == 65535 << 24
    assert [int(v) for v in many["m1"]] == [folds * int(v) for v in one["m1"]]
    assert [int(v) for v in many["m2"]] == [folds * int(v) for v in one["m2"]]
    assert max(int(v) for v in many["m2"]) < 65535 * 255 ** 2 << 24 < 1 << 63


def test_queries_are_refused_as_the_witness_says(exe, tmp_path):
    def query(group=W.ALL, flags=0, palette=-1, lo=(0, 0, 0), hi=(255, 255, 255), reserved=(0, 0)):
        return (48, group, flags, palette, lo, hi, reserved)
    cases = [query(), query(group=3), query(group=4), query(group=0xFFFFFFFF), query(flags=1), query(reserved=(1, 0)), query(reserved=(0, 5)),
             query(palette=-2), query(palette=254), query(palette=255), query(lo=(256, 0, 0)), query(hi=(255, 255, 256)), query(lo=(9, 9, 9), hi=(9, 9, 9)),
             query(lo=(17, 40, 3), hi=(200, 41, 255), palette=7, group=W.MATERIALS), query(lo=(5, 0, 0), hi=(4, 255, 255)), query(lo=(0, 0, 255), hi=(0, 0, 0))]
    queries = np.array(cases, W.QUERY_DTYPE)
    _, _, _, answers = run(exe, tmp_path, queries=queries)
    for q, a in zip(queries, answers):
        region = (q["lo"].tolist(), q["hi"].tolist())
        assert bool(a["refused"]) == W.refused(int(q["group"]), int(q["flags"]), int(q["palette"]), region, q["reserved"].tolist()), q
        if a["refused"]:
            continue
        assert a["group"] == q["group"] and a["byte"] == q["palette"] + 1
        assert bool(a["empty"]) == any(l > h for l, h in zip(*region))
        if not a["empty"]:
            assert a["lo"].tolist() == region[0] and a["hi"].tolist() == region[1]
            assert a["box_lo"].tolist() == [v >> 4 for v in region[0]] and a["box_hi"].tolist() == [v >> 4 for v in region[1]]
    assert answers["refused"].sum() == 9
