"""The device-free half of dust_hip_model_joints run as native code on a CPU: tests/cpp/joint_rule_test.cpp compiled with g++ under
AddressSanitizer and UBSan into a program of its own (no HIP compiler, not linked against the library). It drives joint_part, the pair
key, the fold, the emit and the table's hash and probe sequence of dust_amd/csrc/joint_rule.hpp -- the one text k_joints runs -- and
device_joints of dust_amd/csrc/model_records.hpp, and is held to a bit loop written here and to tests/joints_witness.py."""
import os
import subprocess

import numpy as np
import pytest

import joints_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "joint_rule_test.cpp")

PART = np.dtype([("word", "<u8"), ("axis", "<u4"), ("flip", "<u4"), ("at", "<u4", 3), ("key", "<u4")])
PAIR_OUT = np.dtype([("key", "<u4"), ("flip", "<u4"), ("a", "<u4"), ("b", "<u4")])
QUERY_OUT = np.dtype([("refused", "<u4"), ("empty", "<u4"), ("group", "<u4"), ("pad", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3), ("box_lo", "<u4", 3),
                      ("box_hi", "<u4", 3)])
TABLE_OUT = np.dtype([("keys", "<u4"), ("inserted", "<u4"), ("found", "<u4"), ("full", "<u4"), ("longest", "<u4")])
assert (PART.itemsize, QUERY_OUT.itemsize) == (32, 64)
BITS = np.arange(64)
LOCAL = np.stack([BITS >> 4, (BITS >> 2) & 3, BITS & 3], axis=1)            # voxel bit -> (lx, ly, lz)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("joint_rule") / "joint_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, tmp_path, parts=(), folds=0, pairs=(), queries=()):
    """one run of the program (which must end clean under both sanitizers) -> (per part, all folded, part 0 folded `folds` times, per
    pair, per query, first slots_log2, the two tables)"""
    parts = np.zeros(0, PART) if len(parts) == 0 else np.asarray(parts, PART).reshape(-1)
    pairs = np.asarray(pairs, "<u4").reshape(-1, 2)
    queries = np.zeros(0, W.QUERY_DTYPE) if len(queries) == 0 else np.asarray(queries, W.QUERY_DTYPE).reshape(-1)
    head = np.array([len(parts), folds, len(pairs), len(queries)], "<u4")
    (tmp_path / "in.bin").write_bytes(head.tobytes() + parts.tobytes() + pairs.tobytes() + queries.tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    data = (tmp_path / "out.bin").read_bytes()
    per = np.frombuffer(data, W.JOINT_DTYPE, len(parts))
    at = per.nbytes
    rest = np.frombuffer(data, W.JOINT_DTYPE, 2, at)
    at += rest.nbytes
    keyed = np.frombuffer(data, PAIR_OUT, len(pairs), at)
    at += keyed.nbytes
    answers = np.frombuffer(data, QUERY_OUT, len(queries), at)
    at += answers.nbytes
    first = int(np.frombuffer(data, "<u4", 1, at)[0])
    tables = np.frombuffer(data, TABLE_OUT, 2, at + 4)
    assert at + 4 + tables.nbytes == len(data)
    return per, rest[0], rest[1], keyed, answers, first, tables


def bit_loop(parts):
    """the records of a list of parts folded into one, a bit at a time: the face of lower voxel `bit` of brick `at` along `axis`"""
    rec = np.zeros(1, W.JOINT_DTYPE)[0]
    lo2, hi2, sum2 = [512] * 3, [0] * 3, [0] * 3
    for p in parts:
        for bit in range(64):
            if not (int(p["word"]) >> bit) & 1:
                continue
            centre = [2 * (4 * int(p["at"][k]) + int(LOCAL[bit, k])) + 1 + (k == p["axis"]) for k in range(3)]
            rec["faces"] += 1
            rec["by_face"][2 * int(p["axis"]) + (0 if p["flip"] else 1)] += 1
            for k in range(3):
                lo2[k], hi2[k], sum2[k] = min(lo2[k], centre[k]), max(hi2[k], centre[k]), sum2[k] + centre[k]
    key = int(parts[0]["key"])
    rec["a"], rec["b"] = key >> 13, W.REST if key & 8191 == 4096 else key & 8191
    rec["lo2"], rec["hi2"], rec["sum2"] = lo2, hi2, sum2
    return rec


def test_joint_part_fold_and_emit_against_a_bit_loop(exe, tmp_path):
    rng = np.random.default_rng(81)
    n = 240
    parts = np.zeros(n, PART)
    parts["at"] = rng.integers(0, 64, (n, 3))
    parts["at"][:8] = [[0, 0, 0], [63, 63, 63], [63, 0, 0], [0, 63, 0], [0, 0, 63], [63, 63, 0], [0, 63, 63], [63, 0, 63]]   # the tree's corners
    parts["axis"], parts["flip"] = np.arange(n) % 3, rng.integers(0, 2, n)
    on = rng.random((n, 64)) < rng.random(n)[:, None]
    on[8], on[9] = True, False
    on[9, 63] = True                                                          # full, one voxel
    on[on.sum(axis=1) == 0, 0] = True                                         # (a part has a face)
    parts["word"] = (on.astype(np.uint64) << BITS.astype(np.uint64)).sum(axis=1, dtype=np.uint64)
    parts["key"] = (rng.integers(0, 4096, n) << 13) | rng.integers(0, 4097, n)
    parts["key"][1] = (4095 << 13) | 4096                                     # the last cell against REST
    per, folded, _, _, _, _, _ = run(exe, tmp_path, parts)
    for p, got in zip(parts, per):
        assert got.tobytes() == bit_loop([p]).tobytes(), p
    assert folded.tobytes() == bit_loop(parts).tobytes()
    # every single voxel on every axis, both directions
    singles = np.zeros(64 * 6, PART)
    singles["word"] = np.uint64(1) << np.tile(BITS, 6).astype(np.uint64)
    singles["axis"], singles["flip"], singles["at"], singles["key"] = np.repeat(np.arange(6) >> 1, 64), np.repeat(np.arange(6) & 1, 64), (17, 0, 63), 5 << 13 | 9
    per, _, _, _, _, _, _ = run(exe, tmp_path, singles)
    for p, got in zip(singles, per):
        assert got.tobytes() == bit_loop([p]).tobytes()


def test_fold_whose_sums_pass_two_to_the_thirty_two(exe, tmp_path):
    part = np.zeros(1, PART)
    part["word"], part["axis"], part["at"], part["key"] = (1 << 64) - 1, 1, (63, 62, 63), (3 << 13) | 4096
    folds = 1 << 18
    per, _, many, _, _, _, _ = run(exe, tmp_path, part, folds=folds)
    one = bit_loop(part)
    assert per[0].tobytes() == one.tobytes() and (int(one["a"]), int(one["b"])) == (3, W.REST)
    assert int(many["faces"]) == 64 * folds == int(many["by_face"][3]) and many["lo2"].tolist() == one["lo2"].tolist() and many["hi2"].tolist() == one["hi2"].tolist()
    assert [int(v) for v in many["sum2"]] == [folds * int(v) for v in one["sum2"]] and min(int(v) for v in many["sum2"]) > 1 << 32


def test_pair_keys_order_like_the_records(exe, tmp_path):
    groups = [0, 1, 2, 254, 255, 4094, 4095, W.REST]
    pairs = [(g, n) for g in groups for n in groups if g != n]
    _, _, _, keyed, _, _, _ = run(exe, tmp_path, pairs=pairs)
    for (g, n), got in zip(pairs, keyed):
        assert (int(got["a"]), int(got["b"]), bool(got["flip"])) == (min(g, n), max(g, n), g > n) and int(got["key"]) < 1 << 25
    by_key = sorted(range(len(pairs)), key=lambda i: int(keyed["key"][i]))
    by_pair = sorted(range(len(pairs)), key=lambda i: W.pair_key(min(pairs[i]), max(pairs[i])))
    assert [sorted(pairs[i]) for i in by_key] == [sorted(pairs[i]) for i in by_pair]                 # the packing's order is the records' order, REST last
    assert all(int(keyed["key"][i]) == int(keyed["key"][j]) for i, (g, n) in enumerate(pairs) for j in [pairs.index((n, g))])


def test_queries_are_refused_as_the_witness_says(exe, tmp_path):
    def query(group=W.MATERIALS, flags=0, palette=-1, lo=(0, 0, 0), hi=(255, 255, 255), reserved=(0, 0)):
        return (48, group, flags, palette, lo, hi, reserved)
    cases = [query(), query(group=1), query(group=2), query(group=0xFFFFFFFF), query(flags=1), query(reserved=(1, 0)), query(reserved=(0, 5)),
             query(palette=0), query(palette=-2), query(palette=254), query(lo=(256, 0, 0)), query(hi=(255, 255, 1000)), query(lo=(9, 9, 9), hi=(9, 9, 9)),
             query(lo=(17, 40, 3), hi=(200, 41, 255), group=W.CELLS), query(lo=(5, 0, 0), hi=(4, 255, 255)), query(lo=(0, 0, 255), hi=(0, 0, 0))]
    queries = np.array(cases, W.QUERY_DTYPE)
    _, _, _, _, answers, _, _ = run(exe, tmp_path, queries=queries)
    for q, a in zip(queries, answers):
        assert bool(a["refused"]) == W.refused(int(q["group"]), int(q["flags"]), int(q["palette"]), q["reserved"].tolist()), q
        if a["refused"]:
            continue
        box = W.clip((q["lo"].tolist(), q["hi"].tolist()))
        assert a["group"] == q["group"] and bool(a["empty"]) == (box is None)
        if box is not None:
            assert a["lo"].tolist() == box[0] and a["hi"].tolist() == box[1]
            assert a["box_lo"].tolist() == [v >> 4 for v in box[0]] and a["box_hi"].tolist() == [v >> 4 for v in box[1]]
    assert answers["refused"].sum() == 8 and answers["empty"].sum() == 3


def test_table_holds_every_material_pair_and_reports_a_full_one(exe, tmp_path):
    _, _, _, _, _, first, tables = run(exe, tmp_path)
    whole, smallest = tables
    # the first table of a whole-tree call: every MATERIALS pair at a load below one half, found again, with short probes
    assert first == 16 and int(whole["keys"]) == 255 * 254 // 2 == 32385 == int(whole["inserted"]) == int(whole["found"]) and int(whole["full"]) == 0
    assert int(whole["longest"]) < 128                                       # (kJointMaxProbes: no pair of a whole-tree MATERIALS call is given up)
    # more keys than slots: what fits is found again, the rest is reported
    assert int(smallest["keys"]) == 1200 and int(smallest["inserted"]) <= 1024 and int(smallest["full"]) == 1200 - int(smallest["inserted"]) > 0
    assert int(smallest["found"]) == int(smallest["inserted"])
