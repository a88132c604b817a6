"""dust_amd/csrc/hierarchy.hpp, the host build of a model's upper levels (what dust_hip_model_create uploads), run as native code on a
CPU: tests/cpp/hierarchy_test.cpp compiled with g++ under AddressSanitizer and UBSan (no HIP compiler, not linked against the library)
reads blocks from a file and writes the root, the l2 nodes and cells, the mid nodes, dense_mask and the bounds -- or the refusal -- to
another. Every byte is held to tests/hierarchy_witness.py, and the witness's descend() must find every block, and only those, in both."""
import os
import subprocess

import numpy as np
import pytest

import hierarchy_witness as HW
from dust_amd import synth
from dust_amd.api import BLOCK_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "hierarchy_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "hierarchy_test")
INVALID = -1
FULL = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe():
    """built once, again when the program or a header it includes is newer (as tests/test_model_records.py caches its binary)"""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "dust_hip.h")] + [os.path.join(CSRC, h) for h in ("hierarchy.hpp", "dust_dev.h", "vdb.hpp")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE])   # (no HIP include path: the header needs none)
    return EXE


def run(exe, tmp_path, blocks, extent_log2):
    """one run of the program (which must end clean under both sanitizers) -> ("refused", message) or the arrays as the witness names them"""
    blocks = np.ascontiguousarray(blocks, BLOCK_DTYPE).reshape(-1)
    (tmp_path / "in.bin").write_bytes(np.array([extent_log2, len(blocks)], "<u4").tobytes() + blocks.tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    data = (tmp_path / "out.bin").read_bytes()
    at = 0

    def take(dtype, n=1):
        nonlocal at
        a = np.frombuffer(data, dtype, n, at)
        at += a.nbytes
        return a
    status = int(take("<i4")[0])
    if status != 0:
        message = bytes(take(np.uint8, int(take("<u4")[0]))).decode()
        assert at == len(data)
        return status, message
    n_mid, n_l2, n_dense, n_cells = (int(v) for v in take("<u4", 4))
    r = dict(extent_log2=extent_log2, n_mid=n_mid, n_l2=n_l2, bmin=take("<f4", 3), bmax=take("<f4", 3), root=take(np.uint8, HW.N16_BYTES),
             l2=take(np.uint8, n_l2 * HW.N16_BYTES), mid=take(HW.MID_DTYPE, n_mid), dense_mask=take("<u8", n_dense), l2_cells=take(HW.L2_CELL_DTYPE, n_cells))
    assert at == len(data) and n_dense == n_mid * 64 and n_cells == (n_l2 * 4096 if extent_log2 == 12 else 0)
    return 0, r


def blocks_of(want):
    """the witness's block order as the caller's records (material_ptr and avg_albedo play no part in the upper levels)"""
    blocks = np.zeros(len(want["block_mask"]), BLOCK_DTYPE)
    blocks["x"], blocks["y"], blocks["z"] = want["block_xyz"].T
    blocks["mask"] = want["block_mask"]
    return blocks


ARRAYS = ("root", "l2", "mid", "dense_mask", "l2_cells", "bmin", "bmax")


def same_bytes(got, want, what=""):
    assert (got["n_mid"], got["n_l2"]) == (want["n_mid"], want["n_l2"]), what
    for name in ARRAYS:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), f"{what}: {name} differs"


def check_descent(arrays, bricks, extent_log2, rng=None, max_empty=4000):
    keys = {(int(x) >> 2, int(y) >> 2, int(z) >> 2): i for i, (x, y, z) in enumerate(arrays_order(bricks, extent_log2))}
    assert len(keys) == len(bricks)
    for k, i in keys.items():
        assert HW.descend(arrays, *k) == i, k
    empty = HW.probes(bricks, extent_log2, rng)
    if len(empty) > max_empty:
        empty = [empty[i] for i in np.random.default_rng(1).choice(len(empty), max_empty, replace=False)] + \
            [c for c in empty if all(v in (0, (1 << (extent_log2 - 2)) - 1) for v in c)]
    for k in empty:
        assert HW.descend(arrays, *k) == -1, k
    return len(empty)


def arrays_order(bricks, extent_log2):
    return HW.build(bricks, extent_log2)["block_xyz"]


def accepted(exe, tmp_path, bricks, extent_log2, rng=None):
    """program == witness byte for byte, and descend() finds every block and no other brick in either"""
    want = HW.build(bricks, extent_log2)
    status, got = run(exe, tmp_path, blocks_of(want), extent_log2)
    assert status == 0, got
    same_bytes(got, want)
    assert check_descent(want, bricks, extent_log2, rng) > 0
    check_descent(got, bricks, extent_log2, rng)
    return want, got


def prefixes(node):
    return np.asarray(node[512:640]).view("<u2")


def test_no_blocks(exe, tmp_path):
    want, got = accepted(exe, tmp_path, {}, 8)
    assert got["n_mid"] == 0 and not got["root"].any() and not got["bmin"].any() and not got["bmax"].any()
    assert len(got["mid"]) == 0 and len(got["dense_mask"]) == 0


def test_one_brick_at_the_origin(exe, tmp_path):
    want, got = accepted(exe, tmp_path, {(0, 0, 0): 1}, 8)
    assert got["root"][0] == 1 and not got["root"][1:512].any() and prefixes(got["root"]).tolist() == [0] + [1] * 63 and not got["root"][640:].any()
    assert got["mid"].tolist() == [(1, 0, 0, 0)] and got["dense_mask"][0] == 1 and not got["dense_mask"][1:].any()
    assert got["bmin"].tolist() == [0, 0, 0] and got["bmax"].tolist() == [4, 4, 4]


def test_one_brick_in_the_last_corner(exe, tmp_path):
    """(252, 252, 252): root bit 4095 -- word 63, bit 63 --, mid bit 63"""
    want, got = accepted(exe, tmp_path, {(63, 63, 63): 1 << 63}, 8)
    assert got["root"][511] == 0x80 and not got["root"][:511].any() and not got["root"][512:].any()
    assert got["mid"].tolist() == [(0, 1 << 31, 0, 0)] and got["dense_mask"][63] == 1 << 63
    assert got["bmin"].tolist() == [252] * 3 and got["bmax"].tolist() == [256] * 3


def test_every_root_cell_occupied(exe, tmp_path):
    rng = np.random.default_rng(5)
    bricks = {}
    for cell in range(4096):
        sub = rng.integers(0, 4, 3)
        bricks[(int((cell >> 8) * 4 + sub[0]), int(((cell >> 4) & 15) * 4 + sub[1]), int((cell & 15) * 4 + sub[2]))] = int(rng.integers(1, 1 << 63))
    want, got = accepted(exe, tmp_path, bricks, 8)
    assert got["n_mid"] == 4096 and (got["root"][:512] == 0xFF).all()
    assert prefixes(got["root"]).tolist() == list(range(0, 4096, 64)) and prefixes(got["root"])[-1] == 4032
    assert got["mid"]["first_block"].tolist() == list(range(4096))


def test_one_root_cell_full(exe, tmp_path):
    bricks = {(20 + x, 40 + y, 60 + z): FULL for x in range(4) for y in range(4) for z in range(4)}
    want, got = accepted(exe, tmp_path, bricks, 8)
    assert got["mid"].tolist() == [(0xFFFFFFFF, 0xFFFFFFFF, 0, 0)] and (got["dense_mask"] == np.uint64(FULL)).all()
    assert got["bmin"].tolist() == [80, 160, 240] and got["bmax"].tolist() == [96, 176, 256]


def test_mid_bits_on_both_sides_of_the_word_boundary(exe, tmp_path):
    """mid bits 0, 31, 32 and 63: the last of mask_lo, the first of mask_hi"""
    def brick(cell, bit):
        return (cell[0] * 4 + (bit >> 4), cell[1] * 4 + ((bit >> 2) & 3), cell[2] * 4 + (bit & 3))
    bricks = {brick((3, 7, 11), bit): 0x8000000000000001 + bit for bit in (0, 31, 32, 63)}
    bricks.update({brick((3, 7, 12), 31): 5, brick((4, 0, 0), 32): 6})
    want, got = accepted(exe, tmp_path, bricks, 8)
    assert got["mid"].tolist() == [(0x80000001, 0x80000001, 0, 0), (0x80000000, 0, 4, 0), (0, 1, 5, 0)]


def random_model(rng, n_sparse=2500):
    """a sparse model over the whole tree plus a slab of full bricks: a few thousand bricks"""
    bricks = {tuple(int(v) for v in c): int(rng.integers(1, 1 << 63)) | int(rng.integers(0, 2)) << 63 for c in rng.integers(0, 64, (n_sparse, 3))}
    bricks.update({(x, 30, z): FULL for x in range(10, 40) for z in range(5, 35)})
    return bricks


def test_random_sparse_model_with_a_dense_slab(exe, tmp_path):
    rng = np.random.default_rng(6)
    bricks = random_model(rng)
    want, got = accepted(exe, tmp_path, bricks, 8, rng)
    assert 3000 < len(bricks) < 4000 and 1500 < got["n_mid"] < 4096


def test_deep_procedural_blocks(exe, tmp_path):
    blocks, _ = synth.procedural_deep_blocks(occupancy=1e-7, sample=True)
    bricks = {(int(b["x"]) >> 2, int(b["y"]) >> 2, int(b["z"]) >> 2): int(b["mask"]) for b in blocks}
    assert 80 < len(bricks) == len(blocks)
    want = HW.build(bricks, 12)
    assert blocks_of(want)[["x", "y", "z", "mask"]].tolist() == blocks[["x", "y", "z", "mask"]].tolist()   # the generator's order is iter_leaf order
    want, got = accepted(exe, tmp_path, bricks, 12, np.random.default_rng(7))
    assert got["n_l2"] > 50 and got["n_mid"] >= got["n_l2"]


def test_deep_far_corners(exe, tmp_path):
    want, got = accepted(exe, tmp_path, {(0, 0, 0): 3, (1023, 1023, 1023): 1 << 63}, 12)
    assert got["n_l2"] == 2 and got["n_mid"] == 2
    assert got["root"][0] == 1 and got["root"][511] == 0x80 and prefixes(got["root"])[63] == 1
    assert got["l2"][640:644].view("<u4")[0] == 0 and got["l2"][HW.N16_BYTES + 640:HW.N16_BYTES + 644].view("<u4")[0] == 1
    assert got["l2_cells"][0].tolist() == (0, 0, 1) and got["l2_cells"][4096 + 4095].tolist() == (1, 3 | 3 << 2 | 3 << 4 | 3 << 6 | 3 << 8 | 3 << 10, 1 << 63)
    assert got["l2_cells"][1].tolist() == (HW.EMPTY_CELL, 0, 0)
    assert got["bmin"].tolist() == [0] * 3 and got["bmax"].tolist() == [4096] * 3


def test_deep_two_l2_cells_with_several_mid_nodes(exe, tmp_path):
    """the second l2 node's child_base is the number of the first one's mid nodes; bounds with lo != 0 and hi != 3"""
    def brick(top, c16, sub):
        return tuple(top[k] * 64 + c16[k] * 4 + sub[k] for k in range(3))
    bricks = {}
    for c16 in ((0, 0, 0), (3, 9, 15), (15, 15, 15)):
        for sub in ((1, 2, 1), (2, 2, 3), (1, 1, 2)):
            bricks[brick((2, 5, 7), c16, sub)] = 0x10 + sub[0]
    for c16 in ((0, 1, 0), (8, 8, 8), (8, 8, 9), (15, 0, 4)):
        bricks[brick((9, 0, 15), c16, (2, 1, 2))] = 7
        bricks[brick((9, 0, 15), c16, (2, 2, 1))] = 9
    want, got = accepted(exe, tmp_path, bricks, 12)
    assert got["n_l2"] == 2 and got["n_mid"] == 7
    assert got["l2"][HW.N16_BYTES + 640:HW.N16_BYTES + 644].view("<u4")[0] == 3
    occupied = got["l2_cells"][got["l2_cells"]["mid"] != HW.EMPTY_CELL]
    assert occupied["mid"].tolist() == list(range(7))
    assert occupied["bounds"][:3].tolist() == [1 | 1 << 2 | 1 << 4 | 2 << 6 | 2 << 8 | 3 << 10] * 3
    assert occupied["bounds"][3:].tolist() == [2 | 1 << 2 | 1 << 4 | 2 << 6 | 2 << 8 | 2 << 10] * 4


REFUSALS = [
    ("unaligned", [(4, 8, 12), (16, 18, 20)], 8, "block position is not a 4-aligned coordinate inside the tree extent"),
    ("at the extent", [(4, 8, 12), (252, 256, 252)], 8, "block position is not a 4-aligned coordinate inside the tree extent"),
    ("at the deep extent", [(4096, 0, 0)], 12, "block position is not a 4-aligned coordinate inside the tree extent"),
    ("far outside", [(65532, 65532, 65532)], 8, "block position is not a 4-aligned coordinate inside the tree extent"),
    ("empty mask", [(4, 8, 12), (16, 20, 24, 0)], 8, "block with empty occupancy mask"),
    ("out of order", [(16, 20, 24), (4, 8, 12)], 8, "blocks are not in Tree::iter_leaf order (depth-first, ascending child bits)"),
    ("row-major, not depth first", [(0, 0, 16), (0, 4, 0)], 8, "blocks are not in Tree::iter_leaf order (depth-first, ascending child bits)"),
    ("deep out of order", [(256, 0, 0), (0, 0, 4092)], 12, "blocks are not in Tree::iter_leaf order (depth-first, ascending child bits)"),
    ("duplicate", [(4, 8, 12), (4, 8, 12)], 8, "blocks are not in Tree::iter_leaf order (depth-first, ascending child bits)"),
    ("duplicate of the first block at the origin", [(0, 0, 0), (0, 0, 0)], 8, "blocks are not in Tree::iter_leaf order (depth-first, ascending child bits)"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(exe, tmp_path, case):
    _, records, extent_log2, message = case
    blocks = np.zeros(len(records), BLOCK_DTYPE)
    for b, r in zip(blocks, records):
        b["x"], b["y"], b["z"] = r[:3]
        b["mask"] = r[3] if len(r) > 3 else 1
    assert run(exe, tmp_path, blocks, extent_log2) == (INVALID, message)


def test_witness_helpers_agree():
    """the grid helper and the voxel helper name the same bricks, with bit x << 4 | y << 2 | z"""
    rng = np.random.default_rng(8)
    xyz = rng.integers(0, 256, (500, 3))
    grid = np.zeros((256, 256, 256), np.uint8)
    grid[xyz[:, 0], xyz[:, 1], xyz[:, 2]] = 9
    assert HW.bricks_of_grid(grid) == HW.bricks_of_voxels(xyz.tolist())
    assert HW.bricks_of_voxels([(5, 2, 3), (4, 0, 1)]) == {(1, 0, 0): 1 << (16 + 8 + 3) | 1 << 1}
