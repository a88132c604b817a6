"""dust_amd/csrc/mesh_rule.hpp (the row functions the kernels of mesh.hip run) and the mesh records of dust_amd/csrc/model_records.hpp
(device_mesh, mesh_result) run as native code on a CPU: tests/cpp/mesh_rule_test.cpp compiled with g++ under AddressSanitizer and UBSan
into a program of its own, fed bit planes on stdin and held to the witness (tests/mesh_witness.py): a slice is handed to the witness
as a one-voxel-thick slab seen from +x, where every solid voxel shows its face, v is y and u is z."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import mesh_witness as W
import surface_witness as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "mesh_rule_test.cpp")
ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mesh_rule") / "mesh_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, lines):
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return [[int(v) for v in line.split()[1:]] for line in done.stdout.splitlines()]


def words(bits):
    """rows of 256 flags -> rows of eight 32-bit words, bit u & 31 of word u >> 5"""
    return np.packbits(np.asarray(bits, bool), axis=-1, bitorder="little").view("<u4")


def planes(slab, any_palette):
    """F, J, K of a slab[v, u] of bytes (0: the face is not in F), from their definitions"""
    f = slab != 0
    j, k = np.zeros_like(f), np.zeros_like(f)
    j[:, 1:] = f[:, 1:] & f[:, :-1] & (any_palette | (slab[:, 1:] == slab[:, :-1]))
    k[1:] = f[1:] & f[:-1] & (any_palette | (slab[1:] == slab[:-1]))
    return f, j, k


def slice_lines(slab, any_palette, stride=8, heights=1):
    f, j, k = (words(p) for p in planes(slab, any_palette))
    return [f"slice {len(slab)} {stride} {heights}"] + [" ".join(str(v) for v in np.concatenate([f[v], j[v], k[v]])) for v in range(len(slab))]


def witness_quads(slab, any_palette):
    """(v0, u0, u1, v1) in the documented order"""
    grid = np.zeros((1, 256, 256), np.uint8)
    grid[0, :len(slab)] = slab
    result, quads = W.mesh(grid, faces=S.POS_X, any_palette=any_palette)
    key = quads["key"].astype(np.int64)
    v0, u0 = (key >> 8) & 255, key & 255
    return [list(q) for q in zip(v0.tolist(), u0.tolist(), (u0 + quads["du"]).tolist(), (v0 + quads["dv"]).tolist())], result


def check_slab(exe, slab, any_palette, stride=8):
    want, result = witness_quads(slab, any_palette)
    got = run(exe, slice_lines(slab, any_palette, stride))
    assert got[-1] == [len(want)] == [int(result["quads"])] and got[:-1] == want, (got[:3], want[:3])
    flat = run(exe, slice_lines(slab, any_palette, stride, heights=0))             # the count-only walk: the same quads, no heights
    assert flat[-1] == got[-1] and flat[:-1] == [[v0, u0, u1, v0] for v0, u0, u1, _ in want]
    return want


@pytest.mark.parametrize("density", [0.5, 0.9, 0.97])
def test_random_slices_against_the_witness(exe, density):
    rng = np.random.default_rng(int(density * 100))
    merged = 0
    for materials, rows, stride in ((1, 256, 8), (3, 256, 9), (2, 37, 8)):
        slab = np.where(rng.random((rows, 256)) < density, rng.integers(1, materials + 1, (rows, 256)), 0).astype(np.uint8)
        for any_palette in (False, True):
            want = check_slab(exe, slab, any_palette, stride)
            merged += sum(1 for v0, _, _, v1 in want if v1 > v0)
    assert merged > 0


def test_row_ends_word_edges_and_runs_that_must_not_merge(exe):
    slab = np.zeros((256, 256), np.uint8)
    slab[0, :] = 1                                                               # bit 0 .. bit 255, the first row
    slab[2:5, :] = 1                                                             # ... three rows of it: one quad 256 x 3
    slab[6, 0:1], slab[6, 255:256] = 1, 1                                        # single bits at both ends
    slab[8, 20:32], slab[9, 20:33], slab[10, 20:33] = 1, 1, 1                    # ends at 31; crosses 31 | 32 twice: the first does not merge
    slab[12:14, 60:70] = 1                                                       # crosses 63 | 64
    slab[12:14, 32:40] = 2                                                       # starts at bit 0 of a word
    slab[16, 100:140], slab[17, 100:120], slab[18, 100:120] = 1, 1, 1            # under a longer run over the same start: only the lower two merge
    slab[20, 90:130], slab[21, 100:130] = 1, 1                                   # the same end, another start
    slab[23, 200:210], slab[24, 200:210] = 1, 2                                  # identical runs of two materials
    slab[26:28, 150:160] = 1
    slab[26:28, 155] = 2                                                         # a stripe cuts the run in three
    slab[254:256, 250:256] = 3                                                   # the last rows, the last bits
    want = check_slab(exe, slab, False)
    for quad in ([0, 0, 255, 0], [2, 0, 255, 4], [6, 0, 0, 6], [6, 255, 255, 6], [8, 20, 31, 8], [9, 20, 32, 10], [12, 60, 69, 13], [12, 32, 39, 13],
                 [16, 100, 139, 16], [17, 100, 119, 18], [20, 90, 129, 20], [21, 100, 129, 21], [23, 200, 209, 23], [24, 200, 209, 24],
                 [26, 150, 154, 27], [26, 155, 155, 27], [26, 156, 159, 27], [254, 250, 255, 255]):
        assert quad in want, quad
    merged = check_slab(exe, slab, True, stride=9)
    assert [23, 200, 209, 24] in merged and [26, 150, 159, 27] in merged and [12, 32, 39, 13] in merged and [12, 60, 69, 13] in merged
    assert len(merged) == len(want) - 1 - 2                                      # the two stacked runs become one quad, the three striped ones too


def test_all_ones_and_all_zero_planes(exe):
    assert check_slab(exe, np.ones((256, 256), np.uint8), False) == [[0, 0, 255, 255]]
    assert check_slab(exe, np.ones((256, 256), np.uint8), True, stride=9) == [[0, 0, 255, 255]]
    assert check_slab(exe, np.zeros((256, 256), np.uint8), False) == []
    stripes = np.tile(np.array([1, 2], np.uint8), (256, 128))                    # every run one bit long, every quad 256 high
    assert check_slab(exe, stripes, False) == [[0, u, u, 255] for u in range(256)]
    checker = (np.indices((256, 256)).sum(axis=0) & 1).astype(np.uint8)          # nothing merges
    assert len(check_slab(exe, checker, True)) == 256 * 128


def test_join_and_run_end(exe):
    rng = np.random.default_rng(5)
    rows = [np.zeros(256, bool), np.ones(256, bool)] + [rng.random(256) < p for p in (0.5, 0.9, 0.99)]
    got = run(exe, ["j " + " ".join(str(v) for v in words(r)) for r in rows])
    for r, row in zip(rows, got):
        want = np.zeros(256, bool)
        want[1:] = r[1:] & r[:-1]
        assert row == words(want).tolist()
    cases = []
    for r in rows:
        j = np.zeros(256, bool)
        j[1:] = r[1:] & r[:-1]
        for u0 in [0, 30, 31, 32, 62, 63, 64, 254, 255] + rng.integers(0, 256, 20).tolist():
            end = u0
            while end + 1 < 256 and j[end + 1]:
                end += 1
            cases.append((u0, j, end))
    got = run(exe, [f"e {u0} " + " ".join(str(v) for v in words(j)) for u0, j, _ in cases])
    assert [row[0] for row in got] == [end for _, _, end in cases]


def brick_word(flags):
    """a 4^3 boolean cube -> its word: bit x << 4 | y << 2 | z"""
    return sum(1 << ((x << 4) | (y << 2) | z) for x, y, z in np.argwhere(flags).tolist())


def test_brick_words_axes_and_records(exe):
    rng = np.random.default_rng(6)
    cubes = [rng.random((4, 4, 4)) < p for p in (0.2, 0.5, 0.9)] + [np.ones((4, 4, 4), bool), np.zeros((4, 4, 4), bool)]
    cases = [(cube, n, c) for cube in cubes for n in range(3) for c in range(4)]
    got = run(exe, [f"n {brick_word(cube)} {n} {c}" for cube, n, c in cases])
    for (cube, n, c), row in zip(cases, got):
        n_axis, v_axis, u_axis = W.AXES[n]
        rows = np.moveaxis(cube, (n_axis, v_axis, u_axis), (0, 1, 2))[c]          # [v, u]
        assert row == [sum(int(rows[j, i]) << i for i in range(4)) for j in range(4)], (n, c)
    got = run(exe, [f"p {n} {c}" for n in range(3) for c in range(4)])
    for (n, c), (plane,) in zip(itertools.product(range(3), range(4)), got):
        assert plane == brick_word(np.indices((4, 4, 4))[n] == c)
    # E_d of a brick needs the word across d only: against the witness on a 12^3 block, off the block empty or walls
    for walls in (False, True):
        grid = np.where(rng.random((12,) * 3) < 0.6, 1, 0).astype(np.uint8)
        exposed = S.exposure(grid, walls)
        cases = []
        for b in itertools.product(range(3), repeat=3):
            for d, step in enumerate(S.STEPS):
                nb = tuple(p + q for p, q in zip(b, step))
                inside = all(0 <= p < 3 for p in nb)
                cut = lambda at: tuple(slice(4 * p, 4 * p + 4) for p in at)
                across = brick_word(grid[cut(nb)] != 0) if inside else (ONES if walls else 0)
                cases.append((brick_word(grid[cut(b)] != 0), across, d, brick_word((exposed[cut(b)] >> d) & 1 == 1)))
        got = run(exe, [f"x {own} {across} {d}" for own, across, d, _ in cases])
        assert [row[0] for row in got] == [want for _, _, _, want in cases]
    got = run(exe, [f"a {n} 7 100 200" for n in range(3)])
    assert got == [[7, 200, 100], [200, 7, 100], [200, 100, 7]]                   # (s, u, v) = (7, 100, 200): x: u = z, v = y; y: u = z, v = x; z: u = y, v = x
    quads = np.zeros(3, W.QUAD_DTYPE)
    quads[0] = ((7 << 16) | (200 << 8) | 100, 1, 254, 155, 55)
    quads[1] = ((200 << 16) | (7 << 8) | 0, 2, 0, 255, 0)
    quads[2] = ((0 << 16) | (0 << 8) | 255, 5, 9, 255, 255)
    got = run(exe, ["c 1 7 100 255 200 255 254", "c 2 7 0 255 200 200 0", "c 5 255 0 255 0 255 9"])
    assert [row[0] for row in got] == quads.view("<u8").tolist()


def test_query_validation_table_and_clipping(exe):
    queries = [(faces, flags, palette, lo, hi)
               for faces in (0, 1, 8, 63, 64, 0xFFFFFFFF) for flags in (0, 1, 2, 3, 4, 7, 1 << 31) for palette in (-2, -1, 0, 254, 255)
               for lo, hi in (((0, 0, 0), (255, 255, 255)), ((17, 3, 250), (40, 3, 255)), ((5, 5, 5), (4, 9, 9)), ((0, 256, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 4000)))]
    got = run(exe, ["m " + " ".join(str(v) for v in (faces, flags, palette) + lo + hi) for faces, flags, palette, lo, hi in queries])
    accepted = 0
    for (faces, flags, palette, lo, hi), row in zip(queries, got):
        if W.refused(faces, flags, palette, lo, hi):
            assert row == [0], (faces, flags, palette, lo, hi)
            continue
        accepted += 1
        empty = any(l > h for l, h in zip(lo, hi))
        assert row[:6] == [1, int(empty), faces, flags & 1, palette + 1, (flags >> 1) & 1]
        assert row[6:] == ([] if empty else list(lo) + list(hi))
    assert 0 < accepted < len(queries)


def test_result_record(exe):
    acc = [1, 2, 3, 4, 5, 6, 10, 20, 30, 40, 50, 60, 17]
    got = run(exe, ["r", "r " + " ".join(str(v) for v in acc)])
    zero = W.zero_result()
    assert got[0] == [0] * 16 and zero.tobytes() == bytes(64)                    # the zero result is all zero bytes
    assert got[1] == [21, 210, 1, 2, 3, 4, 5, 6, 10, 20, 30, 40, 50, 60, 17, 0]
