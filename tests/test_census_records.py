"""The device-free half of dust_hip_model_census run as native code on a CPU: tests/cpp/census_records_test.cpp compiled with g++
-ffp-contract=off under AddressSanitizer and UBSan into a program of its own (no HIP compiler, not linked against the library). It
drives shape_bounds, device_census_shape, census_record, census_records and census_tables of dust_amd/csrc/model_records.hpp and the
membership text of dust_amd/csrc/shape_cover.hpp -- the one text k_edit_shapes and k_census run -- and is held to device_shape, to
tests/census_witness.py and, voxel by voxel, to tests/shape_edit_witness.py's coverage on shapes whose surfaces pass exactly through
voxel centres."""
import os
import subprocess

import numpy as np
import pytest

import census_witness as W
import shape_edit_witness as SW
from test_model_records import DEV_SHAPE, edge_shapes, random_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "census_records_test.cpp")

ACC = np.dtype([("covered", "<u4"), ("solid", "<u4"), ("lo", "<u4", 3), ("hi", "<u4", 3), ("sum", "<u8", 3)])
ACC_CASE = np.dtype([("live", "<u4"), ("pad", "<u4"), ("acc", ACC)])
COVER_CASE = np.dtype([("shape", SW.SHAPE_DTYPE), ("lo", "<u4", 3), ("hi", "<u4", 3)])
SHAPE_OUT = np.dtype([("bounds_live", "<u4"), ("lo", "<u4"), ("hi", "<u4"), ("shape_live", "<u4"), ("shape", DEV_SHAPE), ("census_live", "<u4"),
                      ("census", DEV_SHAPE)])
assert (ACC.itemsize, ACC_CASE.itemsize, COVER_CASE.itemsize) == (56, 64, 72)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("census_records") / "census_records_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out])
    return out


def run(exe, tmp_path, shapes=(), accs=(), index=(), covers=()):
    """one run of the program (which must end clean under both sanitizers) -> what it wrote, parsed"""
    shapes = np.zeros(0, SW.SHAPE_DTYPE) if len(shapes) == 0 else np.asarray(shapes, SW.SHAPE_DTYPE).reshape(-1)
    accs = np.zeros(0, ACC_CASE) if len(accs) == 0 else np.asarray(accs, ACC_CASE).reshape(-1)
    covers = np.zeros(0, COVER_CASE) if len(covers) == 0 else np.asarray(covers, COVER_CASE).reshape(-1)
    index = np.asarray(index, "<u4").reshape(-1)
    head = np.array([len(shapes), len(accs), len(index), len(covers)], "<u4")
    (tmp_path / "in.bin").write_bytes(b"".join(a.tobytes() for a in (head, shapes, accs, index, covers)))
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    data, at = (tmp_path / "out.bin").read_bytes(), 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(data, dtype, n, at)
        at += a.nbytes
        return a
    r = {"shapes": take(SHAPE_OUT, len(shapes)), "records": take(W.RECORD_DTYPE, len(accs)), "scattered": take(W.RECORD_DTYPE, len(accs)),
         "tables": take("<u4", len(accs) * 256).reshape(-1, 256), "covers": []}
    for c in covers:
        live = int(take("<u4", 1)[0])
        size = tuple(int(h) - int(l) for l, h in zip(c["lo"], c["hi"]))
        r["covers"].append(take("u1", size[0] * size[1] * size[2]).reshape(size).astype(bool) if live else None)
    assert at == len(data)
    return r


def test_bounds_helper_is_device_shapes_half(exe, tmp_path):
    rng = np.random.default_rng(51)
    shapes = np.concatenate([edge_shapes(), random_shapes(rng, 400, -30.0, 286.0, 20.0), random_shapes(rng, 40, 100.0, 156.0, 120.0)])
    odd = shapes[40:80].copy()      # what a census does not look at, valid or not
    odd["op"], odd["palette"], odd["reserved"] = rng.integers(4, 1 << 31, 40), rng.integers(-(1 << 31), 1 << 31, 40), rng.integers(0, 1 << 32, (40, 2))
    got = run(exe, tmp_path, shapes=np.concatenate([shapes, odd]))["shapes"]
    plain, strange = got[:len(shapes)], got[len(shapes):]
    # false exactly where device_shape is false, and the same lo / hi
    assert np.array_equal(plain["bounds_live"], plain["shape_live"]) and np.array_equal(plain["bounds_live"], plain["census_live"])
    live = plain["bounds_live"] == 1
    assert np.array_equal(plain["lo"][live], plain["shape"]["lo"][live]) and np.array_equal(plain["hi"][live], plain["shape"]["hi"][live])
    assert 30 < np.count_nonzero(~live) < len(shapes) // 2
    # ... and exactly where the witness says the shape covers nothing or lies wholly outside the tree
    for s, g in zip(shapes, plain):
        if not g["bounds_live"]:
            assert not SW.coverage(s)[1].any(), s
        else:
            assert not SW.covers_nothing(s), s
    # the census record: the same bounds and geometry, the two operation bytes 0
    for name in ("a", "kind", "b", "radius", "lo", "hi"):
        assert plain["census"][name][live].tobytes() == plain["shape"][name][live].tobytes(), name
    assert not plain["census"]["solid_to"].any() and not plain["census"]["empty_to"].any() and plain["shape"]["empty_to"][live].any()
    # op, palette and reserved change nothing
    assert strange["bounds_live"].tobytes() == plain["bounds_live"][40:80].tobytes() and strange["census"].tobytes() == plain["census"][40:80].tobytes()


def test_census_record_and_scatter(exe, tmp_path):
    rng = np.random.default_rng(52)
    n = 300
    accs = np.zeros(n, ACC_CASE)
    accs["live"] = rng.random(n) < 0.8
    accs["live"][:4] = 1
    a = accs["acc"]
    a["covered"] = rng.integers(1, 1 << 24, n)
    a["solid"] = np.where(rng.random(n) < 0.3, 0, rng.integers(1, 1 << 24, n))
    a["lo"], a["hi"] = rng.integers(0, 256, (n, 3)), rng.integers(0, 256, (n, 3))
    a["sum"] = rng.integers(0, 1 << 32, (n, 3)).astype(np.uint64)
    a[0] = (1 << 24, 1 << 24, (0, 0, 0), (255, 255, 255), ((1 << 24) * 255 // 2,) * 3)      # the whole tree, solid: sums above 2^31
    a[1] = (5, 0, (255, 255, 255), (0, 0, 0), (0, 0, 0))                                        # the neutral element the init kernel writes
    a[2] = (0xFFFFFFFF, 0xFFFFFFFF, (0, 255, 7), (255, 0, 9), ((1 << 64) - 1, 1 << 63, 1))
    index = np.sort(rng.choice(n, 200, replace=False)).astype(np.uint32)
    r = run(exe, tmp_path, accs=accs, index=index)

    def want(case, live):
        w = W.zero_record()
        if live:
            w["covered"], w["solid"] = case["covered"], case["solid"]
            if case["solid"]:
                w["lo"], w["hi"], w["sum"] = case["lo"], case["hi"], case["sum"]
        return w
    for i in range(n):
        assert r["records"][i].tobytes() == want(a[i], accs["live"][i]).tobytes(), i
    # scattered through index: acc[k] to place index[k], the zero record and a zero row everywhere else
    place = {int(p): k for k, p in enumerate(index)}
    for i in range(n):
        k = place.get(i)
        assert r["scattered"][i].tobytes() == want(a[k] if k is not None else a[0], k is not None).tobytes(), i
        row = np.zeros(256, np.uint32)
        if k is not None:
            row[k % 256] = k + 1
            row[255] += 7
        assert np.array_equal(r["tables"][i], row), i
    assert r["records"][0]["sum"].tolist() == [2139095040] * 3 and r["records"][1]["lo"].tolist() == [255] * 3


def boundary_shapes():
    B, S, C = SW.BOX, SW.SPHERE, SW.CAPSULE
    out = []
    for r in (0.0, 1.0, 5.0, 13.0, 25.0):      # centres on voxel centres, integer radii: (3, 4, 0) * k, (5, 12, 0), (7, 24, 0) lie exactly on the surface
        out.append(SW.shape(S, (40.5, 50.5, 60.5), radius=r))
        out.append(SW.shape(C, (40.5, 50.5, 60.5), (40.5, 50.5, 60.5), radius=r))                 # a == b: the same sphere
        out.append(SW.shape(C, (30.5, 50.5, 60.5), (50.5, 50.5, 60.5), radius=r))                 # an axis: voxel centres on the cylinder and both caps
    out.append(SW.shape(S, (40.0, 50.0, 60.0), radius=1.5))                                        # (+-1.5, +-.5, +-.5): 2.75 > 2.25; (+-.5, +-.5, +-.5): inside
    out.append(SW.shape(S, (40.0, 50.0, 60.0), radius=float(np.sqrt(np.float32(2.75)))))           # the radius rounded: whichever side numpy float32 says
    out.append(SW.shape(C, (10.5, 10.5, 10.5), (20.5, 20.5, 20.5), radius=float(np.sqrt(np.float32(0.5)))))   # a diagonal: neighbours at distance sqrt(2/3), sqrt(1/2)..
    out.append(SW.shape(C, (10.25, 10.75, 10.5), (10.25 + 1e-20, 10.75, 10.5), radius=3.0))        # l underflows to 0
    out.append(SW.shape(C, (10.5, 10.5, 10.5), (10.5 + 1e-18, 10.5 + 1e-18, 10.5), radius=2.0))    # l tiny but not 0
    out.append(SW.shape(B, (10.5, 20.5, 30.5), (12.5, 22.5, 30.5)))                                # extent exactly on voxel centres
    out.append(SW.shape(B, (10.5, 20.5, 30.5), (10.5, 20.5, 30.5)))
    out.append(SW.shape(B, (np.nextafter(np.float32(10.5), np.float32(11)), 20.0, 30.0), (np.nextafter(np.float32(12.5), np.float32(0)), 22.0, 31.0)))
    out.append(SW.shape(B, (-1e30,) * 3, (1e30,) * 3))
    # coordinates near 65 536: a thin shell of a huge sphere through the tree, a capsule from far outside, the limit itself
    out.append(SW.shape(S, (65536.0, 30.5, 30.5), radius=65281.0))
    out.append(SW.shape(S, (65536.0, 128.0, 128.0), radius=65408.5))
    out.append(SW.shape(S, (-65536.0, 100.5, 100.5), radius=65536.0))
    out.append(SW.shape(S, (128.5, -65535.5, 128.5), radius=65536.0))
    out.append(SW.shape(C, (-65536.0, 100.3, 30.1), (65536.0, 110.2, 31.7), radius=1.7))
    out.append(SW.shape(C, (65536.0, 65536.0, 65536.0), (100.5, 100.5, 100.5), radius=2.0))
    out.append(SW.shape(C, (-65000.0, 65536.0, 128.0), (65000.0, -65536.0, 128.0), radius=65536.0))
    return SW.shapes(*out)


def test_membership_text_is_the_witness_coverage(exe, tmp_path):
    rng = np.random.default_rng(53)
    shapes = np.concatenate([boundary_shapes(), random_shapes(rng, 120, -20.0, 276.0, 24.0), random_shapes(rng, 12, 100.0, 156.0, 120.0)])
    shapes = shapes[[not SW.covers_nothing(s) and SW.coverage(s)[1].size > 0 for s in shapes]]
    covers = np.zeros(len(shapes), COVER_CASE)
    covers["shape"] = shapes
    regions = [SW.region(s) for s in shapes]
    covers["lo"], covers["hi"] = [[r.start for r in reg] for reg in regions], [[r.stop for r in reg] for reg in regions]
    r = run(exe, tmp_path, shapes=shapes, covers=covers)
    on_surface = 0
    for i, (s, reg, got, bounds) in enumerate(zip(shapes, regions, r["covers"], r["shapes"])):
        want = SW.coverage(s)[1]
        if got is None:      # wholly outside the tree by the bounds: the witness covers nothing there either
            assert not bounds["bounds_live"] and not want.any(), (i, s)
            continue
        assert got.shape == want.shape and np.array_equal(got, want), (i, s, np.argwhere(got != want)[:5] + [x.start for x in reg])
        if want.any():       # the kernels cull by the bounds: nothing covered may lie outside them
            idx = np.argwhere(want) + [x.start for x in reg]
            lo, hi = [(int(bounds["lo"]) >> (8 * k)) & 255 for k in range(3)], [(int(bounds["hi"]) >> (8 * k)) & 255 for k in range(3)]
            assert np.all(idx.min(axis=0) >= lo) and np.all(idx.max(axis=0) <= hi), (i, s)
        on_surface += int(want.any())
    assert on_surface > 100
    # the cases stand on what they claim: exact hits on the surface are inside
    sphere5 = SW.covered_voxels(SW.shape(SW.SPHERE, (40.5, 50.5, 60.5), radius=5.0))
    assert (43, 54, 60) in sphere5 and (45, 50, 60) in sphere5 and (44, 54, 60) not in sphere5
    assert len(SW.covered_voxels(SW.shape(SW.SPHERE, (40.5, 50.5, 60.5), radius=0.0))) == 1
