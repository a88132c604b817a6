"""dust_amd/csrc/frame_plan.hpp, the device-free half of the frame path, run as native code on a CPU: tests/cpp/frame_plan_test.cpp
compiled with g++ under AddressSanitizer and UBSan (no HIP compiler, not linked against the library) reads launch-shaping inputs from a
file and writes the plans to another. They are held to a Python port of the frame path as it stood before the header existed:
dust_amd/csrc/capi.cpp of commit f3eae53, whose line numbers the port cites formula by formula (`:971` is line 971 of that file). The
port is written from that text, not from the header. uint32 arithmetic is masked where the C++ could wrap; the two share formulas are
evaluated in the precision the C++ used (noted at each)."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "frame_plan_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "frame_plan_test")

M32 = 0xFFFFFFFF
N16_LDS, MAX_CAND, REGIONS, MAX_BAND, MAX_BATCH, DEV_ENTER = 640, 160, 8, 65536, 8, 80   # dust_dev.h, kernels.hip: the program's last words pin them
RESERVE_AUTO, IN_FLIGHT_SHARE, IN_FLIGHT_ALL = 0xFFFFFFFF, 0, 1                          # include/dust_hip.h
PATH_AUTO, PATH_PACKETS, PATH_STREAMS = 0, 1, 2
PASS_FINAL_GATHER, PASS_SURFEL = 1 << 2, 1 << 3
SECTIONS = 14


@pytest.fixture(scope="module")
def exe():
    """built once, again when the program or a header it includes is newer (as tests/test_model_records.py caches its binary)"""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "dust_hip.h")] + [os.path.join(CSRC, h) for h in ("frame_plan.hpp", "dust_dev.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE])
    return EXE


def u64(v):
    return [int(v) & M32, int(v) >> 32]


def f32(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def run(exe, tmp_path, sections):
    """one run of the program (which must end clean under both sanitizers): {section: [case words, ...]} -> the output words, the constants checked"""
    head, body = [0] * SECTIONS, []
    for k in sorted(sections):
        head[k] = len(sections[k])
        for case in sections[k]:
            body.extend(case)
    (tmp_path / "in.bin").write_bytes(np.asarray(head + body, "<u4").tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    out = np.fromfile(tmp_path / "out.bin", "<u4")
    assert out[-4:].tolist() == [DEV_ENTER, MAX_BAND, MAX_BATCH, REGIONS]
    return out[:-4]


# ---------------------------------------------------------------------------------------------- slot plan and fused shape
SLOT_FIELDS = ("flags", "lds", "n_lds_boxes", "bpc", "resident", "reserve_blocks", "side_slots", "main_resident", "frame_slots", "grid", "fblock", "fgrid")
NO_LDS_BOXES, WIDE_FUSED, WIDE_SHARE = 1, 2, 4
AXES = ("cus", "max_lds", "block", "bpc", "models", "inst", "reserve", "share", "flight", "oversub", "tiles", "batch")


def slot_words(axes, flags):
    w = []
    for name in AXES:
        w.append(len(axes[name]))
        for v in axes[name]:
            w.extend(v if isinstance(v, tuple) else (v,))
    return w + [flags]


def slot_cases(axes):
    """the product the program walks, last axis fastest, as int64 columns"""
    idx = np.indices([len(axes[n]) for n in AXES]).reshape(len(AXES), -1)
    c = {}
    for k, name in enumerate(AXES):
        vals = np.asarray(axes[name], np.int64)
        col = vals[idx[k]]
        if name == "inst":
            c["inst"], c["groups"] = col[:, 0], col[:, 1]
        elif name == "reserve":
            c["reserve"], c["coll"] = col[:, 0], col[:, 1] != 0
        elif name == "share":
            c["busy"], c["share"] = col[:, 0] != 0, col[:, 1]
        elif name == "flight":
            c["fif"], c["mode"] = col[:, 0], col[:, 1]
        else:
            c[name] = col
    return c


def slot_port(c, flags):
    """capi.cpp:968-1045 (the plan) and :1107-1120 (the fused shape), over columns of cases"""
    W = np.where
    lds = c["models"] * N16_LDS + (c["block"] // 64) * (MAX_CAND * 8 + 8) + 16                          # :971 (size_t)
    too_big = lds > c["max_lds"]                                                                        # :972
    cull = W(c["groups"] != 0, c["groups"], c["inst"])                                                   # :975
    ride = ((lds + cull * 32) * c["bpc"] <= 160 * 1024) & (lds + cull * 32 <= c["max_lds"])             # :976
    if flags & NO_LDS_BOXES:
        ride = np.zeros_like(ride)
    n_lds_boxes = W(ride, cull, 0)                                                                      # :974, :977
    lds = W(ride, lds + cull * 32, lds)                                                                 # :978
    bpc = c["bpc"].copy()
    for _ in range(int(bpc.max())):                                                                     # :980 while (bpc > 1 && lds * bpc > 160 KB) --bpc
        bpc = W((bpc > 1) & (lds * bpc > 160 * 1024), bpc - 1, bpc)
    resident = (c["cus"] * bpc) & M32                                                                   # :985
    reserve = W(c["reserve"] == RESERVE_AUTO, W(c["coll"], 32, 0), c["reserve"]) & ~7 & M32              # :988
    resident = W((reserve != 0) & (((reserve + 8) & M32) <= resident), resident - reserve, resident)    # :989
    side = W(c["busy"], np.maximum(8, (((resident * c["share"]) & M32) // 100) & ~7), 0)                 # :1036
    main = np.maximum(8, (resident - np.minimum((resident - 8) & M32, side)) & M32)                     # :1037
    share_slots = (c["fif"] > 1) & (c["mode"] == IN_FLIGHT_SHARE)                                       # :1042
    per = ((((main // np.maximum(c["fif"], 1)) * (100 + c["oversub"])) & M32) // 100) & ~7              # :1044
    frame_slots = W(share_slots, np.minimum(main, np.maximum(8, per)), main)
    tiles8 = ((c["tiles"] + 7) & M32) // 8
    grid = np.maximum(8, np.minimum(frame_slots, tiles8))                                               # :1045
    batch_lds = (16 * (c["batch"] - 1)) & M32                                                           # :1108 (the Lead of n frames; 0 for a frame alone)
    f_too_big = lds + batch_lds > c["max_lds"]                                                          # :1109
    lds_wide = c["models"] * N16_LDS + 16 * (MAX_CAND * 8 + 8) + 16 + n_lds_boxes * 32 + batch_lds      # :1110
    alone = (c["block"] == 512) & (bpc == 2) & ~c["busy"] & (reserve == 0) & (lds_wide <= c["max_lds"])
    if not flags & WIDE_FUSED:
        alone = np.zeros_like(alone)
    wide1 = alone & ~share_slots & (grid == resident)                                                   # :1111-1112
    wide2 = ~wide1 & alone & share_slots & (c["fif"] == 2) & (grid == frame_slots) & (((frame_slots * 2) & M32) == resident)   # :1115-1116
    if not flags & WIDE_SHARE:
        wide2 = np.zeros_like(wide2)
    fblock = W(wide1 | wide2, 1024, c["block"])                                                         # :1107, :1113, :1118
    fgrid = W(wide1, np.maximum(8, np.minimum(c["cus"], tiles8)), W(wide2, np.maximum(8, (frame_slots // 2) & ~7), grid))   # :1114, :1119
    out = dict(flags=too_big * 1 + share_slots * 2 + (f_too_big & ~too_big) * 4, lds=lds, n_lds_boxes=n_lds_boxes, bpc=bpc, resident=resident,
               reserve_blocks=reserve, side_slots=side, main_resident=main, frame_slots=frame_slots, grid=grid, fblock=fblock, fgrid=fgrid)
    return out, dict(wide1=wide1, wide2=wide2, alone=alone, share_slots=share_slots)


def check_slots(exe, tmp_path, products):
    """products: [(axes, flags)] -> per product (cases, got); every output equal to the port's, and the properties on top"""
    got_all = run(exe, tmp_path, {0: [slot_words(a, f) for a, f in products]}).astype(np.int64)
    at, res = 0, []
    for axes, flags in products:
        c = slot_cases(axes)
        n = len(c["cus"])
        got = dict(zip(SLOT_FIELDS, got_all[at:at + n * len(SLOT_FIELDS)].reshape(n, -1).T))
        at += n * len(SLOT_FIELDS)
        want, why = slot_port(c, flags)
        fits = (want["flags"] & 1) == 0
        assert np.array_equal(got["flags"] & 1, want["flags"] & 1)
        for name in SLOT_FIELDS:   # (a plan that does not fit says only that; a fused shape that does not fit leaves the plan)
            mask = fits & ((want["flags"] & 4) == 0) if name in ("fblock", "fgrid") else fits
            bad = np.nonzero(mask & (got[name] != want[name]))[0]
            assert bad.size == 0, (name, {k: int(v[bad[0]]) for k, v in c.items()}, int(got[name][bad[0]]), int(want[name][bad[0]]))
        ok = fits & ((want["flags"] & 4) == 0)
        g = {k: v[ok] for k, v in got.items()}
        assert (g["grid"] >= 8).all() and (g["grid"] <= np.maximum(8, g["frame_slots"])).all()
        assert (g["reserve_blocks"] % 8 == 0).all() and (g["fgrid"] >= 8).all()
        # a wide shape: only with wide_fused, 512-thread workgroups two per CU, no surfel pass beside it, nothing reserved, and either the device to
        # itself or (WIDE_SHARE) two frames in flight on half of the slots each
        wide = g["fblock"] != c["block"][ok]
        assert (g["fblock"][wide] == 1024).all() and (not wide.any() or flags & WIDE_FUSED)
        assert (c["block"][ok][wide] == 512).all() and (g["bpc"][wide] == 2).all() and not c["busy"][ok][wide].any() and (g["reserve_blocks"][wide] == 0).all()
        shared = (g["flags"][wide] & 2) != 0
        assert (not shared.any() or flags & WIDE_SHARE) and (c["fif"][ok][wide][shared] == 2).all()
        assert (g["grid"][wide][~shared] == g["resident"][wide][~shared]).all()
        res.append((c, got, want))
    assert at == len(got_all)
    return res


FULL = dict(cus=[8, 64, 256], max_lds=[65280, 163584], block=[128, 512, 1024], bpc=[1, 2, 4], models=[0, 1, 255],
            inst=[(0, 0), (4, 0), (256, 0), (5000, 79)], reserve=[(RESERVE_AUTO, 1), (0, 0), (8, 0), (32, 0), (4096, 0)],
            share=[(0, 0), (1, 10), (1, 65)], flight=[(f, m) for f in (1, 2, 3) for m in (IN_FLIGHT_SHARE, IN_FLIGHT_ALL)],
            oversub=[0, 50, 100], tiles=[1, 7, 8, 9, 4050 * 8], batch=[1, 2, 8])


def test_slot_plan_and_fused_shape_are_the_port_over_the_full_grid(exe, tmp_path):
    """the issue's grid as a full product (2 624 400 cases), one product per (cus, max_lds, block) to keep the columns small"""
    products = [(dict(FULL, cus=[cu], max_lds=[ml], block=[b]), WIDE_FUSED) for cu in FULL["cus"] for ml in FULL["max_lds"] for b in FULL["block"]]
    res = check_slots(exe, tmp_path, products)
    assert sum(len(c["cus"]) for c, _, _ in res) == 2624400
    flags = np.concatenate([g["flags"] for _, g, _ in res])
    wide = np.concatenate([(g["fblock"] == 1024) & (c["block"] == 512) & ((g["flags"] & 5) == 0) for c, g, _ in res])
    assert np.count_nonzero(flags & 1) > 1000 and np.count_nonzero(wide) > 1000   # plans that do not fit, wide shapes


def test_slot_plan_under_every_flag(exe, tmp_path):
    """a thinner grid under each of NO_LDS_BOXES, NO_WIDE_FUSED and WIDE_SHARE; AUTO reserve outside a collective; a busy side stream at share 0"""
    thin = dict(FULL, cus=[256], max_lds=[163584], oversub=[0, 100], tiles=[9, 4050 * 8], batch=[1, 8],
                reserve=[(RESERVE_AUTO, 0), (RESERVE_AUTO, 1), (0, 0), (12, 0)], share=[(0, 0), (1, 0), (0, 65), (1, 65)])
    res = check_slots(exe, tmp_path, [(thin, f) for f in range(8)])
    for f, (c, got, _) in enumerate(res):
        ok = (got["flags"] & 5) == 0
        assert (f & NO_LDS_BOXES) == 0 or (got["n_lds_boxes"] == 0).all()
        two_wide = ok & (got["fblock"] != c["block"]) & ((got["flags"] & 2) != 0)
        assert two_wide.any() == (f & (WIDE_FUSED | WIDE_SHARE) == (WIDE_FUSED | WIDE_SHARE))
    c, got, _ = res[WIDE_FUSED]
    fits = (got["flags"] & 1) == 0
    assert (got["reserve_blocks"][fits & (c["reserve"] == 12)] == 8).all() and (got["side_slots"][fits & c["busy"] & (c["share"] == 0)] == 8).all()


def test_hand_worked_anchors(exe, tmp_path):
    """256 CUs, block 512, 2 per CU, one LDS model, 4 instances, no groups, 32 400 tiles, one frame in flight, nothing reserved, no side stream; then
    the same in a collective with the automatic reserve"""
    base = dict(cus=[256], max_lds=[163584], block=[512], bpc=[2], models=[1], inst=[(4, 0)], reserve=[(RESERVE_AUTO, 0), (RESERVE_AUTO, 1)], share=[(0, 0)],
                flight=[(1, IN_FLIGHT_SHARE)], oversub=[0], tiles=[32400], batch=[1])
    (_, got, _), = check_slots(exe, tmp_path, [(base, WIDE_FUSED)])
    assert 640 + 8 * 1288 + 16 + 128 == 11088
    assert [int(got[k][0]) for k in ("lds", "n_lds_boxes", "resident", "grid", "fblock", "fgrid")] == [11088, 4, 512, 512, 1024, 256]
    assert [int(got[k][1]) for k in ("lds", "n_lds_boxes", "resident", "reserve_blocks", "grid", "fblock", "fgrid")] == [11088, 4, 480, 32, 480, 512, 480]
    # a launch of several frames adds a 16-byte tile queue per further frame: 85 roots and the lists are 64 720 bytes, 100 below this limit
    tight = dict(base, max_lds=[64820], models=[85], inst=[(0, 0)], reserve=[(0, 0)], batch=[1, 2, 7, 8])
    (_, got, _), = check_slots(exe, tmp_path, [(tight, WIDE_FUSED)])
    assert got["lds"].tolist() == [64720] * 4 and got["flags"].tolist() == [0, 0, 0, 4] and got["fblock"].tolist()[:3] == [512, 512, 512]


# ---------------------------------------------------------------------------------------------- shares
def calibrated_port(P, Q, deep):
    """:1016-1017, in float (np.float32 at every step, as the C++ `float` expression rounds)"""
    f = np.float32
    P, Q = f(P), f(Q)
    k = f(1.05) if deep else f(1.4)
    return int(min(f(65.0), max(f(10.0), f(100.0) * Q / (Q + k * P) - f(3.0))))


def guessed_port(pool, width, rows):
    """:1032-1033, in double (Python floats)"""
    surfel, pixel = float(pool) * 18.0, 3.0 * float(width) * float(rows)
    return int(min(60.0, max(15.0, 100.0 * surfel / (surfel + pixel))))


def test_shares_are_the_port_and_clamp(exe, tmp_path):
    rng = np.random.default_rng(51)
    cal = [(P, Q, d) for d in (0, 1) for P, Q in [(1.0, 0.01), (1.0, 1e-6), (0.01, 1.0), (1e-6, 5.0), (0.23, 0.19), (0.9, 0.25), (4.2, 1.1)]]
    for d in (0, 1):   # the clamps' edges: Q / P at which 100 Q / (Q + k P) - 3 crosses 10, 11, 64 and 65, a hair to either side
        k = 1.05 if d else 1.4
        for edge in (10.0, 11.0, 64.0, 65.0):
            r = (edge + 3.0) / 100.0
            for eps in (-1e-4, -1e-6, 0.0, 1e-6, 1e-4):
                cal.append((1.0, k * r / (1.0 - r) * (1.0 + eps), d))
    cal += [(float(p), float(q), int(d)) for p, q, d in zip(rng.uniform(0.01, 5.0, 400), rng.uniform(0.01, 5.0, 400), rng.integers(0, 2, 400))]
    guess = [(345600, 1920, 1080), (345600, 3840, 2160), (345600, 64, 64), (1, 16384, 16384), (777, 64, 40), (0xFFFFFFFF, 1, 1), (345600, 1920, 1)]
    for edge in (15, 16, 59, 60):   # pool sizes at which the guess crosses the clamps' edges, for a 1080p frame
        pool = edge / (100.0 - edge) * 3.0 * 1920 * 1080 / 18.0
        guess += [(int(pool) + k, 1920, 1080) for k in (-1, 0, 1, 2)]
    guess += [tuple(int(v) for v in g) for g in zip(rng.integers(1, 1 << 22, 300), rng.integers(1, 16385, 300), rng.integers(1, 16385, 300))]
    out = run(exe, tmp_path, {1: [[f32(P), f32(Q), d] for P, Q, d in cal], 2: [list(g) for g in guess]}).tolist()
    want_cal, want_guess = [calibrated_port(*c) for c in cal], [guessed_port(*g) for g in guess]
    assert out == want_cal + want_guess
    assert min(want_cal) == 10 and max(want_cal) == 65 and {11, 63, 64} <= set(want_cal) and min(want_guess) == 15 and max(want_guess) == 60
    assert calibrated_port(0.23, 0.19, 0) != calibrated_port(0.23, 0.19, 1)
    assert (guessed_port(345600, 1920, 1080), guessed_port(345600, 3840, 2160)) == (50, 20)   # the castle at 1080p and at 4K


# ---------------------------------------------------------------------------------------------- stream layout
def layout_port(budget, bin_, dim, n_items, n_inst, no_lds):
    """:911-928"""
    at = 0

    def place(nbytes):
        nonlocal at
        nbytes = (nbytes + 15) & ~15
        if no_lds or at + nbytes > budget:
            return M32
        off = at & M32
        at += nbytes
        return off
    cells = place(dim[0] * dim[1] * dim[2] * 4) if bin_ else M32
    items = place(n_items * 2) if bin_ else M32
    boxes = place(n_inst * 32) if bin_ else M32
    enters = M32 if bin_ else place(n_inst * DEV_ENTER)
    return [boxes, cells, items, enters, at & M32]


def walk_budget_port(max_lds, n_lds_models):
    """:930 (the min keeps roots beyond max_lds from wrapping)"""
    return max_lds - min(max_lds, n_lds_models * N16_LDS)


def test_stream_layout_is_the_port(exe, tmp_path):
    a16 = lambda v: (v + 15) & ~15
    cases = []
    for dim, n_items, n_inst in [((8, 4, 8), 700, 300), ((3, 5, 7), 1, 1), ((16, 16, 16), 5000, 40), ((1, 1, 1), 0, 0), ((32, 16, 8), 4096, 1200)]:
        cells, items, boxes, enters = a16(dim[0] * dim[1] * dim[2] * 4), a16(n_items * 2), a16(n_inst * 32), a16(n_inst * DEV_ENTER)
        # budgets at which each of cells, items and boxes first stops fitting (a section that does not fit is skipped: the next may)
        budgets = {0, cells - 1, cells, cells + items - 1, cells + items, cells + items + boxes - 1, cells + items + boxes, items, boxes, 40 * 1024}
        cases += [(b, 1, dim, n_items, n_inst, no) for b in sorted(v for v in budgets if v >= 0) for no in (0, 1)]
        cases += [(b, 0, dim, n_items, n_inst, no) for b in (0, max(enters - 1, 0), enters, 163584) for no in (0, 1)]
    walks = [(ml, m) for ml in (65280, 163584) for m in (0, 1, 101, 102, 103, 255, 256)]
    assert any(m * N16_LDS > ml for ml, m in walks)
    cases += [(walk_budget_port(ml, m), 0, (8, 8, 8), 100, 300, 0) for ml, m in walks]   # the walk's budget as the frame asks for it
    out = run(exe, tmp_path, {3: [u64(b) + [bn, *dim, ni, nn, no] for b, bn, dim, ni, nn, no in cases], 4: [u64(ml) + [m] for ml, m in walks]})
    got = out[:len(cases) * 5].reshape(-1, 5).tolist()
    for c, g in zip(cases, got):
        assert g == layout_port(*c), (c, g)
    assert [int(lo) | int(hi) << 32 for lo, hi in out[len(cases) * 5:].reshape(-1, 2)] == [walk_budget_port(*w) for w in walks]
    assert walk_budget_port(65280, 103) == 0 and walk_budget_port(65280, 102) == 0 and walk_budget_port(65280, 101) == 640
    staged = np.asarray(got)[:, :4] != M32
    assert staged[:, 1].any() and (~staged[:, 1]).any() and (staged[:, 2] & ~staged[:, 1]).any() and (staged[:, 0] & ~staged[:, 2]).any() and staged[:, 3].any()
    assert not any(s.any() for c, s in zip(cases, staged) if c[5])   # NO_STREAM_LDS: nothing staged


# ---------------------------------------------------------------------------------------------- grids, paths, keys, runs, stride, shards
def test_grids_and_gi_paths_are_the_port(exe, tmp_path):
    rng = np.random.default_rng(52)
    grids = [(s, t, b, w, sh) for s in (0, 7, 8, 9, 480, 512, 1024) for t in (0, 1, 8, 9, 32400, 4095 * 64, M32) for b, w, sh in ((512, 2025, 50), (128, 0, 10), (1024, 675, 65))]
    grids += [tuple(int(v) for v in g) for g in zip(rng.integers(0, 2048, 200), rng.integers(0, 1 << 20, 200), rng.choice([128, 256, 512, 1024], 200),
                                                    rng.integers(0, 1 << 16, 200), rng.integers(0, 101, 200))]
    paths = list(itertools.product((0, PASS_FINAL_GATHER, PASS_SURFEL, PASS_FINAL_GATHER | PASS_SURFEL | 3), (0, 1), (PATH_AUTO, PATH_PACKETS, PATH_STREAMS), (0, 1),
                                   (0, 1, 4, 8, 16), (0, 1)))
    out = run(exe, tmp_path, {5: [list(g) for g in grids], 6: [list(p) for p in paths]}).tolist()

    def grids_port(slots, tiles, block, want, share):
        packet = max(8, min(slots, ((tiles + 7) & M32) // 8))                                           # :806, :1045, :1114, :1207, :1217
        walk = max(8, min((((slots * block) & M32) // 1024) & ~7, ((want + 7) & M32) & ~7))              # :818, :1199
        return [packet, walk, max(8, (((slots * share) & M32) // 100) & ~7)]                            # :1238

    def paths_port(passes, has_grid, path, deep, debug, no_gather_order):
        packet_gi, packet_only = path != PATH_STREAMS, path == PATH_PACKETS                             # :178-179
        fg = bool(passes & PASS_FINAL_GATHER) and bool(has_grid) and (not packet_gi or bool(deep and not packet_only and not debug & 12 and not no_gather_order))   # :963-964, :1183
        sf = bool(passes & PASS_SURFEL) and bool(has_grid) and not packet_gi                            # :965 (and :802, but for the sharded trace)
        return [int(fg), int(sf)]
    want = [v for g in grids for v in grids_port(*g)] + [v for p in paths for v in paths_port(*p)]
    assert out == want
    assert grids_port(512, 32400, 512, 2025, 50) == [512, 256, 256]


VIEW_KEY_BASIS = 1469598103934665603   # :1047, as written there: the published offset basis (14695981039346656037) less its last digit


def fnv1a(data, k=0xCBF29CE484222325):
    for b in data:
        k = ((k ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return k


def test_view_key_is_fnv1a_over_the_parents_bytes(exe, tmp_path):
    """:1046-1052: camera (60 bytes), the scene handle, its revision, the sky state (224 bytes), row_begin, row_end, mixed from the parent's own start
    value; the mixing function itself is pinned, independently of the port, by the published vectors of 64-bit FNV-1a from its published
    offset basis ("" -> cbf29ce484222325, "a" -> af63dc4c8601ec8c, "foobar" -> 85944171f73967e8)"""
    rng = np.random.default_rng(53)
    vectors = [(b"", 0xCBF29CE484222325), (b"a", 0xAF63DC4C8601EC8C), (b"foobar", 0x85944171F73967E8)]
    keys = []
    for _ in range(20):
        cam, sky = rng.integers(0, 1 << 32, 15, dtype=np.uint64), rng.integers(0, 1 << 32, 56, dtype=np.uint64)
        keys.append((cam.astype("<u4"), int(rng.integers(1, 1 << 62)), int(rng.integers(0, 1 << 40)), sky.astype("<u4"), int(rng.integers(0, 2000)), int(rng.integers(0, 2161))))
    keys.append((keys[0][0], keys[0][1], keys[0][2] + 1, keys[0][3], keys[0][4], keys[0][5]))   # the next revision of the same scene
    fnv = [[len(b)] + np.frombuffer(b + b"\0" * (-len(b) % 4), "<u4").tolist() for b, _ in vectors]
    out = run(exe, tmp_path, {7: [c.tolist() + u64(s) + u64(r) + k.tolist() + [rb, re] for c, s, r, k, rb, re in keys], 8: fnv})
    got = [int(lo) | int(hi) << 32 for lo, hi in out.reshape(-1, 2)]
    want = [fnv1a(c.tobytes() + struct.pack("<QQ", s, r) + k.tobytes() + struct.pack("<II", rb, re), VIEW_KEY_BASIS) for c, s, r, k, rb, re in keys]
    assert got == want + [v for _, v in vectors] and len(set(want)) == len(want)
    assert [fnv1a(b) for b, _ in vectors] == [v for _, v in vectors]


def test_view_runs_timing_stride_shards_and_key_bits(exe, tmp_path):
    runs = [(n, m) for n in range(1, MAX_BATCH + 1) for m in range(1 << n)] + [(0, 0)]
    timing = [(cs, b, n, c) for cs in (1, 4) for b in (0, 1) for n in (1, 2, 3, 4, 5, 8) for c in (0, 1, 2, 3, 4, 7, 8, M32)]
    shards = [(pool, r, w) for pool in (1, 63, 64, 65, 777, 4096, 345600) for w in (1, 2, 3, 7, 64) for r in sorted({0, 1, w // 2, w - 1})]
    caps = [1, 2, 3, 4, 5, 4093, 4096, 4097, 1 << 25, (1 << 25) - 1, (1 << 31) - 1, 1 << 31, M32]   # powers of two and not
    out = run(exe, tmp_path, {9: [list(r) for r in runs], 10: [list(t) for t in timing], 11: [list(s) for s in shards], 12: [[c] for c in caps]}).tolist()

    def runs_port(n, mask):
        """:1133-1139"""
        cont, run_of, i = [(mask >> k) & 1 for k in range(n)], [M32] * MAX_BATCH, 0
        while i < n:
            run = 1
            while i + run < n and cont[i + run]:
                run += 1
            run_of[i] = run
            for m in range(1, run):
                run_of[i + m] = 0
            i += run
        return run_of

    def timing_port(cs, batched, n, counter):
        stride = max(1, cs // n) if batched else cs                                                     # :996
        return [stride, int(counter % stride == 0)]                                                     # :998

    def shard_port(pool, rank, world):
        groups = ((pool + 63) & M32) // 64                                                              # :780
        per = ((groups + world - 1) & M32) // world
        begin = min(groups, (rank * per) & M32)                                                         # :796
        return [groups, per] + u64(((groups + 64) & M32) * 64) + [begin, min(per, groups - begin), (per * 64) & M32]   # :781, :797, :800

    def bits_port(capacity):
        bits = 1                                                                                        # :744-745
        while (1 << bits) <= capacity:
            bits += 1
        return bits
    want = [v for r in runs for v in runs_port(*r)] + [v for t in timing for v in timing_port(*t)] + [v for s in shards for v in shard_port(*s)] + [bits_port(c) for c in caps]
    assert out == want
    assert runs_port(5, 0b10110) == [3, 0, 0, 2, 0, M32, M32, M32]
    assert [bits_port(c) for c in (4093, 4096, 1 << 25, M32)] == [12, 13, 26, 32]
    assert shard_port(777, 3, 2)[4:6] == [13, 0] and shard_port(777, 1, 2)[4:] == [7, 6, 448]          # a rank past the end traces nothing


# ---------------------------------------------------------------------------------------------- tile schedule
NO_TILE_ORDER, EQUAL_BANDS, DILATE, FORCE_MOVING = 1, 2, 4, 8
ALLOCATE, RESET, BLEND, DO_DILATE, REUSE_CUTS, HAND_ORDER, HAND_CUTS, MEASURE = (1 << k for k in range(8))


class History:
    """DustHipPipeline::TileHistory without its buffers (:232-239)"""
    def __init__(self):
        self.tiles_x = self.tiles_y = self.capacity = self.age = 0
        self.refresh, self.view = 8, 0
        self.recorded = self.ordered = self.measured = self.moving = False
        self.cuts_age = 0

    def words(self):
        return [self.tiles_x, self.tiles_y, self.capacity, self.age, self.refresh] + u64(self.view) + \
               [self.recorded * 1 + self.ordered * 2 + self.measured * 4 + self.moving * 8, self.cuts_age]


def order_tiles_port(h, tx, ty, view, flags, cuts_reuse, moving_refresh, still_refresh_max):
    """order_tiles, :626-677: the decisions as the launches, memsets and pointers the parent made -> [decision bits, total, per_band]"""
    d = 0
    if flags & NO_TILE_ORDER:                                                                           # :628
        return [0, 0, 0]
    total = (tx * ty) & M32                                                                             # :630
    per_band = ((total + REGIONS - 1) & M32) // REGIONS                                                 # :631
    if per_band > MAX_BAND:                                                                             # :632
        return [0, total, per_band]
    if total > h.capacity:                                                                              # :633-638
        d |= ALLOCATE
        h.capacity, h.tiles_x, h.tiles_y = total, 0, 0
    if h.tiles_x != tx or h.tiles_y != ty:                                                              # :639-643
        d |= RESET
        h.recorded = h.ordered = h.measured = False
        h.tiles_x, h.tiles_y = tx, ty
    if h.recorded:                                                                                      # :644-653
        reuse = h.ordered and h.cuts_age + 1 < cuts_reuse and h.moving                                  # :646
        d |= BLEND | (REUSE_CUTS if reuse else 0)                                                       # :647, :650-651
        if h.moving and flags & DILATE and ty > 1:                                                      # :648-649
            d |= DO_DILATE
        h.cuts_age = h.cuts_age + 1 if reuse else 0                                                     # :652
        h.recorded, h.ordered, h.age = False, True, 0                                                   # :653
    elif h.ordered:                                                                                     # :654-656
        h.age += 1
    if h.ordered:                                                                                       # :657-660
        d |= HAND_ORDER | (0 if flags & EQUAL_BANDS else HAND_CUTS)
    still = h.ordered and h.view == view and not flags & FORCE_MOVING                                   # :661
    if not still:                                                                                       # :662
        h.refresh = 8
    jumped = not still and not h.moving                                                                 # :666
    period = min(h.refresh, still_refresh_max) if still else moving_refresh                             # :667
    if not h.ordered or jumped or h.age + 1 >= period:                                                  # :668-672
        d |= MEASURE
        h.recorded = h.measured = True
        if still:
            h.refresh = min(64, h.refresh * 2)
    h.moving = bool(not still and h.measured and h.view != 0 and (h.view != view or flags & FORCE_MOVING))   # :673
    h.view = view                                                                                       # :675
    return [d, total, per_band]


def schedule_sequences():
    """seeded sequences of launches: (first, tiles_x, tiles_y, view, flags, cuts_reuse, moving_refresh, still_refresh_max)"""
    rng = np.random.default_rng(54)
    grids = [(240, 135), (240, 135), (240, 68), (1, 1), (30, 1), (241, 136), (480, 270), (1024, 513)]   # a one-row grid, growth, a band beyond kTileOrderMaxBand
    seqs = []
    for s in range(16):
        flags = DILATE
        if s % 4 == 1:
            flags |= EQUAL_BANDS
        if s % 4 == 2:
            flags &= ~DILATE
        if s == 7:
            flags |= FORCE_MOVING
        tune = (int(rng.choice([1, 2, 4])), int(rng.choice([1, 2, 4, 6])), int(rng.choice([4, 16, 64, 100]))) if s >= 4 else (4, 4, 64)
        grid, view, mode, steps = grids[0], 1000 * (s + 1), "still", []
        for i in range(300):
            r = rng.random()
            if r < 0.03:
                mode = str(rng.choice(["still", "moving", "still", "moving", "zero"]))
            if r > 0.985:
                grid = grids[int(rng.integers(0, len(grids)))]
            if mode == "moving" or rng.random() < 0.02:   # (the second: a jump in a view that stands still)
                view = int(rng.integers(1, 1 << 63))
            f = flags
            if s >= 8 and rng.random() < 0.03:
                f ^= int(rng.choice([NO_TILE_ORDER, FORCE_MOVING, EQUAL_BANDS, DILATE]))
            steps.append((int(i == 0), grid[0], grid[1], 0 if mode == "zero" else view, f) + tune)
        seqs.append(steps)
    return seqs


def run_schedule(exe, tmp_path, steps):
    out = run(exe, tmp_path, {13: [[s[0], s[1], s[2]] + u64(s[3]) + list(s[4:]) for s in steps]})
    return out.reshape(len(steps), 12).tolist()


def test_tile_schedule_is_the_port_step_by_step(exe, tmp_path):
    steps = [s for seq in schedule_sequences() for s in seq]
    got = run_schedule(exe, tmp_path, steps)
    h, seen = None, 0
    for i, (s, g) in enumerate(zip(steps, got)):
        if s[0]:
            h = History()
        want = order_tiles_port(h, *s[1:]) + h.words()
        assert g == want, (i, s, g, want)
        seen |= g[0]
    assert seen == 255 and len(steps) == 4800
    assert any(g[1] > MAX_BAND * REGIONS and g[0] == 0 for g in got) and any(s[2] == 1 and g[0] & BLEND and not g[0] & DO_DILATE for s, g in zip(steps, got))


def test_tile_schedule_documented_behaviour(exe, tmp_path):
    """a still view's refresh doubles from 8 to at most 64; a jump is measured at once; a moving view re-measures every moving_refresh launches"""
    tune = (DILATE, 4, 4, 64)
    still = [(int(i == 0), 240, 135, 77) + tune for i in range(400)]
    jump = [(0, 240, 135, 78) + tune, (0, 240, 135, 78) + tune]
    moving = [(0, 240, 135, 100 + i) + tune for i in range(40)]
    got = run_schedule(exe, tmp_path, still + jump + moving)
    measured = [i for i in range(400) if got[i][0] & MEASURE]
    assert measured[0] == 0 and got[1][0] & BLEND and not got[1][0] & MEASURE   # the first launch measures, the second orders by it
    gaps = [b - a for a, b in zip(measured, measured[1:])]
    assert gaps[:4] == [8, 16, 32, 64] and set(gaps[4:]) == {64}, gaps
    refresh = [g[7] for g in got[:400]]
    assert sorted(set(refresh)) == [8, 16, 32, 64] and refresh == sorted(refresh)
    assert not got[399][0] & MEASURE and got[400][0] & MEASURE and got[400][7] == 8   # the jump: measured at once, the refresh back at 8
    assert got[401][0] & BLEND                                                       # ... and the launch after it re-orders
    mv = [g[0] for g in got[402:]]
    blends = [i for i, d in enumerate(mv) if d & BLEND]
    assert all(b - a == 4 for a, b in zip(blends[1:], blends[2:])) and len(blends) >= 8   # every moving_refresh launches
    assert any(d & REUSE_CUTS for d in mv) and any(d & BLEND and not d & REUSE_CUTS for d in mv[8:]) and any(d & DO_DILATE for d in mv)
