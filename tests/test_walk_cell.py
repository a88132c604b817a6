"""dust_amd/csrc/walk_cell.hpp, the cell arithmetic both conservative walks share, run as native code on a CPU: tests/cpp/walk_cell_test.cpp
compiled with g++ under AddressSanitizer and UBSan (-ffp-contract=off like the device build; no HIP compiler, not linked against the library)
reads cases from a file and writes every output of walk_enter, whole_cell_screen and cell_exit as raw 32-bit words. They are held, bit for
bit, to a numpy float32 port of the packet walk as it stood before the header existed: trace_instance in dust_amd/csrc/traverse.hpp of commit
7f50c05, whose line numbers the port cites (`:726` is line 726 of that file). The port is written from that text, not from the header. Every
array below is float32 or int32, so each numpy operation rounds once, as the C++ does without contraction; fminf / fmaxf are np.fmin / np.fmax
(both drop a NaN), rintf is np.rint (ties to even)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "walk_cell_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "walk_cell_test")

F, I = np.float32, np.int32
INF = F(np.inf)
POP = np.array([0, 1, 1, 2, 1, 2, 2, 3])
N = 120000   # random cases per function, beside the constructed ones


@pytest.fixture(scope="module")
def exe():
    """built once, again when the program or the header is newer (as tests/test_frame_plan.py caches its binary)"""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "walk_cell.hpp")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-ffp-contract=off",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to load first)
                               "-I", CSRC, SRC, "-o", EXE])
    return EXE


def words(*cols):
    """columns (float32 -> its bits, int32 / uint32 / bool -> the value) side by side, one row per case"""
    out = []
    for c in cols:
        c = np.asarray(c)
        c = c.reshape(len(c), -1)
        out.append(c.view(np.uint32) if c.dtype == np.float32 else c.astype(np.int64).astype(np.uint32))
    return np.concatenate(out, axis=1)


def run(exe, tmp_path, enter=None, screen=None, exit_=None):
    """one run of the program, which must end clean under both sanitizers: the three sections' output words"""
    secs = [np.zeros((0, w), np.uint32) if s is None else s for s, w in ((enter, 16), (screen, 16), (exit_, 15))]
    assert [s.shape[1] for s in secs] == [16, 16, 15]
    head = np.array([len(s) for s in secs], np.uint32)
    (tmp_path / "in.bin").write_bytes(np.concatenate([head] + [s.reshape(-1) for s in secs]).astype("<u4").tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    out = np.fromfile(tmp_path / "out.bin", "<u4")
    n = [len(s) for s in secs]
    assert len(out) == n[0] * 7 + n[1] + n[2] * 8
    return out[:n[0] * 7].reshape(-1, 7), out[n[0] * 7:n[0] * 7 + n[1]], out[n[0] * 7 + n[1]:].reshape(-1, 8)


# ---------------------------------------------------------------------------------------------- the port (traverse.hpp of 7f50c05)
def f2i_clamp(f, lo, hi):
    """:141-144  fminf(fmaxf(f, (float)lo), (float)hi), then (int): a NaN comes out as lo"""
    return np.fmin(np.fmax(f, lo.astype(F)), hi.astype(F)).astype(I)


def enter_port(o, d, bmin, bmax, te, tx, tmin, rt):
    """:711-746 -> t, ijk, near_tol, screen, tx_stop; and per axis whether the first cell's entry point is near its low / high brick plane,
    and whether a brick can lie beyond that plane (for the counts)"""
    with np.errstate(all="ignore"):
        t = np.fmax(te, F(0.0))                                                              # :711
        t = np.where(rt >= 2, np.fmax(t, tmin * (F(1.0) - F(1e-6))), t)                       # :712
        ijk = np.zeros((len(o), 3), I)
        reach = np.zeros(len(o), F)                                                           # :718
        blo, bhi = bmin.astype(I), bmax.astype(I) - 1
        for a in range(3):
            p = o[:, a] + d[:, a] * t                                                         # :725
            ijk[:, a] = f2i_clamp(np.where(d[:, a] < 0, np.ceil(p) - F(1.0), np.floor(p)), blo[:, a], bhi[:, a])   # :726
            reach = np.fmax(reach, np.abs(o[:, a]) + np.fmax(np.abs(p), np.abs(o[:, a] + d[:, a] * tx)))           # :727
        near_tol = F(3.0e-7) * (reach + F(16.0))                                              # :729
        screen = np.zeros(len(o), bool)
        near = np.zeros((len(o), 3, 2), bool)
        room = np.zeros((len(o), 3, 2), bool)
        for a in range(3):
            b0 = ijk[:, a] & ~3                                                               # :736
            q = (o[:, a] + d[:, a] * t) - b0.astype(F)                                        # :737
            near[:, a, 0], near[:, a, 1] = q <= F(4.0) * near_tol, q >= F(4.0) - F(4.0) * near_tol
            room[:, a, 0], room[:, a, 1] = b0 - 1 >= blo[:, a], b0 + 4 <= bhi[:, a]
            screen = screen | (near[:, a, 0] & room[:, a, 0]) | (near[:, a, 1] & room[:, a, 1])   # :738
        tx_stop = tx * (F(1.0) + F(1e-5)) + F(1e-5)                                           # :746
    return (t, ijk, near_tol, screen, tx_stop), near, room


def screen_port(o, d, t, ijk, stepped, near_tol, prev_whole, key, mask4):
    """:788-815 -> the new screen; and kd, bd, whether the shortcut of :810 was looked at (for building and counting cases)"""
    with np.errstate(all="ignore"):
        n = len(o)
        near16, sided = np.zeros(n, bool), np.ones(n, bool)                                   # :788
        near4 = np.zeros(n, np.int64)                                                         # :789
        c = ijk.astype(np.int64)                                                              # :790 (int64: the shifts of :811 cannot wrap here)
        for a in range(3):
            st = (stepped >> a) & 1 != 0                                                      # :793
            back = np.where(d[:, a] > 0, (ijk[:, a] & ~15) - 1, (ijk[:, a] & ~15) + 16)       # :794
            pa = o[:, a] + d[:, a] * t                                                        # :796
            r4 = pa * F(0.25)                                                                 # :797
            near = ~st & (np.abs(r4 - np.rint(r4)) <= near_tol)                               # :798
            near4 += near                                                                     # :799
            b0 = ijk[:, a] & ~3                                                               # :800
            q = pa - b0.astype(F)                                                             # :801
            lo = near & (q <= F(8.0) * near_tol)                                              # :803
            hi = near & ~lo & (q >= F(4.0) - F(8.0) * near_tol)                               # :804
            sided &= ~(near & ~lo & ~hi)                                                      # :805
            near16 |= (lo & ((b0 & 15) == 0)) | (hi & (((b0 + 4) & 15) == 0))
            c[:, a] = np.where(st, back, np.where(lo, b0 - 1, np.where(hi, b0 + 4, ijk[:, a])))
        pop = POP[stepped]
        across = ~((stepped == 0) | (near4 == 0))                                             # :809
        looked = across & (pop == 1) & (near4 == 1) & sided                                   # :810
        kd = (((c[:, 0] >> 4) << 16) | ((c[:, 1] >> 4) << 8) | (c[:, 2] >> 4)).astype(np.uint64).astype(np.uint32).view(I)   # :811 (the low 32 bits)
        bd = ((((c[:, 0] >> 2) & 3) << 4) | (((c[:, 1] >> 2) & 3) << 2) | ((c[:, 2] >> 2) & 3)).astype(np.uint64)               # :812
        bit = (mask4 >> bd) & np.uint64(1) != 0
        across &= ~(looked & (prev_whole | ((kd == key) & ~bit)))                             # :813
        return (pop > 1) | near16 | ~sided | across, kd, bd, looked                          # :815


def exit_port(o, d, inv, ijk, cl_main, extent, near_tol):
    """:818-850 -> tn, next_ijk, next_stepped, stuck, outside, next_screen"""
    with np.errstate(all="ignore"):
        n = len(o)
        S = (1 << cl_main).astype(I)                                                          # :818
        cc = ijk & ~(S - 1)[:, None]                                                          # :824
        plane = np.where(d > 0, cc + S[:, None], cc).astype(F)                                # :826
        ta = np.where(d != 0, (plane - o) * inv, INF).astype(F)                               # :825-830
        tn = np.full(n, INF, F)
        for a in range(3):
            tn = np.fmin(tn, ta[:, a])                                                        # :831
        stuck = ~(tn < INF)                                                                   # :833
        next_stepped, next_ijk = np.zeros(n, np.int64), np.zeros((n, 3), I)
        outside, next_screen = np.zeros(n, bool), np.zeros(n, bool)
        for a in range(3):
            tie = ta[:, a] == tn                                                              # :839
            next_stepped |= tie.astype(np.int64) << a                                         # :840
            across = np.where(d[:, a] > 0, cc[:, a] + S, cc[:, a] - 1)                        # :841
            outside |= tie & ((across < 0) | (across >= extent))                              # :842
            p = o[:, a] + d[:, a] * tn                                                        # :844
            inside = f2i_clamp(np.floor(p), cc[:, a], cc[:, a] + S - 1)                       # :845
            r = p * F(0.25)                                                                   # :846
            next_screen |= ~tie & (np.abs(r - np.rint(r)) <= near_tol)                        # :847
            next_ijk[:, a] = np.where(tie, across, inside)
        next_screen |= POP[next_stepped] > 1                                                  # :850
    return tn, next_ijk, next_stepped, stuck, outside, next_screen


# ---------------------------------------------------------------------------------------------- case material
TINY = np.array([1e-38, 1e-30, 1e-20, 1e-12, 1e-7], F)
NEAR_K = np.array([0.5, 0.9, 1.0, 1.1, 2.0, 3.9, 4.0, 4.1, 7.9, 8.0, 8.1, 16.0], F)   # offsets from a plane in units of near_tol: the code's own
                                                                                      # thresholds are 4 (:738, :798 on p / 4) and 8 (:803) of them


def directions(rng, n):
    """normal components; then per component a tenth exactly zero, some -0.0, a tenth +-tiny, and a few whole vectors along an axis"""
    d = rng.normal(size=(n, 3)).astype(F)
    k = rng.random((n, 3))
    d[k < 0.10] = F(0.0)
    d[(k >= 0.10) & (k < 0.12)] = F(-0.0)
    tiny = (k >= 0.12) & (k < 0.22)
    d[tiny] = TINY[rng.integers(0, len(TINY), int(tiny.sum()))] * rng.choice(np.array([-1, 1], F), int(tiny.sum()))
    return d


def tolerance(rng, o):
    """a visit's near_tol, :729, for a reach of the size the origin suggests"""
    reach = (np.abs(o).max(axis=1) * rng.uniform(1.0, 2.5, len(o))).astype(F)
    reach = np.where(np.isfinite(reach), reach, F(100.0)).astype(F)
    return F(3.0e-7) * (reach + F(16.0))


def near_lattice(rng, base, tol):
    """base (multiples of 4, float32) moved by 0 or by +-NEAR_K near_tol"""
    k = NEAR_K[rng.integers(0, len(NEAR_K), base.shape)] * rng.choice(np.array([-1, 0, 1], F), base.shape)
    return (base + k * (tol[:, None] if base.ndim == 2 else tol)).astype(F)


def count_directions(d):
    return dict(zero=int((d == 0).sum()), negative=int((d < 0).sum()), tiny=int(((d != 0) & (np.abs(d) <= F(1e-7))).sum()))


def count_lattice(p, tol):
    """how many coordinates lie exactly on a multiple of 4 / of 16, and how many within 1, 2 and 8 near_tol of one on either side"""
    p = p[np.isfinite(p).all(axis=1) & np.isfinite(tol)] if p.ndim == 2 else p
    tol = np.broadcast_to(tol[np.isfinite(tol)][:len(p), None], p.shape) if p.ndim == 2 else tol
    off4 = p.astype(np.float64) - np.rint(p.astype(np.float64) / 4.0) * 4.0
    got = dict(on4=int((off4 == 0).sum()), on16=int((np.mod(p, F(16.0)) == 0).sum()))
    for k in (1, 2, 8):
        got[f"below{k}"] = int(((off4 < 0) & (-off4 <= k * tol)).sum())
        got[f"above{k}"] = int(((off4 > 0) & (off4 <= k * tol)).sum())
    return got


# ---------------------------------------------------------------------------------------------- cell_exit
def exit_cases():
    rng = np.random.default_rng(61)
    parts = []

    def cells(n, faces=0.3):
        extent = rng.choice(np.array([256, 4096], I), n)
        cl = rng.choice(np.array([2, 4, 8, 12], I), n)
        cl = np.where((extent == 256) & (cl == 12), 8, cl).astype(I)   # (a 256^3 model has no 4096-cell: its largest is the model)
        ijk = (rng.random((n, 3)) * extent[:, None]).astype(I)
        face = rng.random((n, 3)) < faces                              # cells on the extent's faces
        ijk = np.where(face, np.where(rng.random((n, 3)) < 0.5, rng.integers(0, 4, (n, 3)), extent[:, None] - 1 - rng.integers(0, 4, (n, 3))), ijk).astype(I)
        return extent, cl, ijk

    # 1: a point inside the cell, the origin some way back along the ray
    n = N // 2
    extent, cl, ijk = cells(n)
    S = (1 << cl).astype(I)
    cc = ijk & ~(S - 1)[:, None]
    d = directions(rng, n)
    pt = (cc + rng.random((n, 3)) * S[:, None]).astype(F)
    back = np.where(rng.random(n) < 0.4, 0.0, rng.uniform(0.0, 60.0, n)).astype(F)
    o = (pt - d * back[:, None]).astype(F)
    parts.append((o, d, ijk, cl, extent, tolerance(rng, o)))
    # 2: origins on and beside the lattice; with a zero or tiny component the next cell's entry point stays there
    n = N // 4
    extent, cl, ijk = cells(n)
    d = directions(rng, n)
    still = rng.random((n, 3)) < 0.5
    d[still] = np.where(rng.random(int(still.sum())) < 0.5, F(0.0), TINY[rng.integers(0, len(TINY), int(still.sum()))])
    base = (((ijk >> 2) + rng.integers(0, 2, (n, 3))) * 4).astype(F)
    base = np.where(rng.random((n, 3)) < 0.4, ((ijk >> 4) + rng.integers(0, 2, (n, 3))) * 16, base).astype(F)
    tol = tolerance(rng, base)
    o = near_lattice(rng, base, tol)
    parts.append((o, d, ijk, cl, extent, tol))
    # 3: exact ties: integer origins inside the cell, components of +-1, the same whole distance to the exit plane on two or on three axes
    # (diagonals through lattice corners); the third axis ties too, stands still, or runs at another speed
    n = N // 4
    extent, cl, ijk = cells(n, faces=0.5)
    S = (1 << cl).astype(I)
    cc = ijk & ~(S - 1)[:, None]
    sign = rng.choice(np.array([-1, 1], I), (n, 3))
    dist = np.repeat(rng.integers(1, S + 1)[:, None], 3, axis=1)
    third = rng.integers(0, 3, n)
    kind = rng.integers(0, 3, n)                                        # 0: three axes tie, 1: the third stands still, 2: it has its own speed
    rows = np.arange(n)
    dist[rows, third] = np.where(kind == 0, dist[rows, third], rng.integers(1, S + 1))
    o = np.where(sign > 0, cc + S[:, None] - dist, cc + dist).astype(F)
    d = sign.astype(F)
    d[rows, third] = np.where(kind == 0, d[rows, third], np.where(kind == 1, F(0.0), rng.normal(size=n).astype(F)))
    ijk = np.where(sign > 0, cc + S[:, None] - dist, cc + dist - 1).astype(I)   # the cell the point is moving into
    ijk = np.clip(ijk, cc, cc + S[:, None] - 1).astype(I)
    parts.append((o, d, ijk, cl, extent, tolerance(rng, o)))
    # 4: NaN and infinite coordinates (f2i_clamp turns a NaN into the cell's low corner), rays that stand still
    n = 6000
    extent, cl, ijk = cells(n)
    d = directions(rng, n)
    o = (ijk + rng.random((n, 3))).astype(F)
    bad = rng.integers(0, 4, n)
    rows, ax = np.arange(n), rng.integers(0, 3, n)
    o[rows[bad == 0], ax[bad == 0]] = F(np.nan)
    d[rows[bad == 1], ax[bad == 1]] = F(np.nan)
    o[rows[bad == 2], ax[bad == 2]] = rng.choice(np.array([np.inf, -np.inf], F), int((bad == 2).sum()))
    d[bad == 3] = F(0.0)
    parts.append((o, d, ijk, cl, extent, tolerance(rng, o)))
    o, d, ijk, cl, extent, tol = (np.concatenate([p[k] for p in parts]) for k in range(6))
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d).astype(F)   # (1 / d in IEEE float32, as the walks divide)
    return o, d, inv, ijk, cl, extent, tol


def test_cell_exit_is_the_parents_step_bit_for_bit(exe, tmp_path):
    o, d, inv, ijk, cl, extent, tol = exit_cases()
    assert len(o) >= 100000
    _, _, got = run(exe, tmp_path, exit_=words(o, d, inv, ijk, cl, extent, tol))
    tn, nijk, nst, stuck, outside, nscreen = exit_port(o, d, inv, ijk, cl, extent, tol)
    want = words(tn, nijk, nst, stuck, outside, nscreen)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (len(bad), o[bad[0]], d[bad[0]], ijk[bad[0]], cl[bad[0]], extent[bad[0]], tol[bad[0]], got[bad[0]], want[bad[0]])
    # the kinds of case the comparison must have seen
    dirs = count_directions(d)
    assert min(dirs.values()) > 5000, dirs
    lat = count_lattice(o, tol)
    assert min(lat.values()) > 300, lat
    with np.errstate(all="ignore"):
        p = o + d * tn[:, None]                      # the next cell's entry point, where it exists
    stay = np.isfinite(p).all(axis=1) & (POP[nst] < 3)
    lat_p = count_lattice(p[stay], tol[stay])
    assert min(lat_p.values()) > 300, lat_p
    ties = np.bincount(POP[nst], minlength=4)
    assert ties[2] > 5000 and ties[3] > 5000 and ties[1] > 50000, ties
    for e in (256, 4096):
        for c in (2, 4, 8, 12):
            sel = (extent == e) & (cl == c)
            whole = (1 << c) >= e   # (the cell is the model: every step leaves it)
            assert (c == 12 and e == 256) or (sel.sum() > 5000 and outside[sel].sum() > 100 and (whole or (~outside[sel]).sum() > 100)), (e, c)
    assert ((nijk < 0).any(axis=1) & outside).sum() > 1000 and ((nijk >= extent[:, None]).any(axis=1) & outside).sum() > 1000
    assert nscreen.sum() > 5000 and (~nscreen).sum() > 5000 and (nscreen & (POP[nst] == 1)).sum() > 1000
    assert stuck.sum() > 1000 and np.isnan(o).any(axis=1).sum() > 1000 and np.isnan(d).any(axis=1).sum() > 1000


# ---------------------------------------------------------------------------------------------- whole_cell_screen
def screen_cases():
    rng = np.random.default_rng(62)
    n = N + 40000
    ijk = rng.integers(16, 4080, (n, 3)).astype(I)
    low = rng.random((n, 3)) < 0.05
    ijk = np.where(low, rng.integers(0, 4, (n, 3)), ijk).astype(I)     # (cells beside plane 0: the neighbour's coordinate is -1)
    stepped = (np.arange(n) % 8).astype(I)
    d = directions(rng, n)
    tol = tolerance(rng, ijk.astype(F))
    # the entry point: on a stepped axis the face of the 16-cell the ray came in through; on the others a brick plane of the cell or
    # a point inside it, beside the plane by 0 or a few near_tol, on the cell's own side of it or (the walk's integer cell and the point
    # may disagree) the other
    st = (stepped[:, None] >> np.arange(3)) & 1 != 0
    face = np.where(d > 0, ijk & ~15, (ijk & ~15) + 16).astype(F)
    plane = (((ijk >> 2) + rng.choice(np.array([-1, 0, 0, 0, 1, 1, 1, 2]), (n, 3))) * 4).astype(F)   # (-1, 2: a plane the cell's brick does not touch; `sided` of :805
    # stays true even so: a point within near_tol of a multiple of 4 is at most 8 near_tol above b0 or at least 4 - 8 near_tol above it)
    inside = (ijk + rng.random((n, 3))).astype(F)
    beside = rng.random((n, 3)) < 0.6
    p = np.where(st, face, np.where(beside, near_lattice(rng, plane, tol), inside)).astype(F)
    t = np.where(rng.random(n) < 0.4, 0.0, rng.uniform(0.0, 80.0, n)).astype(F)
    o = (p - d * t[:, None]).astype(F)
    nan = rng.random(n) < 0.01
    o[nan, rng.integers(0, 3, int(nan.sum()))] = F(np.nan)
    prev_whole = rng.random(n) < 0.3
    # the cache: the key :811 works out for this case (from the port) or another; its mask with the looked-up bit set or clear
    zero = np.zeros(n, np.uint64)
    _, kd, bd, _ = screen_port(o, d, t, ijk, stepped, tol, prev_whole, np.zeros(n, I), zero)
    match = rng.random(n) < 0.6
    key = np.where(match, kd, np.where(rng.random(n) < 0.3, -1, rng.integers(0, 1 << 24, n))).astype(I)
    mask4 = rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
    setbit = rng.random(n) < 0.5
    one = np.uint64(1) << bd
    mask4 = np.where(setbit, mask4 | one, mask4 & ~one)
    return o, d, t, ijk, stepped, tol, prev_whole, key, mask4


def test_whole_cell_screen_is_the_parents_refinement_bit_for_bit(exe, tmp_path):
    o, d, t, ijk, stepped, tol, prev_whole, key, mask4 = screen_cases()
    assert len(o) >= 100000
    lo, hi = (mask4 & np.uint64(0xFFFFFFFF)).astype(np.uint32), (mask4 >> np.uint64(32)).astype(np.uint32)
    _, got, _ = run(exe, tmp_path, screen=words(o, d, t, ijk, stepped, tol, prev_whole, key, lo, hi))
    want, kd, bd, looked = screen_port(o, d, t, ijk, stepped, tol, prev_whole, key, mask4)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (len(bad), o[bad[0]], d[bad[0]], t[bad[0]], ijk[bad[0]], stepped[bad[0]], tol[bad[0]], prev_whole[bad[0]], key[bad[0]], hex(mask4[bad[0]]))
    assert set(got.tolist()) == {0, 1}
    for m in range(8):
        assert want[stepped == m].sum() > 100 and (m == 0 or m in (3, 5, 6, 7) or (~want[stepped == m]).sum() > 100), m   # (two stepped axes: always raised)
    assert (~want[stepped == 0]).sum() > 100
    bit = (mask4 >> bd) & np.uint64(1) != 0
    at_key = looked & ~prev_whole
    tally = {(bool(pw), bool(m), bool(b)): int((looked & (prev_whole == pw) & ((kd == key) == m) & (bit == b)).sum())
             for pw in (False, True) for m in (False, True) for b in (False, True)}
    assert min(tally.values()) > 100, tally
    assert (at_key & (kd == key) & ~bit & ~want).sum() > 100 and (at_key & (kd == key) & bit & want).sum() > 100 and (at_key & (kd != key) & want).sum() > 100
    assert (looked & prev_whole & ~want).sum() > 100 and (looked & (kd < 0)).sum() > 10   # kd < 0: a neighbour beside plane 0
    dirs = count_directions(d)
    assert min(dirs.values()) > 5000, dirs
    with np.errstate(all="ignore"):
        p = o + d * t[:, None]
    lat = count_lattice(p[np.isfinite(p).all(axis=1)], tol[np.isfinite(p).all(axis=1)])
    assert min(lat.values()) > 300, lat
    assert np.isnan(o).any(axis=1).sum() > 500


# ---------------------------------------------------------------------------------------------- walk_enter
def slab(o, d, bmin, bmax):
    """where a ray meets a box, in float32 (any te / tx will do for the comparison: these make the cases the walk meets)"""
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
        t1, t2 = (bmin - o) * inv, (bmax - o) * inv
        lo, hi = np.where(d != 0, np.fmin(t1, t2), -INF), np.where(d != 0, np.fmax(t1, t2), INF)
        return lo.max(axis=1).astype(F), hi.min(axis=1).astype(F)


def enter_cases():
    rng = np.random.default_rng(63)
    parts = []

    def bounds(n):
        extent = rng.choice(np.array([256, 4096], I), n)
        lo = (rng.integers(0, extent[:, None] // 4 - 2, (n, 3)) * 4)
        hi = lo + 4 * rng.integers(1, np.maximum(2, (extent[:, None] - lo) // 4 + 1), (n, 3))
        return lo.astype(F), np.minimum(hi, extent[:, None]).astype(F)

    # 1: from outside, towards a point of the bounds: the walk starts on a face of the bounds, where no brick lies beyond
    n = N // 2
    bmin, bmax = bounds(n)
    target = (bmin + rng.random((n, 3)) * (bmax - bmin)).astype(F)
    d = directions(rng, n)
    o = (target - d * rng.uniform(1.0, 3000.0, n).astype(F)[:, None]).astype(F)
    parts.append((o, d, bmin, bmax))
    # 2: from inside, origins on and beside brick planes (multiples of 4 and of 16), faces of the bounds among them
    n = N // 2
    bmin, bmax = bounds(n)
    d = directions(rng, n)
    cells4 = ((bmax - bmin) / 4).astype(I)
    base = bmin + 4 * (rng.random((n, 3)) * (cells4 + 1)).astype(I)
    onface = rng.random((n, 3)) < 0.3
    base = np.where(onface, np.where(rng.random((n, 3)) < 0.5, bmin, bmax), base).astype(F)
    base = np.where(rng.random((n, 3)) < 0.3, np.clip(np.rint(base / 16) * 16, bmin, bmax), base).astype(F)
    tol = tolerance(rng, base)
    o = np.where(rng.random((n, 3)) < 0.7, near_lattice(rng, base, tol), (bmin + rng.random((n, 3)) * (bmax - bmin))).astype(F)
    parts.append((o, d, bmin, bmax))
    # 3: NaN coordinates
    n = 4000
    bmin, bmax = bounds(n)
    d = directions(rng, n)
    o = (bmin + rng.random((n, 3)) * (bmax - bmin)).astype(F)
    o[np.arange(n), rng.integers(0, 3, n)] = F(np.nan)
    parts.append((o, d, bmin, bmax))
    o, d, bmin, bmax = (np.concatenate([p[k] for p in parts]) for k in range(4))
    te, tx = slab(o, d, bmin, bmax)
    n = len(o)
    rt = (np.arange(n) % 4).astype(I)
    with np.errstate(all="ignore"):
        span = np.where(np.isfinite(te) & np.isfinite(tx), np.abs(te) + np.abs(tx - te), F(10.0)).astype(F)
        tmin = np.where(rng.random(n) < 0.3, F(0.0), (te + span * rng.uniform(-1.0, 1.0, n).astype(F))).astype(F)   # in front of te and behind it
    return o, d, bmin, bmax, te, tx, tmin, rt


def test_walk_enter_is_the_parents_prologue_bit_for_bit(exe, tmp_path):
    o, d, bmin, bmax, te, tx, tmin, rt = enter_cases()
    assert len(o) >= 100000
    got, _, _ = run(exe, tmp_path, enter=words(o, d, bmin, bmax, te, tx, tmin, rt))
    (t, ijk, tol, screen, tx_stop), near, room = enter_port(o, d, bmin, bmax, te, tx, tmin, rt)
    want = words(t, ijk, tol, screen, tx_stop)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (len(bad), o[bad[0]], d[bad[0]], bmin[bad[0]], bmax[bad[0]], te[bad[0]], tx[bad[0]], tmin[bad[0]], rt[bad[0]], got[bad[0]], want[bad[0]])
    for r in range(4):
        sel = rt == r
        front, behind = sel & (tmin < te) & (te > 0), sel & (tmin > te) & (tmin > 0)
        assert front.sum() > 3000 and behind.sum() > 3000, r
        clamped = behind & (t > np.fmax(te, F(0.0)))
        assert (clamped.sum() > 3000) == (r >= 2) and (r >= 2 or clamped.sum() == 0), r    # only the GI ray types start at tmin
        assert screen[sel].sum() > 1000 and (~screen[sel]).sum() > 1000, r
    # a near plane with and without room for a brick beyond it, low and high
    for side in (0, 1):
        assert (near[:, :, side] & room[:, :, side]).sum() > 3000 and (near[:, :, side] & ~room[:, :, side]).sum() > 3000, side
    outside_start = (te > 0) & np.isfinite(te) & (te <= tx)
    assert outside_start.sum() > 30000 and (outside_start & ~screen).sum() > 20000   # a start on the bounds is rarely worth a call
    dirs = count_directions(d)
    assert min(dirs.values()) > 5000, dirs
    inside = (te <= 0) & np.isfinite(o).all(axis=1)
    lat = count_lattice(o[inside], tol[inside])
    assert min(lat.values()) > 300, lat
    assert np.isnan(o).any(axis=1).sum() >= 4000
    assert (ijk >= bmin.astype(I)).all() and (ijk <= bmax.astype(I) - 1).all()       # NaN or not, the first cell lies inside the bounds


# ---------------------------------------------------------------------------------------------- anchors
def bits(*v):
    return np.asarray(v, F).view(np.uint32).tolist()


def test_hand_worked_anchors(exe, tmp_path):
    """cases small enough to work by hand, with the expected words written out"""
    f3 = lambda *v: np.asarray([v], F)
    i3 = lambda *v: np.asarray([v], I)
    one = lambda v, dt=I: np.asarray([v], dt)
    inf = float("inf")
    exits = [
        # from (1,1,1) along (1,1,1) in the 4-cell at 0: every plane is 3 away: a three-axis tie into (4,4,4), which raises the screen
        (words(f3(1, 1, 1), f3(1, 1, 1), f3(1, 1, 1), i3(1, 1, 1), one(2), one(256), one(1e-5, F)), [0x40400000, 4, 4, 4, 7, 0, 0, 1]),
        # along +x only: x = 4 is 3.5 away; y = 1.5 and z = 2.5 are 0.375 of a brick from the nearest plane: no screen
        (words(f3(0.5, 1.5, 2.5), f3(1, 0, 0), f3(1, inf, inf), i3(0, 1, 2), one(2), one(256), one(1e-5, F)), [0x40600000, 4, 1, 2, 1, 0, 0, 0]),
        # the same in the last 4-cell of a 256^3 model: x = 256 is 1.5 away and outside the extent
        (words(f3(254.5, 1.5, 2.5), f3(1, 0, 0), f3(1, inf, inf), i3(254, 1, 2), one(2), one(256), one(1e-5, F)), [0x3FC00000, 256, 1, 2, 1, 0, 1, 0]),
        # -x out of the 16-cell at 16, y exactly on the brick plane 20: 2.5 away, into x = 15, and the screen is raised
        (words(f3(18.5, 20, 41.5), f3(-1, 0, 0), f3(-1, inf, inf), i3(18, 20, 41), one(4), one(4096), one(1e-5, F)), [0x40200000, 15, 20, 41, 1, 0, 0, 1]),
        # a ray that stands still: no plane is ever reached, tn stays infinite, and all three infinite exit times "tie" with it: stuck
        (words(f3(5.5, 6.5, 7.5), f3(0, 0, 0), f3(inf, inf, inf), i3(5, 6, 7), one(2), one(256), one(1e-5, F)), [0x7F800000, 3, 3, 3, 7, 1, 0, 1]),
    ]
    # whole_cell_screen: entered through x = 32 going +x, y exactly on the brick plane 20, z mid-brick: the brick to look for is across both, at
    # (31, 19, 40): 16-cell (1, 1, 2) -> key 0x010102, 4-cell (3, 0, 2) of it -> bit 50
    def scr(prev_whole, key, mask4, stepped=1, x=32.0, y=20.0):
        return words(f3(x, y, 42.5), f3(1, 0, 0), one(0, F), i3(32, 20, 40), one(stepped), one(1e-5, F), one(prev_whole), one(key), one(mask4 & 0xFFFFFFFF, np.uint32), one(mask4 >> 32, np.uint32))
    screens = [(scr(0, 0x010102, 0), [0]), (scr(0, 0x010102, 1 << 50), [1]), (scr(0, 0x010102, ~(1 << 50) & (2 ** 64 - 1)), [0]), (scr(0, 0x010103, 0), [1]),
               (scr(1, 0x010103, 2 ** 64 - 1), [0]),
               (scr(0, 0x010102, 0, stepped=3), [1]),      # two stepped axes: a tie, always raised
               (scr(0, 0x010102, 0, stepped=0, x=33.5), [0]),   # no face entered (x mid-brick): nothing lies across one
               (scr(0, 0x010102, 0, stepped=0), [1]),      # ... but x on the 16-cell's own face 32 has neighbours outside the cell
               (scr(0, 0x010102, 0, y=21.5), [0])]         # y mid-brick: near no plane
    # walk_enter: from x = -10 along +x into bounds [0, 64)^3: t = te = 10, first cell (0, 5, 6); reach = 10 + |-10 + 74| = 74, near_tol = 3e-7f * 90;
    # the start is on plane 0 with nothing beyond: no screen; tx_stop = 74 * (1 + 1e-5f) + 1e-5f. From x = 8 inside: t = 0, on plane 8 with bricks beyond
    tol90 = F(3.0e-7) * F(90.0)
    stop74 = F(74.0) * (F(1.0) + F(1e-5)) + F(1e-5)
    enters = [
        (words(f3(-10, 5.5, 6.5), f3(1, 0, 0), f3(0, 0, 0), f3(64, 64, 64), one(10, F), one(74, F), one(0, F), one(0)), [0x41200000, 0, 5, 6, bits(tol90)[0], 0, bits(stop74)[0]]),
        (words(f3(8, 5.5, 6.5), f3(1, 0, 0), f3(0, 0, 0), f3(64, 64, 64), one(-8, F), one(56, F), one(0, F), one(0)),
         [0, 8, 5, 6, bits(F(3.0e-7) * (F(8.0) + F(64.0) + F(16.0)))[0], 1, bits(F(56.0) * (F(1.0) + F(1e-5)) + F(1e-5))[0]]),
        # a surfel ray (type 2) starts at tmin * (1 - 1e-6f) = 0x41BFFFF3 when that lies behind te; a camera ray (type 0) does not
        (words(f3(-10, 5.5, 6.5), f3(1, 0, 0), f3(0, 0, 0), f3(64, 64, 64), one(10, F), one(74, F), one(24, F), one(2)), [0x41BFFFF3, 13, 5, 6, bits(tol90)[0], 0, bits(stop74)[0]]),
        (words(f3(-10, 5.5, 6.5), f3(1, 0, 0), f3(0, 0, 0), f3(64, 64, 64), one(10, F), one(74, F), one(24, F), one(0)), [0x41200000, 0, 5, 6, bits(tol90)[0], 0, bits(stop74)[0]]),
    ]
    assert bits(tol90, stop74) == [0x37E27E10, 0x42940062]   # 2.7e-5; 74.00075 = 74 + 98 ulps of 2^-17
    e, s, x = run(exe, tmp_path, enter=np.concatenate([c for c, _ in enters]), screen=np.concatenate([c for c, _ in screens]), exit_=np.concatenate([c for c, _ in exits]))
    assert e.tolist() == [w for _, w in enters]
    assert s.tolist() == [w[0] for _, w in screens]
    assert x.tolist() == [w for _, w in exits]
