"""tests/resample_witness.py held to itself: the whole-array int64 formulation against a pure-Python loop over single voxels, on boxes
of at most 12^3 -- all five ops, negative Q, m and t at their limits, a palette map, the order of a call's records, the snapshot rule
and the dry run -- and its range function against the brute-force minimum and maximum. No device, no library."""
import numpy as np
import pytest

import resample_witness as R


def small_grids(seed):
    rng = np.random.default_rng(seed)
    src = np.zeros((256,) * 3, np.uint8)
    dst = np.zeros((256,) * 3, np.uint8)
    src[0:24, 0:24, 0:24] = np.where(rng.random((24,) * 3) < 0.6, rng.integers(1, 256, (24,) * 3), 0)
    dst[0:24, 0:24, 0:24] = np.where(rng.random((24,) * 3) < 0.5, rng.integers(1, 256, (24,) * 3), 0)
    src[250:256, 250:256, 250:256] = rng.integers(1, 256, (6, 6, 6))
    dst[250:256, 250:256, 250:256] = np.where(rng.random((6, 6, 6)) < 0.5, rng.integers(1, 256, (6, 6, 6)), 0)
    return src, dst


def fixed(v):
    return int(round(v * R.ONE))


def general_records():
    c, s = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    rot = [[fixed(c), fixed(s), 0], [fixed(-s), fixed(c), 0], [0, 0, R.ONE]]
    shear = [[R.ONE, fixed(0.5), 0], [0, R.ONE, fixed(-0.25)], [0, 0, R.ONE]]
    half = [[R.ONE // 2, 0, 0], [0, R.ONE // 2, 0], [0, 0, R.ONE // 2]]
    mirror = [[0, -R.ONE, 0], [-R.ONE, 0, 0], [0, 0, fixed(1.5)]]
    out = []
    for k, (m, t) in enumerate(((rot, (fixed(-2.3), fixed(4.1), 0)), (shear, (fixed(-0.25), 0, fixed(1.75))), (half, (fixed(3.0), fixed(-0.25), 0)),
                                (mirror, (fixed(20.0), fixed(21.5), fixed(-1.0))))):
        for op in range(5):
            lo = (k, 1, 2)
            out.append(R.records([m], [t], lo, tuple(v + 11 for v in lo), op, (2, 3, 1), (20, 18, 22))[0])
    return out


def test_whole_array_formulation_against_the_per_voxel_loop():
    src, dst = small_grids(1)
    rng = np.random.default_rng(2)
    palette_map = rng.permutation(255).astype(np.uint8)
    covered = negative = 0
    for i, rec in enumerate(general_records()):
        pm = palette_map if i % 3 == 0 else None
        a, b = dst.copy(), dst.copy()
        got = R.resample_one(a, src, rec, pm)
        want = R.loop_one(b, src, rec, pm)
        assert got == want and np.array_equal(a, b), i
        s = R.source_of(rec, *R.clipped_box(rec))
        negative += int(sum(np.count_nonzero(v < 0) for v in s))
        covered += got[1]
        assert got[0] <= got[1] and got[3] <= got[2] <= got[1]
    assert covered > 2000 and negative > 500        # images, and Q below zero beside them


def test_the_floor_rounds_toward_minus_infinity():
    src = np.zeros((256,) * 3, np.uint8)
    src[0:4, 0:4, 0:4] = 9
    dst = np.zeros((256,) * 3, np.uint8)
    # destination voxel x reads source position x + 0.5 - 0.75: voxel 0 lands at -0.25 -> s = -1, outside; a truncating shift reads 0
    rec = R.records([np.eye(3, dtype=np.int64) * R.ONE], [(fixed(-0.75), 0, 0)], (0, 0, 0), (5, 3, 3), R.REPLACE, (0, 0, 0), (3, 3, 3))[0]
    s = R.source_of(rec, [0, 0, 0], [5, 3, 3])
    assert s[0][:, 0, 0].tolist() == [-1, 0, 1, 2, 3, 4]
    out, counts = R.resample(dst, src, [rec])
    assert out[0, 0, 0] == 0 and out[1:5, 0:4, 0:4].all() and out[5, 0, 0] == 0 and counts["covered"][0] == 4 * 16
    q = R.box_range(rec, [0, 0, 0], [0, 0, 0])[0]
    assert q == (-32768, -32768) and q[0] // 131072 == -1 and int(q[0] / 131072) == 0


@pytest.mark.parametrize("sign_m, sign_t", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_limits_stay_inside_32_bits_and_agree_with_the_loop(sign_m, sign_t):
    src, dst = small_grids(3)
    m = np.full((3, 3), sign_m * R.MAX_M, np.int64)
    t = [sign_t * R.MAX_T] * 3
    for lo, hi in (((0, 0, 0), (5, 5, 5)), ((250, 250, 250), (255, 255, 255))):
        rec = R.records([m], [t], lo, hi, R.OVERWRITE)[0]
        assert not R.refused(rec)
        a, b = dst.copy(), dst.copy()
        assert R.resample_one(a, src, rec) == R.loop_one(b, src, rec) and np.array_equal(a, b)
        for k, (least, most) in enumerate(R.box_range(rec, list(lo), list(hi))):
            assert -(1 << 31) < least <= most < 1 << 31
    # (these cover nothing inside the tree; the next test has an image.) One step beyond either limit is refused
    for field, value in (("m", R.MAX_M + 1), ("m", -R.MAX_M - 1), ("t", R.MAX_T + 1), ("t", -R.MAX_T - 1)):
        rec = R.records([m], [t], (0, 0, 0), (5, 5, 5))[0]
        rec[field].reshape(-1)[1] = value
        assert R.refused(rec)
    rec = R.records([m], [t], (0, 0, 0), (5, 5, 5))[0]
    rec["op"] = 5
    assert R.refused(rec) and R.refused(None, flags=2) and R.refused(None, n=R.MAX_RESAMPLES + 1) and not R.refused(None, flags=R.DRY_RUN)
    assert R.refused(None, palette_map=[255] * 255) and not R.refused(None, palette_map=[254] * 255)


def limit_record(lo, hi, op=R.REPLACE):
    """m entries of +-8.0 and t of +-2^28 (4096 voxels) with an image inside the tree: s[0] = 8 (x + y + z) + 12 - 4096 lies in 0..255 for
    x + y + z in 511..542, s[1] = 4096 - 8 (x + y) - 8 for x + y in 480..511, s[2] = z"""
    m = [[R.MAX_M, R.MAX_M, R.MAX_M], [-R.MAX_M, -R.MAX_M, 0], [0, 0, R.ONE]]
    return R.records([m], [(-R.MAX_T, R.MAX_T, 0)], lo, hi, op)[0]


def test_limit_entries_that_still_reach_the_sub_box():
    src = np.zeros((256,) * 3, np.uint8)
    src[:] = (np.arange(256, dtype=np.uint8) | 1)[:, None, None]
    src[:, 100:140, :] = 0
    dst = np.zeros((256,) * 3, np.uint8)
    rec = limit_record((244, 244, 10), (255, 255, 21))
    assert not R.refused(rec)
    a, b = dst.copy(), dst.copy()
    got = R.resample_one(a, src, rec)
    assert got == R.loop_one(b, src, rec) and np.array_equal(a, b) and 100 < got[1] < 12 ** 3 and 0 < got[2] < got[1]
    for least, most in R.box_range(rec, [0, 0, 0], [255, 255, 255]):
        assert -(1 << 31) < least <= most < 1 << 31


def test_order_snapshot_palette_map_and_dry_run():
    src, dst = small_grids(4)
    recs = np.array(general_records())[[0, 6, 12, 18, 4]]
    together, counts = R.resample(dst, src, recs)
    grid = dst
    for k in range(len(recs)):
        grid, c = R.resample(grid, src, recs[k:k + 1])
        assert c.tolist() == counts[k:k + 1].tolist()
    assert np.array_equal(grid, together)
    swapped, _ = R.resample(dst, src, recs[::-1].copy())
    assert not np.array_equal(swapped, together)
    # src is dst: every record reads the grid as it stood when the call began
    own, _ = R.resample(dst, dst, recs)
    again = dst.copy()
    for r in recs:
        R.resample_one(again, dst, r)
    assert np.array_equal(own, again)
    # a dry run: the grid stands, each record is counted alone
    same, dry = R.resample(dst, src, recs, dry_run=True)
    assert np.array_equal(same, dst)
    for k in range(len(recs)):
        assert dry[k:k + 1].tolist() == R.resample(dst, src, recs[k:k + 1])[1].tolist()
    assert dry.tolist() != counts.tolist()
    # degenerate records
    none = [R.records([np.eye(3) * R.ONE], [(0, 0, 0)], lo, hi, R.REPLACE, sl, sh)[0]
            for lo, hi, sl, sh in (((5, 0, 0), (4, 9, 9), (0, 0, 0), (9, 9, 9)), ((0, 0, 0), (9, 9, 9), (0, 6, 0), (9, 5, 9)), ((256, 0, 0), (300, 9, 9), (0, 0, 0), (255, 255, 255)),
                                   ((-2 ** 31, -5, 0), (-1, 9, 9), (0, 0, 0), (255, 255, 255)))]
    out, c = R.resample(dst, src, none)
    assert np.array_equal(out, dst) and not c.view(np.uint32).any()
    # a singular map: every image voxel takes one source voxel's value
    zero = R.records([np.zeros((3, 3))], [(fixed(3.5), fixed(4.5), fixed(5.5))], (-3, 250, 7), (2, 260, 9), R.REPLACE)[0]
    out, c = R.resample(dst, src, [zero])
    assert (out[0:3, 250:256, 7:10] == src[3, 4, 5]).all() and c["covered"][0] == 3 * 6 * 3


def test_range_function_against_brute_force():
    rng = np.random.default_rng(5)
    rejected = 0
    for rec in general_records()[::5]:
        for _ in range(12):
            lo = [int(v) for v in rng.integers(0, 250, 3)]
            hi = [min(l + int(rng.integers(0, 16)), 255) for l in lo]
            m = rec["m"].astype(np.int64)
            axes = [2 * np.arange(lo[r], hi[r] + 1, dtype=np.int64) + 1 for r in range(3)]
            for k, (least, most) in enumerate(R.box_range(rec, lo, hi)):
                q = (m[k, 0] * axes[0])[:, None, None] + (m[k, 1] * axes[1])[None, :, None] + (m[k, 2] * axes[2])[None, None, :] + 2 * int(rec["t"][k])
                assert (least, most) == (int(q.min()), int(q.max()))
            if not R.box_can_hold(rec, lo, hi):
                rejected += 1
                assert not R.image_of(rec, lo, hi)[0].any()
    assert rejected > 5
