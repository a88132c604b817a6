"""The witness of the model neighbourhoods (dust_hip_model_neighbours, dust_hip_model_neighbours_apply; the contract is in
include/dust_hip.h): whole-array numpy over a grid of bytes (0: empty, 1 + p: palette index p), written from the contract and
independently of the library's method -- no brick, no word, no bit plane. The solid array is padded with 0 (or with 1 under WALLS), the
6 / 18 / 26 shifted views are summed, born and died come from the masks, and a born voxel's material under MAJORITY is an argmax over a
vote count per palette index, lowest among equals. A grid smaller than 256^3 is a tree of its own size (the triple loop of
tests/test_neighbour_witness.py works on such)."""
import itertools

import numpy as np

FACES, EDGES, CORNERS = 6, 18, 26
NEIGHBOURHOODS = (FACES, EDGES, CORNERS)
WALLS, MAJORITY = 1, 2
BINS = 27
MAX_GENERATIONS = 256

QUERY_DTYPE = np.dtype([("struct_size", "<u4"), ("neighbourhood", "<u4"), ("flags", "<u4"), ("palette", "<i4"), ("lo", "<u4", 3), ("hi", "<u4", 3),
                        ("birth", "<u4"), ("survive", "<u4")])
RESULT_DTYPE = np.dtype([("voxels", "<u4"), ("solid", "<u4"), ("born", "<u4"), ("died", "<u4"), ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"),
                         ("reserved", "<u4", 10)])
APPLIED_DTYPE = np.dtype([("generations", "<u4"), ("solid_before", "<u4"), ("solid_after", "<u4"), ("reserved0", "<u4"), ("born", "<u8"), ("died", "<u8"),
                          ("lo", "u1", 3), ("pad0", "u1"), ("hi", "u1", 3), ("pad1", "u1"), ("reserved", "<u4", 6)])


def count_mask(*ranges):
    """bits over the count: each argument a count or an inclusive (first, last) pair"""
    mask = 0
    for r in ranges:
        first, last = (r, r) if isinstance(r, int) else r
        mask |= sum(1 << n for n in range(first, last + 1))
    return mask


def offsets(neighbourhood):
    """the offsets of a neighbourhood: |d|1 == 1, |d|1 <= 2 within the 3^3 box, the box without its centre"""
    reach = {FACES: 1, EDGES: 2, CORNERS: 3}[neighbourhood]
    found = [d for d in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(abs(c) for c in d) <= reach]
    assert len(found) == neighbourhood
    return found


def refused(neighbourhood, flags=0, palette=0, birth=0, survive=0, lo=(0, 0, 0), hi=(255, 255, 255), generations=1):
    """what the header lists under DUST_ERR_INVALID_ARGUMENT (the null pointers and the struct_size aside)"""
    if neighbourhood not in NEIGHBOURHOODS or flags & ~(WALLS | MAJORITY) or not 0 <= palette <= 254:
        return True
    if (birth | survive) >> (neighbourhood + 1):
        return True
    if any(c >= 256 for c in tuple(lo) + tuple(hi)):
        return True
    return not 1 <= generations <= MAX_GENERATIONS


def clip(grid, region):
    """the inclusive region inside the grid as (lo, hi), or None when it is empty"""
    lo, hi = ((0, 0, 0), tuple(s - 1 for s in grid.shape)) if region is None else region
    lo, hi = [int(v) for v in lo], [min(int(h), s - 1) for h, s in zip(hi, grid.shape)]
    return None if any(l > h for l, h in zip(lo, hi)) else (lo, hi)


def zero_result():
    r = np.zeros((), RESULT_DTYPE)
    r["lo"] = 255
    return r


def zero_applied():
    r = np.zeros((), APPLIED_DTYPE)
    r["lo"] = 255
    return r


def _window(array, lo, hi, fill):
    """array[lo - 1 .. hi + 1] on every axis, with `fill` where that leaves the tree"""
    out = np.full([h - l + 3 for l, h in zip(lo, hi)], fill, array.dtype)
    src = tuple(slice(max(l - 1, 0), min(h + 2, s)) for l, h, s in zip(lo, hi, array.shape))
    dst = tuple(slice(s.start - (l - 1), s.stop - (l - 1)) for s, l in zip(src, lo))
    out[dst] = array[src]
    return out


def _shifted(window, d):
    """the window's inner box moved by offset d: entry v holds what lies at v + d"""
    return window[tuple(slice(1 + c, window.shape[k] - 1 + c) for k, c in enumerate(d))]


def _work_box(grid, box, birth, walls):
    """the part of `box` in which a voxel can be solid or have a neighbour: all of it under WALLS, or when count 0 gives birth (then every
    voxel matters); otherwise the solid voxels' bounds grown by one. None: nothing there"""
    if walls or birth & 1:
        return box
    filled = [np.flatnonzero(grid.any(axis=tuple(a for a in range(3) if a != k))) for k in range(3)]
    if any(len(f) == 0 for f in filled):
        return None
    lo = [max(l, int(f[0]) - 1) for l, f in zip(box[0], filled)]
    hi = [min(h, int(f[-1]) + 1) for h, f in zip(box[1], filled)]
    return None if any(l > h for l, h in zip(lo, hi)) else (lo, hi)


def counts_in(grid, neighbourhood, lo, hi, walls=False):
    """the number of solid neighbours of every voxel of lo..hi"""
    window = _window((grid != 0).astype(np.uint8), lo, hi, 1 if walls else 0)
    total = np.zeros([h - l + 1 for l, h in zip(lo, hi)], np.uint8)
    for d in offsets(neighbourhood):
        total += _shifted(window, d)
    return total


def _bounds(mask, lo):
    where = np.argwhere(mask)
    if len(where) == 0:
        return [255] * 3, [0] * 3
    return (where.min(axis=0) + lo).tolist(), (where.max(axis=0) + lo).tolist()


def _decide(grid, neighbourhood, birth, survive, region, walls):
    """(box, work, n, solid, born, died): the clipped region, the part of it looked at, and there the counts and three masks; None for the
    empty region; work None when nothing of the region can be solid or have a neighbour"""
    box = clip(grid, region)
    if box is None:
        return None
    work = _work_box(grid, box, birth, walls)
    if work is None:
        return box, None, None, None, None, None
    lo, hi = work
    n = counts_in(grid, neighbourhood, lo, hi, walls)
    solid = grid[tuple(slice(l, h + 1) for l, h in zip(lo, hi))] != 0
    born = ~solid & (((birth >> n.astype(np.uint32)) & 1) != 0)
    died = solid & (((survive >> n.astype(np.uint32)) & 1) == 0)
    return box, work, n, solid, born, died


def neighbours(grid, neighbourhood, birth=0, survive=None, palette=0, region=None, walls=False):
    """(result, counts): the RESULT_DTYPE record and the (2, 27) table of dust_hip_model_neighbours"""
    if survive is None:
        survive = count_mask((0, neighbourhood))
    assert not refused(neighbourhood, WALLS if walls else 0, palette, birth, survive)
    counts = np.zeros((2, BINS), np.uint32)
    decided = _decide(grid, neighbourhood, birth, survive, region, walls)
    if decided is None:
        return zero_result(), counts
    box, work, n, solid, born, died = decided
    result = zero_result()
    result["voxels"] = int(np.prod([h - l + 1 for l, h in zip(*box)]))
    if work is None:
        counts[0, 0] = result["voxels"]
        return result, counts
    result["solid"], result["born"], result["died"] = np.count_nonzero(solid), np.count_nonzero(born), np.count_nonzero(died)
    result["lo"], result["hi"] = _bounds(born | died, work[0])
    counts[0] = np.bincount(n[~solid], minlength=BINS)
    counts[1] = np.bincount(n[solid], minlength=BINS)
    counts[0, 0] += int(result["voxels"]) - n.size          # the voxels of the region that were not looked at: empty, no neighbour
    return result, counts


def votes(grid, neighbourhood, voxels):
    """per voxel of an (n, 3) coordinate array: the byte most of its solid neighbours hold, the lowest among equals (0: nobody votes),
    how many neighbours vote, and whether the most common byte shares its count with another"""
    padded = np.pad(grid, 1)                                   # walls carry no material: 0 round the tree
    held = np.stack([padded[tuple((voxels[:, k] + 1 + d[k]) for k in range(3))] for d in offsets(neighbourhood)], axis=1)
    bytes_present = np.unique(grid)
    bytes_present = bytes_present[bytes_present != 0]
    if len(bytes_present) == 0 or len(voxels) == 0:
        return np.zeros(len(voxels), np.uint8), np.zeros(len(voxels), np.int64), np.zeros(len(voxels), bool)
    tally = np.stack([(held == b).sum(axis=1) for b in bytes_present], axis=1)     # ascending bytes: argmax takes the lowest among equals
    best = tally.max(axis=1)
    winner = np.where(best > 0, bytes_present[tally.argmax(axis=1)], 0).astype(np.uint8)
    return winner, tally.sum(axis=1), (best > 0) & ((tally == best[:, None]).sum(axis=1) > 1)


def step(grid, neighbourhood, birth, survive, palette=0, majority=False, region=None, walls=False):
    """one generation: (grid after, born, died, lo, hi, info) with the bounds of the changed voxels in the 255 / 0 convention; info
    counts the born voxels whose vote was a tie, had two or more voters, had none"""
    info = {"ties": 0, "voted_by_two": 0, "fallback": 0}
    decided = _decide(grid, neighbourhood, birth, survive, region, walls)
    if decided is None or decided[1] is None:
        return grid.copy(), 0, 0, [255] * 3, [0] * 3, info
    _, work, _, _, born, died = decided
    after = grid.copy()
    inner = after[tuple(slice(l, h + 1) for l, h in zip(*work))]
    inner[died] = 0
    if majority:
        voxels = np.argwhere(born) + np.array(work[0])
        winner, voters, tie = votes(grid, neighbourhood, voxels)
        inner[born] = np.where(winner != 0, winner, palette + 1)
        info = {"ties": int(np.count_nonzero(tie)), "voted_by_two": int(np.count_nonzero(voters >= 2)), "fallback": int(np.count_nonzero(winner == 0))}
    else:
        inner[born] = palette + 1
    lo, hi = _bounds(born | died, work[0])
    return after, int(np.count_nonzero(born)), int(np.count_nonzero(died)), lo, hi, info


def apply(grid, neighbourhood, birth, survive, generations=1, palette=0, majority=False, region=None, walls=False):
    """(grid after, applied, per_generation, info): what dust_hip_model_neighbours_apply leaves, its APPLIED_DTYPE record, the
    (generations, 2) table and the summed info of the steps"""
    assert not refused(neighbourhood, (WALLS if walls else 0) | (MAJORITY if majority else 0), palette, birth, survive, generations=generations)
    applied = zero_applied()
    table = np.zeros((generations, 2), np.uint32)
    info = {"ties": 0, "voted_by_two": 0, "fallback": 0}
    box = clip(grid, region)
    if box is None:
        return grid.copy(), applied, table, info
    inside = tuple(slice(l, h + 1) for l, h in zip(*box))
    applied["solid_before"] = np.count_nonzero(grid[inside])
    lo, hi = [255] * 3, [0] * 3
    now = grid
    for g in range(generations):
        now, born, died, step_lo, step_hi, step_info = step(now, neighbourhood, birth, survive, palette, majority, region, walls)
        if born + died == 0:
            break                                               # a fixed point: every later generation finds the same model
        table[g] = born, died
        applied["generations"] = g + 1
        lo, hi = [min(a, b) for a, b in zip(lo, step_lo)], [max(a, b) for a, b in zip(hi, step_hi)]
        for key in info:
            info[key] += step_info[key]
    applied["born"], applied["died"] = int(table[:, 0].sum(dtype=np.uint64)), int(table[:, 1].sum(dtype=np.uint64))
    applied["solid_after"] = np.count_nonzero(now[inside])
    applied["lo"], applied["hi"] = lo, hi
    return now.copy() if now is grid else now, applied, table, info
