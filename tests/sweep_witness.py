"""The numpy witness of the scene box sweeps (dust_hip_scene_sweep_boxes; the contract is in include/dust_hip.h). A helper module, not a
test: tests/test_sweep_witness.py checks it on hand-built scenes, tests/test_gpu_sweep.py holds the device to it.

Axis-aligned instances: the header's float32 arithmetic, operation by operation (numpy float32 subtractions and divisions round to
nearest), over every voxel of every instance the swept box can reach; the answer minimises (t, instance, block, voxel). Other
instances: a float64 continuous separating-axis test against the box grown or shrunk by tau, for the tolerance check."""
import numpy as np

from dust_amd import api
from test_gpu_overlap import model_voxels, world_boxes32

F = np.float32
INF = F(np.inf)


def miss():
    h = np.zeros(1, api.SWEEP_HIT_DTYPE)[0]
    h["t"] = 1.0
    h["instance"] = 0xFFFFFFFF
    return h


def degenerate(lo, hi, d):
    return not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(np.isfinite(d)) and np.all(lo <= hi))


def slab_times(a, b, lo, hi, d):
    """the contract's entry / exit times of world slabs [a, b] (float32 arrays) on one axis; a resting axis: in contact throughout or never"""
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        if d > 0:
            return (a - hi) / d, (b - lo) / d
        if d < 0:
            return (b - lo) / d, (a - hi) / d
    c = ((a < hi) & (lo < b)) if lo < hi else ((a <= lo) & (lo < b))
    return np.where(c, -INF, INF).astype(F), np.where(c, INF, -INF).astype(F)


def aligned(t):
    a = np.asarray(t, F).reshape(3, 4)[:, :3]
    return bool(np.all((a != 0).sum(0) == 1) and np.all((a != 0).sum(1) == 1))


class SweepWitness:
    def __init__(self, desc):
        self.desc = desc
        self.mv = {}
        self.inst = []
        for mid, t in desc.instances:
            if mid not in self.mv:
                self.mv[mid] = model_voxels(*desc.models[mid])
            xyz = self.mv[mid][0]
            if aligned(t):
                lo, hi = world_boxes32(xyz, t)
                self.inst.append((True, lo, hi))
            else:
                self.inst.append((False, None, None))
        # each instance's world bounds, padded well beyond the float32 rounding of its voxel corners
        self._blo = np.full((len(desc.instances), 3), np.inf)
        self._bhi = np.full((len(desc.instances), 3), -np.inf)
        for i, (mid, t) in enumerate(desc.instances):
            xyz = self.mv[mid][0]
            if len(xyz):
                m = np.asarray(t, np.float64).reshape(3, 4)
                w = np.concatenate([xyz.min(0) + np.array([(c >> k) & 1 for k in range(3)]) * (xyz.max(0) + 1 - xyz.min(0))
                                    for c in range(8)]).reshape(8, 3) @ m[:, :3].T + m[:, 3]
                pad = 1e-3 * (1.0 + np.abs(w).max() + np.abs(m[:, 3]).max())
                self._blo[i], self._bhi[i] = w.min(0) - pad, w.max(0) + pad

    def _near(self, slo, shi):
        return np.nonzero(np.all(self._bhi >= slo, axis=1) & np.all(self._blo <= shi, axis=1))[0].tolist()

    # ---------------------------------------------------------------- exact (axis-aligned instances)
    def exact(self, lo, hi, d, any_hit=False, ignore_start=False):
        """the contract's record for one sweep (instances must be axis-aligned); with any_hit, every hit record (a list)"""
        lo, hi, d = np.asarray(lo, F), np.asarray(hi, F), np.asarray(d, F)
        if degenerate(lo, hi, d):
            return [] if any_hit else miss()
        with np.errstate(over="ignore"):
            slo, shi = np.minimum(lo, lo + d).astype(np.float64), np.maximum(hi, hi + d).astype(np.float64)
        rows = []
        for i in self._near(slo, shi):
            ok, vlo, vhi = self.inst[i]
            assert ok, "exact witness on an instance that is not axis-aligned"
            keep = np.all(vhi >= slo.astype(F), axis=1) & np.all(vlo <= shi.astype(F), axis=1)
            k = np.nonzero(keep)[0]
            if len(k) == 0:
                continue
            e = np.empty((len(k), 3), F)
            x = np.empty((len(k), 3), F)
            for r in range(3):
                e[:, r], x[:, r] = slab_times(vlo[k, r], vhi[k, r], lo[r], hi[r], d[r])
            tin, tout = e.max(1), x.min(1)
            hit = (tin < tout) & (tin < 1) & (tout > 0)
            if ignore_start:
                hit &= tin >= 0
            for j in np.nonzero(hit)[0]:
                rows.append((float(np.where(tin[j] > 0, tin[j], F(0))), i, int(k[j]), e[j], tin[j]))
        if not rows:
            return [] if any_hit else miss()
        recs = [self._record(d, *r) for r in rows]
        if any_hit:
            return recs
        order = sorted(range(len(rows)), key=lambda n: (rows[n][0], rows[n][1], self.mv[self.desc.instances[rows[n][1]][0]][1][rows[n][2]],
                                                         self.mv[self.desc.instances[rows[n][1]][0]][2][rows[n][2]]))
        return recs[order[0]]

    def _record(self, d, t, i, k, e, tin):
        mid = self.desc.instances[i][0]
        xyz, blk, vox, pal = self.mv[mid]
        h = np.zeros(1, api.SWEEP_HIT_DTYPE)[0]
        h["t"] = F(t)
        h["instance"], h["block"], h["voxel"], h["palette"] = i, blk[k], vox[k], pal[k]
        h["xyz"] = xyz[k]
        n = np.zeros(3, F)
        if tin >= 0:
            for r in range(3):
                if d[r] != 0 and e[r] == tin:
                    n[r] = -1.0 if d[r] > 0 else 1.0
                    break
        h["normal"] = n
        return h

    # ---------------------------------------------------------------- tolerance (any instances)
    def contact_times(self, lo, hi, d, s):
        """float64 continuous SAT of every voxel near the sweep against the box grown by s * tau (s = +1 or -1): a list of
        (instance, block, voxel, tin, tout) with tin < tout (s < 0) or tin <= tout (s > 0)"""
        lo, hi, d = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(d, np.float64)
        slo, shi = np.minimum(lo, lo + d), np.maximum(hi, hi + d)
        ctr, half = (lo + hi) / 2.0, (hi - lo) / 2.0
        mbox = np.abs(np.concatenate([lo, hi, lo + d, hi + d])).max()
        out = []
        for i in self._near(slo - 1.0, shi + 1.0):
            mid, t = self.desc.instances[i]
            xyz, blk, vox, _ = self.mv[mid]
            m = np.asarray(t, np.float64).reshape(3, 4)
            a, tr = m[:, :3], m[:, 3]
            cols = [a[:, k] for k in range(3)]
            ax = np.array([np.eye(3)[r] for r in range(3)] + [np.cross(cols[(k + 1) % 3], cols[(k + 2) % 3]) for k in range(3)] +
                          [np.cross(np.eye(3)[r], cols[k]) for r in range(3) for k in range(3)])
            c = (xyz + 0.5) @ a.T + tr
            ext = 0.5 * np.abs(a).sum(axis=1)
            big = np.maximum(mbox, (np.abs(c) + ext).max(axis=1))
            tau = 1e-5 * (1.0 + big)
            h = half[None, :] + s * tau[:, None]
            valid = np.all(h >= 0.0, axis=1)
            reach = 0.5 * np.abs(ax @ a).sum(axis=1)[None, :] + h @ np.abs(ax).T          # (n, 15)
            dist = (c - ctr) @ ax.T                                                        # (n, 15)
            speed = ax @ d                                                                 # (15,)
            tin = np.full(len(xyz), -np.inf)
            tout = np.full(len(xyz), np.inf)
            for k in range(15):
                if abs(speed[k]) < 1e-12:
                    sep = np.abs(dist[:, k]) > reach[:, k]
                    tin = np.where(sep, np.inf, tin)
                    tout = np.where(sep, -np.inf, tout)
                else:
                    e0, e1 = (dist[:, k] - reach[:, k]) / speed[k], (dist[:, k] + reach[:, k]) / speed[k]
                    tin = np.maximum(tin, np.minimum(e0, e1))
                    tout = np.minimum(tout, np.maximum(e0, e1))
            ok = valid & ((tin < tout) if s < 0 else (tin <= tout)) & (tin < 1.0) & (tout > 0.0)
            for j in np.nonzero(ok)[0]:
                out.append((i, int(blk[j]), int(vox[j]), float(tin[j]), float(tout[j])))
        return out


def first_time(contacts):
    return min((max(c[3], 0.0) for c in contacts), default=1.0)
