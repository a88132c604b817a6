"""The synchronous scene queries (dust_hip_scene_trace_rays / overlap_boxes / sweep_boxes) share three device staging slots of the
context with each other and with the island calls, grown on demand. One sequence of calls in which every one regrows or reuses a slot
another kind has just used, with a query of yet another kind in flight and model edits and island lookups in between: every synchronous
result is byte for byte what the device path (the _async calls on caller-owned tensors, which staging cannot touch) gives."""
import numpy as np
import pytest

import parity_util as P
from dust_amd import _lib as L
from dust_amd import api
from test_gpu_overlap import world_bounds

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (1, 65, 5000)
CAPACITY = 6                       # record slots per box query: some boxes hold more voxels, most fewer
SENTINEL = 0xA5C3F00D              # what every record word holds before a box query runs
ORDER = [("ray", 5000), ("overlap", 1), ("sweep", 5000), ("overlap", 5000), ("ray", 1), ("sweep", 65), ("ray", 65), ("overlap", 65)]
IN_FLIGHT = {"ray": "sweep", "overlap": "ray", "sweep": "overlap"}   # the kind enqueued just before a synchronous call of the key's kind


def batches(desc):
    """per kind and size: the records of the first n of 5000 random rays, boxes and sweeps over the scene"""
    rng = np.random.default_rng(7)
    lo, hi = world_bounds(desc)
    n = max(SIZES)
    at = lambda: lo + rng.random((n, 3)) * (hi - lo)
    origin = at() + rng.normal(size=(n, 3)) * 40.0
    toward = at() - origin
    rays = api.ray_records(origin, toward / np.linalg.norm(toward, axis=1, keepdims=True))
    blo = at()
    bhi = blo + rng.uniform(0.0, 5.0, (n, 3))
    slo = at()
    sweeps = api.box_sweeps(slo, slo + rng.uniform(0.0, 2.0, (n, 3)), rng.normal(size=(n, 3)) * 20.0)
    return {"ray": {k: rays[:k].copy() for k in SIZES},
            "overlap": {k: api.box_queries(blo[:k], bhi[:k], CAPACITY) for k in SIZES},
            "sweep": {k: sweeps[:k].copy() for k in SIZES}}


class DevicePath:
    """one _async call on tensors of its own: made before anything is enqueued, read after Context.sync()"""

    def __init__(self, torch, kind, records):
        self.kind, n = kind, len(records)
        self.inp = torch.from_numpy(records.view(np.int32).reshape(n, -1).copy()).to("cuda")
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
        if kind == "overlap":
            fill = int(np.uint32(SENTINEL).view(np.int32))
            self.out = (zeros(n), torch.full((n * CAPACITY, 4), fill, dtype=torch.int32, device="cuda"))
        else:
            self.out = (zeros(n, 8),)

    def enqueue(self, scene):
        if self.kind == "ray":
            scene.trace_rays(self.inp, hits=self.out[0])
        elif self.kind == "overlap":
            scene.overlap_boxes(self.inp, counts=self.out[0], records=self.out[1])
        else:
            scene.sweep_boxes(self.inp, hits=self.out[0])

    def result(self):
        return tuple(t.cpu().numpy().tobytes() for t in self.out)


def synchronous(scene, kind, records):
    """the synchronous call on host arrays: the same tuple of byte strings as DevicePath.result"""
    lib, n = L.load(), len(records)
    if kind == "ray":
        out = (np.zeros(n, api.HIT_DTYPE),)
        L.check(lib.dust_hip_scene_trace_rays(scene._h, api._ptr(records), api._ptr(out[0]), n, 0))
    elif kind == "overlap":
        out = (np.zeros(n, np.uint32), np.full(n * CAPACITY * 4, SENTINEL, np.uint32))
        L.check(lib.dust_hip_scene_overlap_boxes(scene._h, api._ptr(records), n, api._ptr(out[0]), api._ptr(out[1]), n * CAPACITY, 0))
    else:
        out = (np.zeros(n, api.SWEEP_HIT_DTYPE),)
        L.check(lib.dust_hip_scene_sweep_boxes(scene._h, api._ptr(records), api._ptr(out[0]), n, 0))
    return tuple(a.tobytes() for a in out)


def key(x, y, z):
    return (x << 16) | (y << 8) | z


def empty_model(ctx, pal):
    """an editable-kind (256^3) model, not in the scene, with no voxel left"""
    m = api.Model(ctx, *api.flatten_model(np.array([[0, 0, 0, 1]], np.uint8), (256, 256, 256), pal), pal)
    m.set_voxels([(0, 0, 255)], [-1])          # (where the loader puts the file's voxel (0, 0, 0): it mirrors one axis)
    return m


def test_synchronous_calls_share_regrown_staging():
    import torch
    desc = P.small_scene(seed=7)
    ctx = api.Context(device=0)
    scene = P.hip_scene(ctx, desc)
    batch = batches(desc)

    # the expected values: the device path, per kind and size
    expected = {}
    paths = [DevicePath(torch, kind, batch[kind][n]) for kind in batch for n in SIZES]
    flights = [DevicePath(torch, IN_FLIGHT[kind], batch[IN_FLIGHT[kind]][max(SIZES)]) for kind, _ in ORDER]
    torch.cuda.synchronize()               # the tensors are filled before the library's stream writes them
    for p in paths:
        p.enqueue(scene)
    ctx.sync()
    for p in paths:
        expected[p.kind, len(p.inp)] = p.result()
    ray_hits = np.count_nonzero(np.frombuffer(expected["ray", 5000][0], api.HIT_DTYPE)["instance"] != L.NO_HIT)
    sweep_hits = np.count_nonzero(np.frombuffer(expected["sweep", 5000][0], api.SWEEP_HIT_DTYPE)["instance"] != L.NO_HIT)
    counts = np.frombuffer(expected["overlap", 5000][0], np.uint32)
    over, under = np.count_nonzero(counts > CAPACITY), np.count_nonzero((counts > 0) & (counts < CAPACITY))
    print("hits of 5000: rays", ray_hits, "sweeps", sweep_hits, "boxes over / under capacity", over, under)
    assert min(ray_hits, sweep_hits) > 50 and over > 0 and under > 0      # the batches meet the scene; box slices fill, and stay part empty

    # what runs between the queries: voxel round trips on a model outside the scene, island lookups on two separated cubes
    rng = np.random.default_rng(8)
    scratch = empty_model(ctx, desc.palette)
    cubes = empty_model(ctx, desc.palette)
    a, b = (10, 12, 14), (40, 50, 60)
    solid = [(a[0] + x, a[1] + y, a[2] + z) for x in range(3) for y in range(3) for z in range(3)]
    solid += [(b[0] + x, b[1] + y, b[2] + z) for x in range(4) for y in range(4) for z in range(4)]
    cubes.set_voxels(solid, np.full(len(solid), 5))

    def round_trip(n):
        flat = rng.choice(256 ** 3, n, replace=False)
        xyz = np.stack([flat >> 16, (flat >> 8) & 255, flat & 255], 1)
        values = rng.integers(-1, 255, n)
        scratch.set_voxels(xyz, values)
        assert np.array_equal(scratch.get_voxels(xyz), values)

    def islands():
        n, rec = cubes.find_islands(L.ISLANDS_FACES)
        assert n == 2 and rec["key"].tolist() == [key(*a), key(*b)] and rec["voxels"].tolist() == [27, 64]
        probe = [a, (a[0] + 2, a[1] + 2, a[2] + 2), (a[0] + 3, a[1], a[2]), b, (b[0] + 3, b[1] + 1, b[2] + 2), (b[0] - 1, b[1], b[2])]
        assert cubes.island_of(probe).tolist() == [key(*a), key(*a), L.NO_ISLAND, key(*b), key(*b), L.NO_ISLAND]

    between = [lambda: round_trip(3), lambda: round_trip(3000), islands]

    # the sequence: a query of another kind is in flight whenever a slot is replaced
    for step, (kind, n) in enumerate(ORDER):
        flights[step].enqueue(scene)
        got = synchronous(scene, kind, batch[kind][n])
        assert got == expected[kind, n], (step, kind, n)
        if kind == "overlap":                 # the slots past each query's count hold what the caller wrote
            cnt = np.frombuffer(got[0], np.uint32)
            rec = np.frombuffer(got[1], np.uint32).reshape(n, CAPACITY, 4)
            unused = np.arange(CAPACITY)[None, :] >= np.minimum(cnt, CAPACITY)[:, None]
            assert unused.any() and np.all(rec[unused] == SENTINEL), (step, n)
            assert np.all(rec[~unused][:, 0] != SENTINEL)
        between[step % 3]()
    ctx.sync()
    for step, f in enumerate(flights):       # and the queries that were in flight meanwhile are whole
        assert f.result() == expected[f.kind, max(SIZES)], (step, f.kind)
