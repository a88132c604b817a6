"""The numpy witness of the model censuses (dust_hip_model_census; the contract is in include/dust_hip.h). A helper module, not a test:
tests/test_census_witness.py checks it on hand-built cases, tests/test_gpu_census.py holds the device to it.

Written from the header text on top of the shape edits' witness (tests/shape_edit_witness.py: `coverage`, the voxels whose centre a
shape contains under the float32 contract, and `covers_nothing`): every shape is counted on its own against the grid as it stands --
covered, the voxels the shape contains; solid, those of them that are not None; the inclusive bounds and the coordinate sums of the
solid covered voxels (255 / 0 and zero sums when there is none); and a row of 256 counters, [0] the covered voxels that hold None,
[1 + p] those that hold palette index p. The grid holds palette index + 1 per voxel, 0 = None, indexed [x, y, z]."""
import numpy as np

import shape_edit_witness as SW

BINS = 256
MAX_SHAPES = 65536
MAX_TABLES = 4096
RECORD_DTYPE = np.dtype([("covered", "<u4"), ("solid", "<u4"), ("lo", "u1", 3), ("reserved0", "u1"), ("hi", "u1", 3), ("reserved1", "u1"),
                         ("sum", "<u8", 3)])


def refused(shape_array, tables=True):
    """what the call refuses with DUST_ERR_INVALID_ARGUMENT (beyond null pointers): op, palette and reserved are not looked at"""
    s = np.asarray(shape_array, SW.SHAPE_DTYPE).reshape(-1)
    return bool(len(s) > MAX_SHAPES or (tables and len(s) > MAX_TABLES) or np.any(s["kind"] > SW.CAPSULE))


def zero_record():
    r = np.zeros(1, RECORD_DTYPE)[0]
    r["lo"] = 255
    return r


def census_one(grid, s):
    """one shape -> (record, row)"""
    record, row = zero_record(), np.zeros(BINS, np.uint32)
    if SW.covers_nothing(s):
        return record, row
    reg, m = SW.coverage(s)
    if not m.any():
        return record, row
    idx = np.argwhere(m)
    values = grid[reg][m]                      # (argwhere and boolean indexing walk the mask in the same order)
    row[:] = np.bincount(values, minlength=BINS)
    record["covered"] = len(values)
    solid = idx[values != 0] + np.array([r.start for r in reg])
    record["solid"] = len(solid)
    if len(solid):
        record["lo"], record["hi"] = solid.min(axis=0), solid.max(axis=0)
        record["sum"] = solid.sum(axis=0, dtype=np.uint64)
    return record, row


def census(grid, shape_array, tables=True):
    """(records, counts) of a call; counts is None with tables=False"""
    s = np.asarray(shape_array, SW.SHAPE_DTYPE).reshape(-1)
    assert not refused(s, tables)
    records, counts = np.zeros(len(s), RECORD_DTYPE), np.zeros((len(s), BINS), np.uint32)
    for i, one in enumerate(s):
        records[i], counts[i] = census_one(grid, one)
    return records, (counts if tables else None)
