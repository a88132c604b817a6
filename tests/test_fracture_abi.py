"""Model fracture on the host side (dust_hip_model_fracture, _fracture_at, _fracture_detach, _fracture_apply): the entry points are
declared, exported, bound, documented and mirrored; the four records' layouts and the constants are the same in the C header, the ctypes
binding, the numpy dtypes and the witness; the calls refuse without a device and leave the outputs alone; the header states the rules
and what is out of scope; the host helper makes the records the header describes; the C++ mirror compiles. (What device_fracture and
its companions make of every query, refusals included, is tests/test_fracture_rule.py's tables.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import fracture_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_fracture", "dust_hip_model_fracture_at", "dust_hip_model_fracture_detach", "dust_hip_model_fracture_apply")
RECORDS = ("DustHipFractureSeed", "DustHipFractureQuery", "DustHipFractureResult", "DustHipFractureCell")


def test_entry_points_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mirror = open(os.path.join(ROOT, "include", "dust_hip.hpp")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    lib = L.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header)
        assert name in L.SYMBOLS and getattr(lib, name) is not None
        assert re.search(r"pub fn " + name + r"\(", doc)
        assert re.search(r"\b" + name + r"\(", mirror) and re.search(r"`" + name + r"`", readme) and re.search(r"`" + name + r"`", design)
    for record in RECORDS:
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert all(callable(f) for f in (api.Model.fracture, api.Model.fracture_at, api.Model.fracture_detach, api.Model.fracture_apply, api.fracture_seeds))
    assert header.index("Model voxelisation:") < header.index("Model fracture:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model fracture:"):])   # (the comment's line breaks and stars out of the way, the products' too)
    block = block[:block.index("dust_hip_model_fracture_apply(DustHipModel")]
    for sentence in ("each in DUST_HIP_FRACTURE_SEED_MIN .. DUST_HIP_FRACTURE_SEED_MAX = -1024 .. 1279", "seeds may lie outside the tree",
                     "n_seeds == 0 is legal: nothing is labelled and `solid` is still counted", "d2(v, s) = sx (x - s.x)^2 + sy (y - s.y)^2 + sz (z - s.z)^2",
                     "d2 stays below 2^27", "clipped to the tree as dust_hip_model_columns clips it", "lo > hi on an axis is the empty region",
                     "minimises (d2, i) lexicographically", "ties go to the lowest index", "the later one gets nothing", "Every other voxel holds DUST_HIP_NO_CELL",
                     "it need not be connected", "both labelled, with different cells", "labelled with a higher cell index: seams are one voxel thick",
                     "exactly as flood does", "the lowest index among equals", "the sum of cells[i].cut_faces equals 2 cut_faces", "Two runs give the same bytes",
                     "byte for byte a host build", "The copy is made before the carve", "Duplicates and empty cells are legal",
                     "the rest of the labelling STANDS", "one fracture, then one KEEP_SOURCE detach per piece, then one deleting detach of all of them",
                     "Every decision is made on the labelling as it stands", "invalidated by exactly what invalidates the flood field",
                     "fracture leaves the island labelling and both other fields standing", "fracture_apply invalidates all of them",
                     "a cell index >= n_seeds", "exactly where set_voxels returns it", "DUST_ERR_NOT_READY"):
        assert sentence in block, sentence
    for scope in ("weighted (power) diagrams and non-integer seeds", "seeds chosen by the library", "find_islands does it", "world-space or scene-level fracture",
                  "an asynchronous form", "4096^3 trees"):                        # what the header rules out
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "fracture_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fracture_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipFractureSeed", L.FractureSeed, api.FRACTURE_SEED_DTYPE, W.SEED_DTYPE, 16),
               ("DustHipFractureQuery", L.FractureQuery, W.QUERY_DTYPE, W.QUERY_DTYPE, 48),
               ("DustHipFractureResult", L.FractureResult, api.FRACTURE_RESULT_DTYPE, W.RESULT_DTYPE, 64),
               ("DustHipFractureCell", L.FractureCell, api.FRACTURE_CELL_DTYPE, W.CELL_DTYPE, 40))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == dtype.itemsize == size
        assert [f for f, _ in struct._fields_] == list(witness.names) == list(dtype.names)
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1] == dtype.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            assert dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert c["DustHipFractureQuery.scale"] == 16 and c["DustHipFractureQuery.lo"] == 20 and c["DustHipFractureQuery.reserved"] == 44
    assert c["DustHipFractureResult.lo"] == 28 and c["DustHipFractureResult.reserved"] == 36
    # laid out like DustHipCensus
    assert c["DustHipFractureCell"] == c["DustHipCensus"] and [c["DustHipFractureCell." + f] for f in ("lo", "hi", "sum")] == [c["DustHipCensus." + f] for f in ("lo", "hi", "sum")]
    assert c["DUST_HIP_MAX_FRACTURE_SEEDS"] == L.MAX_FRACTURE_SEEDS == W.MAX_SEEDS == 4096
    assert (c["DUST_HIP_FRACTURE_SEED_MIN"], c["DUST_HIP_FRACTURE_SEED_MAX"]) == (L.FRACTURE_SEED_MIN, L.FRACTURE_SEED_MAX) == (W.SEED_MIN, W.SEED_MAX) == (-1024, 1279)
    assert c["DUST_HIP_FRACTURE_MAX_SCALE"] == L.FRACTURE_MAX_SCALE == W.MAX_SCALE == 16
    assert c["DUST_HIP_FRACTURE_NO_LIMIT"] == L.FRACTURE_NO_LIMIT == W.NO_LIMIT == 0xFFFFFFFF and c["DUST_HIP_NO_CELL"] == L.NO_CELL == W.NO_CELL == 0xFFFF
    assert (c["DUST_HIP_FRACTURE_SEAMS"], c["DUST_HIP_FRACTURE_LABELLED"]) == (L.FRACTURE_SEAMS, L.FRACTURE_LABELLED) == (W.SEAMS, W.LABELLED) == (0, 1)
    assert c["DUST_HIP_DETACH_KEEP_SOURCE"] == L.DETACH_KEEP_SOURCE
    # the metric's bound: the largest d2 any legal voxel and seed can have
    assert 3 * W.MAX_SCALE * max(255 - W.SEED_MIN, W.SEED_MAX) ** 2 < 1 << 27 and max(255 - W.SEED_MIN, W.SEED_MAX) < 1 << 11


def test_host_helper_makes_the_records_the_header_describes():
    s = api.fracture_seeds([(1, 2, 3), (-1024, 1279, 0)])
    assert s.dtype == api.FRACTURE_SEED_DTYPE and s["x"].tolist() == [1, -1024] and s["y"].tolist() == [2, 1279] and s["z"].tolist() == [3, 0] and not s["reserved"].any()
    assert s.tobytes() == W.seed_records([(1, 2, 3), (-1024, 1279, 0)]).tobytes()
    assert api.fracture_seeds(s) is s or api.fracture_seeds(s).tobytes() == s.tobytes()
    assert len(api.fracture_seeds(np.zeros((0, 3)))) == 0 and api.fracture_seeds([(5000, -5000, 7)])["x"].tolist() == [5000]      # not clamped: the call refuses


def test_calls_refuse_without_a_device_and_leave_the_outputs_alone():
    lib = L.load()
    seeds = W.seed_records([(1, 2, 3), (4, 5, 6)])
    sp = seeds.ctypes.data_as(C.c_void_p)
    result = np.full(64, 0x5A, np.uint8).view(api.FRACTURE_RESULT_DTYPE)
    cells = np.full(80, 0x5A, np.uint8).view(api.FRACTURE_CELL_DTYPE)
    labels = np.full(2, 0x5A5A, np.uint16)
    xyz = np.zeros((2, 3), np.uint32)
    which = np.zeros(2, np.uint32)
    changed = C.c_uint32(0x5A5A5A5A)
    out = C.c_void_p(0x5A5A)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def query(palette=-1, scale=(1, 1, 1), flags=0, reserved0=0, reserved=0, size=C.sizeof(L.FractureQuery)):
        q = L.FractureQuery(struct_size=size, flags=flags, palette=palette, max_distance2=L.FRACTURE_NO_LIMIT, reserved0=reserved0, reserved=reserved)
        q.scale[:] = scale
        q.hi[:] = (255, 255, 255)
        return q
    # a null model, with every other argument right or wrong
    queries = [query(), query(size=47), query(size=0), query(palette=255), query(palette=-2), query(scale=(0, 1, 1)), query(scale=(1, 1, 17)), query(flags=1),
               query(reserved0=1), query(reserved=7)]
    for q in queries:
        for n, pointer in ((2, sp), (0, None), (2, None), (L.MAX_FRACTURE_SEEDS + 1, sp)):
            assert lib.dust_hip_model_fracture(None, C.byref(q), pointer, n, ptr(result), ptr(cells)) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_fracture(None, None, None, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_fracture_at(None, ptr(xyz), ptr(labels), 2) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_fracture_at(None, None, None, 0) == L.ERR_INVALID_ARGUMENT
    for flags in (0, L.DETACH_KEEP_SOURCE, 2):
        assert lib.dust_hip_model_fracture_detach(None, ptr(which), 2, flags, C.byref(out)) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_fracture_detach(None, None, 0, flags, None) == L.ERR_INVALID_ARGUMENT
    for where, value in ((0, -1), (1, 254), (2, 0), (0, 255), (0, -2)):
        assert lib.dust_hip_model_fracture_apply(None, where, value, C.byref(changed)) == L.ERR_INVALID_ARGUMENT
    assert result.tobytes() == bytes([0x5A]) * 64 and cells.tobytes() == bytes([0x5A]) * 80 and labels.tolist() == [0x5A5A] * 2
    assert changed.value == 0x5A5A5A5A and out.value == 0x5A5A
    for q in queries[3:]:                                                         # ... and each of those is one the witness refuses too
        assert W.refused(q.palette, tuple(q.scale), q.flags, q.reserved0, q.reserved)
    assert not W.refused(254, (16, 16, 16)) and not W.refused(-1, (1, 16, 3))


def test_cpp_mirror_fracture_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "fracture_mirror.cpp"), "-o", str(tmp_path / "fracture_mirror.o")])
