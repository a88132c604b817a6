"""Model neighbourhoods on the host side (dust_hip_model_neighbours, dust_hip_model_neighbours_apply): the entry points are declared,
exported, bound, documented and mirrored; the three records' layouts and the constants are the same in the C header, the ctypes
binding, the numpy dtypes and the witness; the query is a surface query field for field, with the two masks in its reserved words; the
calls refuse without a device and leave the outputs alone; the header states the contract and what is out of scope; the C++ mirror
compiles. (What device_neighbours makes of every query, refusals included, is tests/test_neighbour_rule.py's validation table.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import neighbour_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dust_hip_model_neighbours", "dust_hip_model_neighbours_apply")


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
    for record in ("DustHipNeighboursQuery", "DustHipNeighboursResult", "DustHipNeighboursApplied"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + record + r" \{", doc)
    assert callable(api.Model.neighbours) and callable(api.Model.neighbours_apply) and callable(api.count_mask)
    assert header.index("Model columns:") < header.index("Model neighbourhoods:")
    block = re.sub(r"[\s*]+", " ", header[header.index("Model neighbourhoods:"):])  # (the comment's line breaks and margin stars out of the way)
    block = block[:block.index("dust_hip_model_neighbours_apply(DustHipModel")]
    for sentence in ("the 3^3 box without its centre", "A neighbour outside the tree is empty, or solid under DUST_HIP_NEIGHBOURS_WALLS",
                     "An empty voxel with bit n of birth set becomes solid", "a solid voxel with bit n of survive clear becomes empty", "survivors keep their material",
                     "a synchronous update", "the lowest index among equals", "Walls carry no material and do not vote", "the fallback is query.palette",
                     "are consulted as they are, in every generation", "ask first, apply after", "1 + the index of the last generation that changed a voxel",
                     "the rows after a fixed point are 0", "how often it looks does not show in any output", "it needs no grid byte at all", "is never expanded",
                     "rebuilds ONCE", "even when nothing changed", "A null per_generation is fine"):
        assert sentence in block, sentence
    for scope in ("a list of the voxels that would change", "radius above 1, weighted or asymmetric neighbourhoods", "rules that count only one material",
                  "asynchronous (sequential-sweep) updates", "neighbourhoods across the instances of a scene", "4096^3 trees", "an asynchronous form",
                  "a brick worklist between generations"):                            # what the header rules out
        assert scope in block[block.index("Out of scope:"):], scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "neighbour_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "neighbour_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    records = (("DustHipNeighboursQuery", L.NeighboursQuery, api.NEIGHBOURS_QUERY_DTYPE, W.QUERY_DTYPE, 48),
               ("DustHipNeighboursResult", L.NeighboursResult, api.NEIGHBOURS_RESULT_DTYPE, W.RESULT_DTYPE, 64),
               ("DustHipNeighboursApplied", L.NeighboursApplied, api.NEIGHBOURS_APPLIED_DTYPE, W.APPLIED_DTYPE, 64))
    for name, struct, dtype, witness, size in records:
        assert c[name] == C.sizeof(struct) == witness.itemsize == dtype.itemsize == size
        assert [f for f, _ in struct._fields_] == list(witness.names) == list(dtype.names)
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == witness.fields[field][1] == dtype.fields[field][1], (name, field)
            assert getattr(struct, field).size == witness.fields[field][0].itemsize, (name, field)
            assert dtype.fields[field][0] == witness.fields[field][0], (name, field)
    assert c["DUST_HIP_NEIGHBOURS_FACES"] == L.NEIGHBOURS_FACES == W.FACES == 6 and c["DUST_HIP_NEIGHBOURS_EDGES"] == L.NEIGHBOURS_EDGES == W.EDGES == 18
    assert c["DUST_HIP_NEIGHBOURS_CORNERS"] == L.NEIGHBOURS_CORNERS == W.CORNERS == 26
    assert c["DUST_HIP_NEIGHBOURS_WALLS"] == L.NEIGHBOURS_WALLS == W.WALLS == c["DUST_HIP_SURFACE_WALLS"] == 1
    assert c["DUST_HIP_NEIGHBOURS_MAJORITY"] == L.NEIGHBOURS_MAJORITY == W.MAJORITY == 2
    assert c["DUST_HIP_NEIGHBOURS_BINS"] == L.NEIGHBOURS_BINS == W.BINS == 27
    assert c["DUST_HIP_NEIGHBOURS_MAX_GENERATIONS"] == L.NEIGHBOURS_MAX_GENERATIONS == W.MAX_GENERATIONS == 256


def test_the_query_is_a_surface_query_with_the_masks_in_its_reserved_words(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipNeighboursQuery"] == c["DustHipSurfaceQuery"] == C.sizeof(L.SurfaceQuery)
    for mine, other in (("struct_size", "struct_size"), ("neighbourhood", "faces"), ("flags", "flags"), ("palette", "palette"), ("lo", "lo"), ("hi", "hi"),
                        ("birth", "reserved")):
        assert getattr(L.NeighboursQuery, mine).offset == getattr(L.SurfaceQuery, other).offset == c["DustHipNeighboursQuery." + mine] == c["DustHipSurfaceQuery." + other]
    assert c["DustHipNeighboursQuery.survive"] == c["DustHipSurfaceQuery.reserved"] + 4 == 44
    assert dict(L.NeighboursQuery._fields_)["palette"] is C.c_int32
    assert dict(L.NeighboursApplied._fields_)["born"] is C.c_uint64 and c["DustHipNeighboursApplied.born"] == 16 and c["DustHipNeighboursApplied.died"] == 24


def test_count_mask():
    assert api.count_mask((14, 26)) == W.count_mask((14, 26)) == sum(1 << n for n in range(14, 27))
    assert api.count_mask(5, 6) == 0x60 and api.count_mask() == 0 and api.count_mask(0, (2, 3), np.int64(6)) == 0b1001101
    assert api.count_mask((0, 6)) == 0x7F and api.count_mask((0, 18)) == (1 << 19) - 1 and api.count_mask((0, 26)) == (1 << 27) - 1


def test_calls_refuse_without_a_device_and_leave_the_outputs_alone():
    lib = L.load()

    def query(neighbourhood=26, flags=0, palette=0, birth=0, survive=0, hi=(255, 255, 255), size=C.sizeof(L.NeighboursQuery)):
        q = L.NeighboursQuery(struct_size=size, neighbourhood=neighbourhood, flags=flags, palette=palette, birth=birth, survive=survive)
        q.hi[:] = hi
        return q
    result = np.full(64, 0x5A, np.uint8).view(api.NEIGHBOURS_RESULT_DTYPE)
    applied = np.full(64, 0x5A, np.uint8).view(api.NEIGHBOURS_APPLIED_DTYPE)
    counts = np.full(54, 0x5A5A5A5A, np.uint32)
    rows = np.full(512, 0x5A5A5A5A, np.uint32)
    before = result.tobytes(), applied.tobytes(), counts.tobytes(), rows.tobytes()
    rp, ap, cp, gp = (a.ctypes.data_as(C.c_void_p) for a in (result, applied, counts, rows))
    # every refusal of the header, through the entry points: a null model, then the query's faults one at a time
    queries = [query(), query(size=47), query(size=0), query(neighbourhood=0), query(neighbourhood=8), query(neighbourhood=27), query(flags=4), query(palette=-1),
               query(palette=255), query(birth=1 << 27), query(neighbourhood=6, survive=1 << 7), query(hi=(255, 256, 255))]
    for q in queries:
        assert lib.dust_hip_model_neighbours(None, C.byref(q), rp, cp) == L.ERR_INVALID_ARGUMENT
        assert lib.dust_hip_model_neighbours_apply(None, C.byref(q), 1, ap, gp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_neighbours(None, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.dust_hip_model_neighbours_apply(None, None, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert (result.tobytes(), applied.tobytes(), counts.tobytes(), rows.tobytes()) == before
    for q in queries[3:]:                                                         # ... and each of those is one the witness refuses too
        assert W.refused(q.neighbourhood, q.flags, q.palette, q.birth, q.survive, tuple(q.lo), tuple(q.hi))
    assert not W.refused(26, 3, 254, (1 << 27) - 1, (1 << 27) - 1) and W.refused(26, generations=0) and W.refused(26, generations=257)


def test_cpp_mirror_neighbour_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "neighbour_mirror.cpp"), "-o", str(tmp_path / "neighbour_mirror.o")])
