"""Model casts on the host side (dust_hip_model_cast): the entry point is declared, exported, bound, documented and mirrored; the two
records' layouts and the constants are the same in the C header, the ctypes binding, the numpy dtypes and the witness; api.casts writes
the witness's records; the call refuses a null model without a device and leaves `hits` alone; the header says what is out of scope;
the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import cast_witness as W
from dust_amd import _lib as L
from dust_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_hip_model_cast"


def test_entry_point_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "dust_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mirror = open(os.path.join(ROOT, "include", "dust_hip.hpp")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    lib = L.load()
    assert re.search(r"\b" + NAME + r"\s*\(", header)
    assert NAME in L.SYMBOLS and getattr(lib, NAME) is not None
    assert re.search(r"pub fn " + NAME + r"\(", doc)
    assert re.search(r"\b" + NAME + r"\(", mirror) and re.search(r"`" + NAME + r"`", readme)
    for struct in ("DustHipCast", "DustHipCastHit"):
        assert re.search(r"#\[repr\(C\)\] pub struct " + struct + r" \{", doc), struct
    assert callable(api.Model.cast) and callable(api.casts)
    for scope in ("not an integer translation", "instances in world space", "undetached island", "4096^3", "asynchronous form"):   # what the header rules out
        assert scope in header, scope


def _c_layout(tmp_path):
    exe = str(tmp_path / "cast_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cast_layout.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_and_constants_match_the_header(tmp_path):
    c = _c_layout(tmp_path)
    assert c["DustHipCast"] == C.sizeof(L.Cast) == api.CAST_DTYPE.itemsize == W.CAST_DTYPE.itemsize == 48
    assert c["DustHipCastHit"] == C.sizeof(L.CastHit) == api.CAST_HIT_DTYPE.itemsize == W.HIT_DTYPE.itemsize == 32
    for name, struct, mine, witness in (("DustHipCast", L.Cast, api.CAST_DTYPE, W.CAST_DTYPE), ("DustHipCastHit", L.CastHit, api.CAST_HIT_DTYPE, W.HIT_DTYPE)):
        assert [f for f, _ in struct._fields_] == list(mine.names) == list(witness.names)
        for field, _ in struct._fields_:
            off = c[f"{name}.{field}"]
            assert getattr(struct, field).offset == off == mine.fields[field][1] == witness.fields[field][1], field
            assert mine.fields[field][0] == witness.fields[field][0], field
            assert getattr(struct, field).size == mine.fields[field][0].itemsize, field
    assert c["DUST_HIP_CAST_WALLS"] == L.CAST_WALLS == W.WALLS == 1
    assert c["DUST_HIP_CAST_HIT"] == L.CAST_HIT == W.HIT == 1
    assert c["DUST_HIP_CAST_OVERLAP"] == L.CAST_OVERLAP == W.OVERLAP == 2
    assert c["DUST_HIP_CAST_HIT_WALL"] == L.CAST_HIT_WALL == W.HIT_WALL == 4
    assert c["DUST_HIP_CAST_MAX_STEPS"] == L.CAST_MAX_STEPS == W.MAX_STEPS == 65535
    assert c["DUST_HIP_MAX_CASTS"] == L.MAX_CASTS == W.MAX_CASTS == 65536
    assert c["DUST_HIP_CAST_NO_KEY"] == L.CAST_NO_KEY == W.NO_KEY == 0xFFFFFFFF


def test_api_casts_writes_the_witness_records():
    rng = np.random.default_rng(1)
    n = 50
    offset = rng.integers(-2 ** 31, 2 ** 31, (n, 3))
    step = rng.integers(-1, 2, (n, 3))
    lo = rng.integers(0, 256, (n, 3))
    hi = rng.integers(0, 256, (n, 3))
    args = (offset, step, rng.integers(0, 65536, n), rng.integers(0, 512, n), rng.integers(0, 2, n), lo, hi)
    assert api.casts(*args).tobytes() == W.records(*args).tobytes()
    # scalars and single rows broadcast; the defaults are the identity, no flags, the whole tree
    one = api.casts([(1, -2, 3)] * 4, (0, -1, 0), 7)
    assert one.tobytes() == W.records([(1, -2, 3)] * 4, (0, -1, 0), 7).tobytes()
    assert one["orient"].tolist() == [api.ORIENT_IDENTITY] * 4 and one["src_hi"].tolist() == [[255] * 3] * 4 and one["step"].tolist() == [[0, -1, 0]] * 4


def test_call_refuses_without_a_model():
    lib = L.load()
    casts = api.casts([(0, 0, 0)] * 2, (0, -1, 0), 10)
    out = np.full(2, 0x5A, np.uint8).repeat(32).view(api.CAST_HIT_DTYPE)
    before = out.tobytes()
    cp, hp = casts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.dust_hip_model_cast(None, None, cp, 2, hp) == L.ERR_INVALID_ARGUMENT
    assert b"null" in lib.dust_hip_last_error()
    assert lib.dust_hip_model_cast(None, None, None, 0, None) == L.ERR_INVALID_ARGUMENT
    assert out.tobytes() == before


def test_cpp_mirror_casts_compile(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "cast_mirror.cpp"), "-o", str(tmp_path / "cast_mirror.o")])
