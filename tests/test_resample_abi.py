"""CPU tests of the resampler's boundary: include/world_class_resample.h declares every wc_resample* symbol with its arity,
RESAMPLE_SIGNATURES lists exactly those with that arity and their result types, the header and the translation unit are part of the
build, the mirror classes exist with their parameter names, the io and stream tables are untouched, and the tree compiles for gfx950
without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "world_class_resample.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_resample_plan": (8, r"int\s+", C.c_int),
    "wc_resample_filter": (7, r"int\s+", C.c_int),
    "wc_resample_out_length": (3, r"long long\s+", C.c_longlong),
    "wc_resample_committed": (6, r"long long\s+", C.c_longlong),
    "wc_resample_tiling": (7, r"int\s+", C.c_int),
    "wc_resampler_create": (5, r"wc_resampler\s*\*", C.c_void_p),
    "wc_resampler_destroy": (1, r"void\s+", None),
    "wc_resample_device": (7, r"int\s+", C.c_int),
    "wc_resample_stream_create": (7, r"wc_resample_stream\s*\*", C.c_void_p),
    "wc_resample_stream_destroy": (1, r"void\s+", None),
    "wc_resample_stream_max_out_per_push": (1, r"int\s+", C.c_int),
    "wc_resample_stream_reset": (2, r"int\s+", C.c_int),
    "wc_resample_stream_push_device": (8, r"int\s+", C.c_int),
    "wc_resample_stream_samples_received": (2, r"long long\s+", C.c_longlong),
    "wc_resample_stream_samples_committed": (2, r"long long\s+", C.c_longlong),
}


def _source(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_arity(symbol, result=r"[A-Za-z_ ]+?[\s*]+", header=HEADER):
    m = re.search(r"^\s*" + result + symbol + r"\s*\(([^)]*)\)\s*;", _source(header), flags=re.M)
    assert m, "%s does not declare %s(...) with that result" % (header, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


def declared_symbols(header, name=r"wc_[a-z0-9_]+"):
    return sorted(set(re.findall(r"\b(" + name + r")\s*\(", re.sub(r"//[^\n]*", "", _source(header)))))


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result) == arity
    res, args = RESAMPLE_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    assert declared_symbols(HEADER) == sorted(RESAMPLE_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.resample import RESAMPLE_SIGNATURES as S
    ip, vp, i, d, ll = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double, C.c_longlong
    rule = [i, i, i, d, d]
    assert S["wc_resample_plan"][1] == rule + [ip, ip, ip]
    assert S["wc_resample_filter"][1] == rule + [C.POINTER(d), ll]
    assert S["wc_resample_out_length"][1] == [i, i, ll]
    assert S["wc_resample_committed"][1] == [i, i, i, d, ll, i]
    assert S["wc_resampler_create"][1] == rule
    assert S["wc_resample_device"][1] == [vp, i, vp, i, ip, vp, i]
    assert S["wc_resample_stream_create"][1] == rule + [i, i]
    assert S["wc_resample_stream_push_device"][1] == [vp, vp, i, ip, ip, vp, i, ip]


def test_header_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert "wc_resample.hip" in build.sources()


def test_mirror_exists_with_its_parameter_names():
    from world_class_amd import resample as rs
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(rs.plan) == ["fs_in", "fs_out", "zeros", "rolloff", "beta"] and sig(rs.filter_taps) == sig(rs.plan)
    assert sig(rs.out_length) == ["fs_in", "fs_out", "n"]
    assert sig(rs.committed) == ["fs_in", "fs_out", "samples_in", "flushed", "zeros", "rolloff"]
    assert sig(rs.Resampler.__init__) == ["self", "fs_in", "fs_out", "zeros", "rolloff", "beta"]
    assert sig(rs.Resampler.run) == ["self", "xs", "out_format"]
    assert sig(rs.ResampleStream.__init__) == ["self", "fs_in", "fs_out", "n_streams", "max_samples", "zeros", "rolloff", "beta"]
    assert sig(rs.ResampleStream.push) == ["self", "chunks", "flush", "out_format"]
    assert inspect.signature(rs.ResampleStream.push).parameters["out_format"].default == "f64"
    for name in ("push_device", "reset", "samples_received", "samples_committed", "max_out_per_push", "close"):
        assert hasattr(rs.ResampleStream, name)
    for name in ("run_device", "close"):
        assert hasattr(rs.Resampler, name)


def test_existing_tables_are_unchanged():
    from world_class_amd import io as wio
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    assert len(STREAM_SIGNATURES) == 46
    assert sorted(wio.IO_SIGNATURES) == declared_symbols("world_class_io.h", r"[A-Za-z_][A-Za-z0-9_]*")  # (wavread and its kin too)
    assert not set(RESAMPLE_SIGNATURES) & (set(STREAM_SIGNATURES) | set(wio.IO_SIGNATURES))
    for header in ("world_class_io.h", "world_class_stream.h"):
        assert "wc_resampl" not in _source(header)


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
