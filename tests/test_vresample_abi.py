"""CPU tests of the variable-ratio resampler's boundary: include/world_class_vresample.h declares every wc_vresample* symbol with its
arity, VRESAMPLE_SIGNATURES lists exactly those with that arity and their result types, the header and the translation unit are part
of the build, the mirror classes exist with their parameter names, the rational converter's table is untouched, and the tree compiles
for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "world_class_vresample.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_vresample_plan": (11, r"int\s+", C.c_int),
    "wc_vresample_filter": (9, r"int\s+", C.c_int),
    "wc_vresample_out_length": (2, r"long long\s+", C.c_longlong),
    "wc_vresample_committed": (6, r"long long\s+", C.c_longlong),
    "wc_vresample_tiling": (9, r"int\s+", C.c_int),
    "wc_vresampler_create": (7, r"wc_vresampler\s*\*", C.c_void_p),
    "wc_vresampler_destroy": (1, r"void\s+", None),
    "wc_vresample_device": (8, r"int\s+", C.c_int),
    "wc_vresample_stream_create": (9, r"wc_vresample_stream\s*\*", C.c_void_p),
    "wc_vresample_stream_destroy": (1, r"void\s+", None),
    "wc_vresample_stream_max_out_per_push": (1, r"int\s+", C.c_int),
    "wc_vresample_stream_reset": (2, r"int\s+", C.c_int),
    "wc_vresample_stream_set_step": (3, r"int\s+", C.c_int),
    "wc_vresample_stream_push_device": (8, r"int\s+", C.c_int),
    "wc_vresample_stream_samples_received": (2, r"long long\s+", C.c_longlong),
    "wc_vresample_stream_samples_committed": (2, r"long long\s+", C.c_longlong),
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
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result) == arity
    res, args = VRESAMPLE_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    assert declared_symbols(HEADER) == sorted(VRESAMPLE_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES as S
    ip, vp, i, d, ll, u64 = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double, C.c_longlong, C.c_ulonglong
    rule = [u64, u64, i, d, d, i, i]
    assert S["wc_vresample_plan"][1] == rule + [ip, ip, ip, C.POINTER(d)]
    assert S["wc_vresample_filter"][1] == rule + [C.POINTER(d), ll]
    assert S["wc_vresample_out_length"][1] == [u64, ll]
    assert S["wc_vresample_committed"][1] == [ll, C.c_uint, u64, i, ll, i]
    assert S["wc_vresample_tiling"][1] == [u64, u64, i, d, i, i, ip, ip, ip]
    assert S["wc_vresampler_create"][1] == rule
    assert S["wc_vresample_device"][1] == [vp, i, vp, i, ip, C.POINTER(u64), vp, i]
    assert S["wc_vresample_stream_create"][1] == rule + [i, i]
    assert S["wc_vresample_stream_set_step"][1] == [vp, i, u64]
    assert S["wc_vresample_stream_push_device"][1] == [vp, vp, i, ip, ip, vp, i, ip]


def test_steps_are_declared_unsigned_64_bit():
    src = _source(HEADER)
    assert len(re.findall(r"unsigned long long step_min, unsigned long long step_max", src)) == 5
    assert "const unsigned long long *step" in src and re.search(r"set_step\([^)]*unsigned long long step\)", src)


def test_header_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert "wc_vresample.hip" in build.sources() and "wc_resample.hip" in build.sources()
    assert os.path.join(build.CSRC, "wc_resample_dev.hpp") in build.headers()   # the device helpers the two converters share


def test_mirror_exists_with_its_parameter_names():
    from world_class_amd import vresample as vr
    sig = lambda f: list(inspect.signature(f).parameters)
    rule = ["step_min", "step_max", "zeros", "rolloff", "beta", "phase_bits", "degree"]
    assert sig(vr.plan) == rule and sig(vr.filter_table) == rule
    assert sig(vr.step_of) == ["ratio"] and sig(vr.out_length) == ["step", "n"]
    assert sig(vr.committed) == ["q", "f", "step", "half_width", "samples_in", "flushed"]
    assert sig(vr.tiling) == ["step_min", "step_max", "zeros", "rolloff", "phase_bits", "degree"]
    assert sig(vr.VResampler.__init__) == ["self"] + rule
    assert sig(vr.VResampler.run) == ["self", "xs", "steps", "out_format"]
    assert sig(vr.VResampler.run_device) == ["self", "d_x", "x_lengths", "steps", "d_y", "in_format", "out_format"]
    assert sig(vr.VResampleStream.__init__) == ["self", "step_min", "step_max", "n_streams", "max_samples"] + rule[2:]
    assert sig(vr.VResampleStream.push) == ["self", "chunks", "flush", "out_format"]
    assert sig(vr.VResampleStream.set_step) == ["self", "stream", "step"]
    assert inspect.signature(vr.VResampleStream.push).parameters["out_format"].default == "f64"
    for name in ("push_device", "reset", "samples_received", "samples_committed", "max_out_per_push", "close"):
        assert hasattr(vr.VResampleStream, name)
    assert hasattr(vr.VResampler, "close")


def test_existing_tables_are_unchanged():
    from world_class_amd import io as wio
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    assert len(RESAMPLE_SIGNATURES) == 15 and len(STREAM_SIGNATURES) == 46
    assert not set(VRESAMPLE_SIGNATURES) & (set(RESAMPLE_SIGNATURES) | set(STREAM_SIGNATURES) | set(wio.IO_SIGNATURES))
    for header in ("world_class_io.h", "world_class_stream.h", "world_class_resample.h"):
        assert "wc_vresampl" not in _source(header)


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
