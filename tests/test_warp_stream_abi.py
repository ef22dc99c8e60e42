"""CPU tests of the warp stream's boundary: include/world_class_warp_stream.h declares exactly the symbols of WARP_STREAM_SIGNATURES
with their arity and types, includes the warp's header and leaves it and its table alone, is part of the build, the mirror exists with
its parameter names, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_warp_stream.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_warp_stream_committed": (2, r"long long\s+", C.c_longlong),
    "wc_warp_along_map_device": (12, r"int\s+", C.c_int),
    "wc_warp_stream_create": (14, r"wc_warp_stream\s*\*\s*", C.c_void_p),
    "wc_warp_stream_destroy": (1, r"void\s+", None),
    "wc_warp_stream_set_track_device": (4, r"int\s+", C.c_int),
    "wc_warp_stream_reset": (6, r"int\s+", C.c_int),
    "wc_warp_stream_max_out_per_push": (1, r"int\s+", C.c_int),
    "wc_warp_stream_max_out_per_flush": (1, r"int\s+", C.c_int),
    "wc_warp_stream_push_device": (6, r"int\s+", C.c_int),
    "wc_warp_stream_flush_device": (6, r"int\s+", C.c_int),
    "wc_warp_stream_rows_received": (2, r"long long\s+", C.c_longlong),
    "wc_warp_stream_entries_consumed": (2, r"long long\s+", C.c_longlong),
    "wc_warp_stream_samples_committed": (2, r"long long\s+", C.c_longlong),
    "wc_warp_stream_get_delay": (2, r"int\s+", C.c_int),
    "wc_warp_stream_track_length": (2, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.warp_stream import WARP_STREAM_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = WARP_STREAM_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.warp_stream import WARP_STREAM_SIGNATURES
    assert declared_symbols(HEADER) == sorted(WARP_STREAM_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.warp_stream import WARP_STREAM_SIGNATURES as S
    ip, vp, i, d, ll, u64 = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double, C.c_longlong, C.c_ulonglong
    plan = [u64, u64, i, d, d, i, i]
    assert S["wc_warp_stream_committed"][1] == [ll, d]
    assert S["wc_warp_along_map_device"][1] == [vp, i, vp, i, ip, vp, ip, d, d, ip, vp, i]
    assert S["wc_warp_stream_create"][1] == plan + [i, i, i, i, i, i, d]
    assert S["wc_warp_stream_destroy"][1] == [vp]
    assert S["wc_warp_stream_set_track_device"][1] == [vp, i, i, vp]
    assert S["wc_warp_stream_reset"][1] == [vp, i, i, i, d, d]
    assert S["wc_warp_stream_push_device"][1] == S["wc_warp_stream_flush_device"][1] == [vp, ip, vp, vp, i, ip]
    for name in ("rows_received", "entries_consumed", "samples_committed", "get_delay", "track_length"):
        assert S["wc_warp_stream_" + name][1] == [vp, i]
    assert S["wc_warp_stream_max_out_per_push"][1] == S["wc_warp_stream_max_out_per_flush"][1] == [vp]


def test_the_header_states_its_types_and_includes_the_warps():
    src = _source(HEADER)
    assert re.search(r'#include\s+"world_class_warp.h"', src)
    assert re.search(r"wc_warp_stream_committed\(long long entries, double out_per_entry\)", src)
    assert "const double *d_map" in src and "const double *d_tail" in src and "int *samples_out" in src
    assert re.search(r"typedef struct wc_warp_stream wc_warp_stream;", src)
    assert re.search(r"wc_warp_stream_create\(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, double beta,\s+int phase_bits, int degree,", src)
    whole = open(os.path.join(ROOT, "include", HEADER)).read()
    for word in ("Bit identity", "carried", "(double)n / out_per_entry <= (double)(E - 1)"):   # the rule stands in the header
        assert word in whole


def test_the_warps_header_and_the_other_tables_are_unchanged():
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    from world_class_amd.warp import WARP_SIGNATURES
    from world_class_amd.warp_stream import WARP_STREAM_SIGNATURES
    assert len(WARP_SIGNATURES) == 5 and len(VRESAMPLE_SIGNATURES) == 16 and len(RESAMPLE_SIGNATURES) == 15 and len(STREAM_SIGNATURES) == 46
    assert not set(WARP_STREAM_SIGNATURES) & (set(WARP_SIGNATURES) | set(VRESAMPLE_SIGNATURES) | set(RESAMPLE_SIGNATURES) | set(STREAM_SIGNATURES))
    assert not [s for s in declared_symbols("world_class_warp.h") if s in WARP_STREAM_SIGNATURES]
    assert "wc_warp_stream" not in open(os.path.join(ROOT, "include", "world_class_warp.h")).read()


def test_header_is_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert os.path.join(ROOT, "include", "world_class_warp.h") in build.headers() and "wc_vresample.hip" in build.sources()


def test_mirror_exists_with_its_parameter_names():
    from world_class_amd import warp_stream as ws
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(ws.committed) == ["entries", "out_per_entry"]
    assert sig(ws.warp_along_map_device) == ["resampler", "d_x", "x_lengths", "d_map", "map_lengths", "out_per_entry", "in_per_unit", "out_lengths",
                                             "d_y", "in_format", "out_format"]
    assert sig(ws.WarpStream.__init__) == ["self", "step_min", "step_max", "n_streams", "n_tracks", "max_track_samples", "max_entries_per_push",
                                           "max_delay", "max_out_per_entry", "track_format", "zeros", "rolloff", "beta", "phase_bits", "degree"]
    assert sig(ws.WarpStream.set_track) == ["self", "track", "x"]
    assert sig(ws.WarpStream.set_track_device) == ["self", "track", "n_samples", "d_x"]
    assert sig(ws.WarpStream.reset) == ["self", "stream", "track", "delay", "out_per_entry", "in_per_unit"]
    assert sig(ws.WarpStream.push_device) == ["self", "n_rows", "d_map", "d_y", "out_format"]
    assert sig(ws.WarpStream.flush_device) == ["self", "want", "d_tail", "d_y", "out_format"]
    for name in ("rows_received", "entries_consumed", "samples_committed", "get_delay"):
        assert sig(getattr(ws.WarpStream, name)) == ["self", "stream"]
    assert sig(ws.WarpStream.track_length) == ["self", "track"]
    assert inspect.signature(ws.WarpStream.push_device).parameters["out_format"].default == "f64"


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
