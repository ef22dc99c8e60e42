"""CPU tests of the warp's boundary: include/world_class_warp.h declares every wc_warp* symbol with its arity, WARP_SIGNATURES lists
exactly those with that arity and their types, the header is part of the build and includes the converter's, which holds none of it,
the other tables keep their sizes, the mirror exists with its parameter names, and the tree compiles for gfx950 without a GPU and
exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_warp.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_warp_tiling": (10, r"int\s+", C.c_int),
    "wc_warp_map_out_length": (2, r"long long\s+", C.c_longlong),
    "wc_warp_map_positions": (6, r"int\s+", C.c_int),
    "wc_warp_device": (9, r"int\s+", C.c_int),
    "wc_warp_map_positions_device": (8, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.warp import WARP_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = WARP_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.warp import WARP_SIGNATURES
    assert declared_symbols(HEADER) == sorted(WARP_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.warp import WARP_SIGNATURES as S
    ip, vp, i, d, ll, u64 = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double, C.c_longlong, C.c_ulonglong
    assert S["wc_warp_tiling"][1] == [u64, u64, i, d, i, i, ip, ip, ip, ip]
    assert S["wc_warp_map_out_length"][1] == [i, d]
    assert S["wc_warp_map_positions"][1] == [C.POINTER(d), i, d, d, ll, C.POINTER(ll)]
    assert S["wc_warp_device"][1] == [vp, i, vp, i, ip, vp, ip, vp, i]
    assert S["wc_warp_map_positions_device"][1] == [vp, i, vp, ip, d, d, ip, vp]


def test_positions_are_declared_signed_64_bit_and_no_position_is_the_lowest():
    from world_class_amd import warp
    src = _source(HEADER)
    assert "const long long *d_pos" in src and re.search(r"long long \*d_pos\)", src) and re.search(r"long long n_out, long long \*pos\)", src)
    assert re.search(r"#define\s+WC_WARP_NO_POSITION\s+LLONG_MIN", src) and warp.NO_POSITION == -(1 << 63)
    assert re.search(r'#include\s+"world_class_vresample.h"', src)


def test_the_converters_header_and_tables_are_unchanged():
    from world_class_amd import io as wio
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    from world_class_amd.warp import WARP_SIGNATURES
    assert len(VRESAMPLE_SIGNATURES) == 16 and len(RESAMPLE_SIGNATURES) == 15 and len(STREAM_SIGNATURES) == 46
    assert not set(WARP_SIGNATURES) & (set(VRESAMPLE_SIGNATURES) | set(RESAMPLE_SIGNATURES) | set(STREAM_SIGNATURES) | set(wio.IO_SIGNATURES))
    for header in ("world_class_vresample.h", "world_class_resample.h", "world_class_io.h", "world_class_stream.h"):
        assert "wc_warp" not in open(os.path.join(ROOT, "include", header)).read()


def test_header_is_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert os.path.join(ROOT, "include", "world_class_vresample.h") in build.headers() and "wc_vresample.hip" in build.sources()


def test_mirror_exists_with_its_parameter_names():
    from world_class_amd import warp
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(warp.tiling) == ["step_min", "step_max", "zeros", "rolloff", "phase_bits", "degree"]
    assert sig(warp.map_out_length) == ["map_length", "out_per_entry"]
    assert sig(warp.map_positions) == ["time_map", "out_per_entry", "in_per_unit", "n_out"]
    assert sig(warp.map_positions_device) == ["resampler", "d_map", "map_lengths", "out_per_entry", "in_per_unit", "out_lengths", "d_pos"]
    assert sig(warp.warp_device) == ["resampler", "d_x", "x_lengths", "d_pos", "out_lengths", "d_y", "in_format", "out_format"]
    assert sig(warp.warp) == ["resampler", "xs", "positions", "out_format"]
    assert inspect.signature(warp.warp).parameters["out_format"].default == "f64"


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
