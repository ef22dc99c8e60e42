"""CPU tests of the alignment streams' boundary: include/world_class_align_stream.h (which world_class_stream.h includes) declares
every wc_align_stream_* symbol with its arity, ALIGN_STREAM_SIGNATURES lists them with that arity and their result types and is
bound together with STREAM_SIGNATURES, the mirror class exists with its parameter names, the existing stream signatures are
unchanged, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "world_class_align_stream.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_align_stream_create": (7, r"wc_align_stream\s*\*", C.c_void_p),
    "wc_align_stream_destroy": (1, r"void\s+", None),
    "wc_align_stream_set_track_device": (4, r"int\s+", C.c_int),
    "wc_align_stream_reset": (4, r"int\s+", C.c_int),
    "wc_align_stream_push_device": (5, r"int\s+", C.c_int),
    "wc_align_stream_rows_received": (2, r"long long\s+", C.c_longlong),
    "wc_align_stream_track_length": (2, r"int\s+", C.c_int),
}


def _source(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_arity(symbol, result=r"[A-Za-z_ ]+?[\s*]+", header=HEADER):
    m = re.search(r"^\s*" + result + symbol + r"\s*\(([^)]*)\)\s*;", _source(header), flags=re.M)
    assert m, "%s does not declare %s(...) with that result" % (header, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.stream import ALIGN_STREAM_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result) == arity
    res, args = ALIGN_STREAM_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity
    assert symbol == "wc_align_stream_create" or args[0] is C.c_void_p  # (the handle)


def test_the_table_is_the_header_and_the_stream_header_includes_it():
    from world_class_amd.stream import ALIGN_STREAM_SIGNATURES, STREAM_SIGNATURES
    declared = sorted(set(re.findall(r"\b(wc_[a-z0-9_]+)\s*\(", _source(HEADER))))
    assert declared == sorted(ALIGN_STREAM_SIGNATURES) == sorted(NEW)
    assert not set(ALIGN_STREAM_SIGNATURES) & set(STREAM_SIGNATURES)
    assert re.search(r'^#include "%s"$' % re.escape(HEADER), _source("world_class_stream.h"), flags=re.M)


def test_argument_types():
    from world_class_amd.stream import ALIGN_STREAM_SIGNATURES as S
    ip, vp = C.POINTER(C.c_int), C.c_void_p
    assert S["wc_align_stream_create"][1] == [C.c_int] * 7
    assert S["wc_align_stream_set_track_device"][1] == [vp, C.c_int, C.c_int, vp]
    assert S["wc_align_stream_reset"][1] == [vp, C.c_int, C.c_int, C.c_int]
    assert S["wc_align_stream_push_device"][1] == [vp, ip, vp, vp, vp]


def test_mirror_class_exists_with_its_parameter_names():
    from world_class_amd.stream import AlignStream
    sig = lambda f: list(inspect.signature(f).parameters)
    p = inspect.signature(AlignStream.__init__).parameters
    assert list(p) == ["self", "dims", "n_streams", "n_tracks", "max_track_frames", "max_rows_per_push", "dim_begin", "dim_end"]
    assert (p["dim_begin"].default, p["dim_end"].default) == (1, None)
    assert sig(AlignStream.set_track) == ["self", "track", "feat"] and sig(AlignStream.set_track_device) == ["self", "track", "m", "d_feat"]
    assert sig(AlignStream.reset) == ["self", "stream", "track", "open_begin"]
    assert inspect.signature(AlignStream.reset).parameters["open_begin"].default is False
    assert sig(AlignStream.push) == ["self", "rows"]
    assert sig(AlignStream.push_device) == ["self", "n_rows", "d_feat", "d_position", "d_cost"]
    assert sig(AlignStream.rows_received) == ["self", "stream"] and sig(AlignStream.track_length) == ["self", "track"]
    assert sig(AlignStream.close) == ["self"]


def test_existing_stream_signatures_are_unchanged():
    from world_class_amd.stream import STREAM_SIGNATURES as S, MorphStream, StreamSynthesizer
    ip, vp = C.POINTER(C.c_int), C.c_void_p
    assert len(S) == 46 and not [n for n in S if n.startswith("wc_align_")]
    assert S["wc_synth_stream_push_device"] == (C.c_int, [vp, ip, ip, vp, vp, vp, vp, ip])
    assert S["wc_synth_stream_set_speed"] == (C.c_int, [vp, C.c_int, C.c_double])
    assert S["wc_morph_stream_create"] == (vp, [C.c_int] * 5)
    assert S["wc_morph_stream_set_speeds"] == (C.c_int, [vp, C.c_int, C.c_double, C.c_double])
    assert S["wc_morph_stream_push_device"] == (C.c_int, [vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, ip])
    for symbol, arity in (("wc_synth_stream_push_device", 8), ("wc_morph_stream_create", 5), ("wc_morph_stream_push_device", 13),
                          ("wc_morph_stream_set_speeds", 4), ("wc_stream_push_coded_device", 11)):
        assert declared_arity(symbol, header="world_class_stream.h") == arity
    assert list(inspect.signature(MorphStream.__init__).parameters) == ["self", "fs", "fft_size", "n_streams", "max_frames", "max_backlog"]
    assert list(inspect.signature(MorphStream.set_speeds).parameters) == ["self", "stream", "speed_a", "speed_b"]
    assert list(inspect.signature(StreamSynthesizer.push_device).parameters) == ["self", "n_frames", "d_f0", "d_sp", "d_ap", "flush", "d_y"]
    from world_class_amd import io as wio
    assert len(wio.IO_SIGNATURES["wc_align_features_ex_device"][1]) == 19 and len(wio.IO_SIGNATURES["wc_align_features_device"][1]) == 14


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
