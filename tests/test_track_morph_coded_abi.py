"""CPU tests of the coded track-morph streams' boundary: include/world_class_track_morph_coded.h (a header of its own, which
world_class_stream.h does NOT include and which includes world_class_stream.h and world_class_codec.h itself) declares exactly the
wc_track_morph_coded_* calls with their arities and results -- wc_track_morph's thirteen with number_of_dimensions added to create,
and device_bytes -- TRACK_MORPH_CODED_SIGNATURES lists them with that arity and their result types, is bound with the other five
tables and shares no symbol with them (whose sizes stay 46, 7, 2, 5 and 13), the mirror class exists with its parameter names and
defaults, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_track_morph_abi import _source, declared_arity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "world_class_track_morph_coded.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_track_morph_coded_create": (8, r"wc_track_morph_coded\s*\*", C.c_void_p),
    "wc_track_morph_coded_destroy": (1, r"void\s+", None),
    "wc_track_morph_coded_set_track_device": (6, r"int\s+", C.c_int),
    "wc_track_morph_coded_reset": (4, r"int\s+", C.c_int),
    "wc_track_morph_coded_set_weight": (4, r"int\s+", C.c_int),
    "wc_track_morph_coded_set_ratios": (4, r"int\s+", C.c_int),
    "wc_track_morph_coded_push_device": (10, r"int\s+", C.c_int),
    "wc_track_morph_coded_flush_device": (7, r"int\s+", C.c_int),
    "wc_track_morph_coded_frames_received": (2, r"long long\s+", C.c_longlong),
    "wc_track_morph_coded_frames_formed": (2, r"long long\s+", C.c_longlong),
    "wc_track_morph_coded_pending": (2, r"int\s+", C.c_int),
    "wc_track_morph_coded_get_delay": (2, r"int\s+", C.c_int),
    "wc_track_morph_coded_track_length": (2, r"int\s+", C.c_int),
    "wc_track_morph_coded_device_bytes": (1, r"long long\s+", C.c_longlong),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.stream import TRACK_MORPH_CODED_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, HEADER) == arity
    res, args = TRACK_MORPH_CODED_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity
    assert symbol == "wc_track_morph_coded_create" or args[0] is C.c_void_p  # (the handle)


def test_the_table_is_the_header_and_disjoint_from_the_other_five():
    from world_class_amd.stream import (ALIGN_LAG_SIGNATURES, ALIGN_STREAM_SIGNATURES, ALIGN_WINDOW_SIGNATURES, STREAM_SIGNATURES,
                                        TRACK_MORPH_CODED_SIGNATURES, TRACK_MORPH_SIGNATURES)
    declared = sorted(set(re.findall(r"\b(wc_[a-z0-9_]+)\s*\(", _source(HEADER))))
    assert declared == sorted(TRACK_MORPH_CODED_SIGNATURES) == sorted(NEW)
    assert re.search(r"typedef struct wc_track_morph_coded wc_track_morph_coded;", _source(HEADER))
    others = [STREAM_SIGNATURES, ALIGN_STREAM_SIGNATURES, ALIGN_WINDOW_SIGNATURES, ALIGN_LAG_SIGNATURES, TRACK_MORPH_SIGNATURES]
    assert not set(TRACK_MORPH_CODED_SIGNATURES) & set().union(*others)
    assert [len(t) for t in others] == [46, 7, 2, 5, 13]
    # the coded calls are the full-row calls' names with the same arguments, create apart, and one getter more
    for name, (res, args) in TRACK_MORPH_SIGNATURES.items():
        coded = TRACK_MORPH_CODED_SIGNATURES[name.replace("wc_track_morph_", "wc_track_morph_coded_")]
        assert coded == ((res, [C.c_int] + args) if name.endswith("_create") else (res, args)), name


def test_a_header_of_its_own_that_the_stream_header_does_not_include():
    assert HEADER not in _source("world_class_stream.h")
    own = [l.strip() for l in _source(HEADER).splitlines() if l.strip().startswith("#include")]
    assert own == ['#include "world_class_stream.h"', '#include "world_class_codec.h"']
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert "wc_track_morph_coded.hip" in build.sources()


def test_argument_types_and_binding():
    from world_class_amd import stream
    ip, vp, i, d = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double
    S = stream.TRACK_MORPH_CODED_SIGNATURES
    assert S["wc_track_morph_coded_create"][1] == [i] * 8
    assert S["wc_track_morph_coded_set_track_device"][1] == [vp, i, i, vp, vp, vp]
    assert S["wc_track_morph_coded_reset"][1] == [vp, i, i, i]
    assert S["wc_track_morph_coded_set_weight"][1] == S["wc_track_morph_coded_set_ratios"][1] == [vp, i, d, d]
    assert S["wc_track_morph_coded_push_device"][1] == [vp, ip, vp, vp, vp, vp, vp, vp, vp, ip]
    assert S["wc_track_morph_coded_flush_device"][1] == [vp, ip, vp, vp, vp, vp, ip]
    for name in ("frames_received", "frames_formed", "pending", "get_delay", "track_length"):
        assert S["wc_track_morph_coded_" + name][1] == [vp, i]
    assert S["wc_track_morph_coded_device_bytes"][1] == [vp]
    L = stream._lib()
    for name, (res, args) in S.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_mirror_class_exists_with_its_parameter_names_and_defaults():
    from world_class_amd.stream import CodedTrackMorph, TrackMorph
    names = lambda f: list(inspect.signature(f).parameters)
    p = inspect.signature(CodedTrackMorph.__init__).parameters
    assert list(p) == ["self", "fs", "fft_size", "number_of_dimensions", "n_streams", "n_tracks", "max_track_frames", "max_frames", "max_delay"]
    assert (p["max_frames"].default, p["max_delay"].default) == (200, 0)
    assert all(v.default is inspect.Parameter.empty for k, v in p.items() if k not in ("max_frames", "max_delay"))
    assert names(CodedTrackMorph.set_track_device) == ["self", "track", "m", "d_f0_b", "d_coded_sp_b", "d_coded_ap_b"]
    assert names(CodedTrackMorph.set_track) == ["self", "track", "f0", "csp", "cap"]
    assert names(CodedTrackMorph.reset) == ["self", "stream", "track", "delay"]
    assert inspect.signature(CodedTrackMorph.reset).parameters["delay"].default == 0
    assert names(CodedTrackMorph.set_weight) == ["self", "stream", "weight", "f0_weight"]
    assert inspect.signature(CodedTrackMorph.set_weight).parameters["f0_weight"].default is None
    assert names(CodedTrackMorph.set_ratios) == ["self", "stream", "ratio_a", "ratio_b"]
    assert names(CodedTrackMorph.push_device) == ["self", "n_a", "d_f0_a", "d_coded_sp_a", "d_coded_ap_a", "d_position_b", "d_f0_out", "d_sp_out", "d_ap_out"]
    assert names(CodedTrackMorph.flush_device) == ["self", "want", "d_tail", "d_f0_out", "d_sp_out", "d_ap_out"]
    assert names(CodedTrackMorph.push) == ["self", "rows", "positions"]
    assert names(CodedTrackMorph.flush) == ["self", "tails", "streams"]
    assert inspect.signature(CodedTrackMorph.flush).parameters["streams"].default is None
    for name in ("frames_received", "frames_formed", "pending", "get_delay"):
        assert names(getattr(CodedTrackMorph, name)) == ["self", "stream"]
    assert names(CodedTrackMorph.track_length) == ["self", "track"]
    assert names(CodedTrackMorph.device_bytes) == ["self"]
    assert names(CodedTrackMorph.close) == ["self"] and hasattr(CodedTrackMorph, "__del__")
    assert not hasattr(TrackMorph, "device_bytes")  # (the full-row class is as it was)


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
