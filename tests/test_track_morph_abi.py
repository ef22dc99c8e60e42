"""CPU tests of the track-morph streams' boundary: include/world_class_track_morph.h (which world_class_stream.h includes at its
bottom, below world_class_align_lag.h) declares exactly the wc_track_morph_* calls with their arities and results,
TRACK_MORPH_SIGNATURES lists them with that arity and their result types, is bound with the other four tables and shares no symbol
with them (whose sizes stay 46, 7, 2 and 5), the mirror class exists with its parameter names, and the tree compiles for gfx950
without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "world_class_track_morph.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_track_morph_create": (7, r"wc_track_morph\s*\*", C.c_void_p),
    "wc_track_morph_destroy": (1, r"void\s+", None),
    "wc_track_morph_set_track_device": (6, r"int\s+", C.c_int),
    "wc_track_morph_reset": (4, r"int\s+", C.c_int),
    "wc_track_morph_set_weight": (4, r"int\s+", C.c_int),
    "wc_track_morph_set_ratios": (4, r"int\s+", C.c_int),
    "wc_track_morph_push_device": (10, r"int\s+", C.c_int),
    "wc_track_morph_flush_device": (7, r"int\s+", C.c_int),
    "wc_track_morph_frames_received": (2, r"long long\s+", C.c_longlong),
    "wc_track_morph_frames_formed": (2, r"long long\s+", C.c_longlong),
    "wc_track_morph_pending": (2, r"int\s+", C.c_int),
    "wc_track_morph_get_delay": (2, r"int\s+", C.c_int),
    "wc_track_morph_track_length": (2, r"int\s+", C.c_int),
}


def _source(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_arity(symbol, result, header=HEADER):
    m = re.search(r"^\s*" + result + symbol + r"\s*\(([^)]*)\)\s*;", _source(header), flags=re.M)
    assert m, "%s does not declare %s(...) with that result" % (header, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.stream import TRACK_MORPH_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result) == arity
    res, args = TRACK_MORPH_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity
    assert symbol == "wc_track_morph_create" or args[0] is C.c_void_p  # (the handle)


def test_the_table_is_the_header_and_disjoint_from_the_other_four():
    from world_class_amd.stream import (ALIGN_LAG_SIGNATURES, ALIGN_STREAM_SIGNATURES, ALIGN_WINDOW_SIGNATURES, STREAM_SIGNATURES,
                                        TRACK_MORPH_SIGNATURES)
    declared = sorted(set(re.findall(r"\b(wc_[a-z0-9_]+)\s*\(", _source(HEADER))))
    assert declared == sorted(TRACK_MORPH_SIGNATURES) == sorted(NEW)
    others = set(STREAM_SIGNATURES) | set(ALIGN_STREAM_SIGNATURES) | set(ALIGN_WINDOW_SIGNATURES) | set(ALIGN_LAG_SIGNATURES)
    assert not set(TRACK_MORPH_SIGNATURES) & others
    assert (len(STREAM_SIGNATURES), len(ALIGN_STREAM_SIGNATURES), len(ALIGN_WINDOW_SIGNATURES), len(ALIGN_LAG_SIGNATURES)) == (46, 7, 2, 5)


def test_existing_signatures_are_unchanged():
    from world_class_amd.stream import ALIGN_LAG_SIGNATURES as A, STREAM_SIGNATURES as S
    ip, vp = C.POINTER(C.c_int), C.c_void_p
    assert S["wc_morph_stream_create"] == (vp, [C.c_int] * 5)
    assert S["wc_morph_stream_push_device"] == (C.c_int, [vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, ip])
    assert S["wc_morph_stream_set_weight"] == (C.c_int, [vp, C.c_int, C.c_double, C.c_double])
    assert S["wc_synth_stream_push_device"] == (C.c_int, [vp, ip, ip, vp, vp, vp, vp, ip])
    assert A["wc_align_stream_push_settled_device"] == (C.c_int, [vp, ip, vp, vp, vp, vp])
    assert A["wc_align_stream_tail_device"] == (C.c_int, [vp, ip, vp])


def test_the_stream_header_includes_it_at_the_bottom():
    lines = [l.strip() for l in _source("world_class_stream.h").splitlines() if l.strip().startswith("#include")]
    assert lines[-1] == '#include "%s"' % HEADER and lines[-2] == '#include "world_class_align_lag.h"'
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()


def test_argument_types_and_binding():
    from world_class_amd import stream
    ip, vp, i, d = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double
    S = stream.TRACK_MORPH_SIGNATURES
    assert S["wc_track_morph_create"][1] == [i] * 7
    assert S["wc_track_morph_set_track_device"][1] == [vp, i, i, vp, vp, vp]
    assert S["wc_track_morph_reset"][1] == [vp, i, i, i]
    assert S["wc_track_morph_set_weight"][1] == S["wc_track_morph_set_ratios"][1] == [vp, i, d, d]
    assert S["wc_track_morph_push_device"][1] == [vp, ip, vp, vp, vp, vp, vp, vp, vp, ip]
    assert S["wc_track_morph_flush_device"][1] == [vp, ip, vp, vp, vp, vp, ip]
    for name in ("frames_received", "frames_formed", "pending", "get_delay", "track_length"):
        assert S["wc_track_morph_" + name][1] == [vp, i]
    L = stream._lib()
    for name, (res, args) in S.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_mirror_class_exists_with_its_parameter_names():
    from world_class_amd.stream import TrackMorph
    names = lambda f: list(inspect.signature(f).parameters)
    p = inspect.signature(TrackMorph.__init__).parameters
    assert list(p) == ["self", "fs", "fft_size", "n_streams", "n_tracks", "max_track_frames", "max_frames", "max_delay"]
    assert (p["max_frames"].default, p["max_delay"].default) == (200, 0)
    assert names(TrackMorph.set_track_device) == ["self", "track", "m", "d_f0_b", "d_sp_b", "d_ap_b"]
    assert names(TrackMorph.set_track) == ["self", "track", "f0", "sp", "ap"]
    assert names(TrackMorph.reset) == ["self", "stream", "track", "delay"]
    assert inspect.signature(TrackMorph.reset).parameters["delay"].default == 0
    assert names(TrackMorph.set_weight) == ["self", "stream", "weight", "f0_weight"]
    assert inspect.signature(TrackMorph.set_weight).parameters["f0_weight"].default is None
    assert names(TrackMorph.set_ratios) == ["self", "stream", "ratio_a", "ratio_b"]
    assert names(TrackMorph.push_device) == ["self", "n_a", "d_f0_a", "d_sp_a", "d_ap_a", "d_position_b", "d_f0_out", "d_sp_out", "d_ap_out"]
    assert names(TrackMorph.flush_device) == ["self", "want", "d_tail", "d_f0_out", "d_sp_out", "d_ap_out"]
    assert names(TrackMorph.push) == ["self", "rows", "positions"]
    assert names(TrackMorph.flush) == ["self", "tails", "streams"]
    assert inspect.signature(TrackMorph.flush).parameters["streams"].default is None
    for name in ("frames_received", "frames_formed", "pending", "get_delay"):
        assert names(getattr(TrackMorph, name)) == ["self", "stream"]
    assert names(TrackMorph.track_length) == ["self", "track"]
    assert names(TrackMorph.close) == ["self"] and hasattr(TrackMorph, "__del__")


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
