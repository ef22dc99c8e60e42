"""CPU tests of the boundary of the synthesis streams' speed setting: include/world_class_stream.h declares
wc_synth_stream_set_speed, wc_synth_stream_source_position, wc_synth_stream_frames_synthesised and wc_synth_stream_frames_for_push
with 3, 2, 2 and 3 arguments, STREAM_SIGNATURES lists them with that arity and their result types, the mirror methods exist with
their parameter names, the existing signatures are unchanged, and the tree compiles for gfx950 without a GPU and exports the four
symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wc_synth_stream_set_speed": ("int", 3, C.c_int), "wc_synth_stream_source_position": ("double", 2, C.c_double),
       "wc_synth_stream_frames_synthesised": (r"long\s+long", 2, C.c_longlong), "wc_synth_stream_frames_for_push": ("int", 3, C.c_int)}


def declared_arity(symbol, result):
    src = open(os.path.join(ROOT, "include", "world_class_stream.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + result + r"\s+" + symbol + r"\s*\(([^)]*)\)\s*;", src)
    assert m, "world_class_stream.h does not declare %s %s(...)" % (result, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity(symbol):
    from world_class_amd.stream import STREAM_SIGNATURES
    result, arity, ctype = NEW[symbol]
    assert declared_arity(symbol, result) == arity
    res, args = STREAM_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity
    assert args[0] is C.c_void_p and args[1] is C.c_int
    assert args[2:] == {"wc_synth_stream_set_speed": [C.c_double], "wc_synth_stream_frames_for_push": [C.c_int]}.get(symbol, [])


def test_mirror_methods_exist_with_their_parameter_names():
    from world_class_amd.stream import StreamSynthesizer
    assert list(inspect.signature(StreamSynthesizer.set_speed).parameters) == ["self", "stream", "speed"]
    assert list(inspect.signature(StreamSynthesizer.source_position).parameters) == ["self", "stream"]
    assert list(inspect.signature(StreamSynthesizer.frames_synthesised).parameters) == ["self", "stream"]
    assert list(inspect.signature(StreamSynthesizer.frames_for_push).parameters) == ["self", "stream", "n_frames"]


def test_existing_signatures_are_unchanged():
    from world_class_amd.stream import STREAM_SIGNATURES, StreamSynthesizer
    assert list(inspect.signature(StreamSynthesizer.push_device).parameters) == ["self", "n_frames", "d_f0", "d_sp", "d_ap", "flush", "d_y"]
    assert list(inspect.signature(StreamSynthesizer.push_coded_device).parameters) == [
        "self", "n_frames", "d_f0", "d_coded_sp", "number_of_dimensions", "d_coded_ap", "flush", "d_y"]
    p = inspect.signature(StreamSynthesizer.set_modification).parameters
    assert list(p) == ["self", "stream", "f0_scale", "spectral_ratio"] and p["f0_scale"].default == 1.0 and p["spectral_ratio"].default == 0.0
    for symbol, arity in (("wc_synth_stream_push_device", 8), ("wc_synth_stream_push_coded_device", 9), ("wc_synth_stream_set_modification", 4),
                          ("wc_synth_stream_frames_received", 2)):
        assert declared_arity(symbol, r"(?:int|long\s+long)") == arity
        assert len(STREAM_SIGNATURES[symbol][1]) == arity


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
