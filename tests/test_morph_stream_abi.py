"""CPU tests of the morph streams' boundary: include/world_class_stream.h declares every wc_morph_stream_* symbol with its arity,
STREAM_SIGNATURES lists them with that arity and their result types, the mirror class exists with its parameter names, the
existing stream signatures are unchanged, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_morph_stream_create": (5, r"wc_morph_stream\s*\*", C.c_void_p),
    "wc_morph_stream_destroy": (1, r"void\s+", None),
    "wc_morph_stream_reset": (2, r"int\s+", C.c_int),
    "wc_morph_stream_set_speeds": (4, r"int\s+", C.c_int),
    "wc_morph_stream_set_weight": (4, r"int\s+", C.c_int),
    "wc_morph_stream_set_ratios": (4, r"int\s+", C.c_int),
    "wc_morph_stream_frames_for_push": (4, r"int\s+", C.c_int),
    "wc_morph_stream_push_device": (13, r"int\s+", C.c_int),
    "wc_morph_stream_push_coded_device": (14, r"int\s+", C.c_int),
    "wc_morph_stream_source_position": (3, r"double\s+", C.c_double),
    "wc_morph_stream_frames_received": (3, r"long long\s+", C.c_longlong),
    "wc_morph_stream_backlog": (3, r"int\s+", C.c_int),
    "wc_morph_stream_frames_formed": (2, r"long long\s+", C.c_longlong),
}


def declared_arity(symbol, result=r"[A-Za-z_ ]+?[\s*]+"):
    src = open(os.path.join(ROOT, "include", "world_class_stream.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*" + result + symbol + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "world_class_stream.h does not declare %s(...) with that result" % symbol
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.stream import STREAM_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result) == arity
    res, args = STREAM_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity
    assert symbol == "wc_morph_stream_create" or args[0] is C.c_void_p  # (the handle)


def test_create_takes_five_ints_and_the_setters_doubles():
    from world_class_amd.stream import STREAM_SIGNATURES as S
    assert S["wc_morph_stream_create"][1] == [C.c_int] * 5
    for name in ("wc_morph_stream_set_speeds", "wc_morph_stream_set_weight", "wc_morph_stream_set_ratios"):
        assert S[name][1] == [C.c_void_p, C.c_int, C.c_double, C.c_double]
    ip = C.POINTER(C.c_int)
    push = S["wc_morph_stream_push_device"][1]
    assert push[1] is ip and push[5] is ip and push[12] is ip and all(a is C.c_void_p for k, a in enumerate(push) if k not in (1, 5, 12))
    coded = S["wc_morph_stream_push_coded_device"][1]
    assert coded[9] is C.c_int and coded[13] is ip


def test_mirror_class_exists_with_its_parameter_names():
    from world_class_amd.stream import MorphStream
    sig = lambda f: list(inspect.signature(f).parameters)
    p = inspect.signature(MorphStream.__init__).parameters
    assert list(p) == ["self", "fs", "fft_size", "n_streams", "max_frames", "max_backlog"]
    assert (p["n_streams"].default, p["max_frames"].default, p["max_backlog"].default) == (1, 200, 16)
    assert sig(MorphStream.push_device) == ["self", "n_a", "d_f0_a", "d_sp_a", "d_ap_a", "n_b", "d_f0_b", "d_sp_b", "d_ap_b", "d_f0_out", "d_sp_out", "d_ap_out"]
    assert sig(MorphStream.push_coded_device) == ["self", "n_a", "d_f0_a", "d_coded_sp_a", "d_coded_ap_a", "n_b", "d_f0_b", "d_coded_sp_b", "d_coded_ap_b",
                                                  "number_of_dimensions", "d_f0_out", "d_sp_out", "d_ap_out"]
    assert sig(MorphStream.push) == ["self", "a", "b"] and sig(MorphStream.push_coded) == ["self", "a", "b"]
    assert sig(MorphStream.set_speeds) == ["self", "stream", "speed_a", "speed_b"]
    assert sig(MorphStream.set_weight) == ["self", "stream", "weight", "f0_weight"]
    assert inspect.signature(MorphStream.set_weight).parameters["f0_weight"].default is None
    assert sig(MorphStream.set_ratios) == ["self", "stream", "ratio_a", "ratio_b"]
    assert sig(MorphStream.reset) == ["self", "stream"] and sig(MorphStream.frames_for_push) == ["self", "stream", "n_a", "n_b"]
    for name in ("source_position", "frames_received", "backlog"):
        assert sig(getattr(MorphStream, name)) == ["self", "stream", "source"]
    assert sig(MorphStream.frames_formed) == ["self", "stream"]


def test_existing_stream_signatures_are_unchanged():
    from world_class_amd.stream import STREAM_SIGNATURES as S, StreamSynthesizer
    ip, vp = C.POINTER(C.c_int), C.c_void_p
    assert S["wc_synth_stream_create"] == (vp, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int])
    assert S["wc_synth_stream_push_device"] == (C.c_int, [vp, ip, ip, vp, vp, vp, vp, ip])
    assert S["wc_synth_stream_push_coded_device"] == (C.c_int, [vp, ip, ip, vp, vp, C.c_int, vp, vp, ip])
    assert S["wc_synth_stream_set_speed"] == (C.c_int, [vp, C.c_int, C.c_double])
    assert S["wc_synth_stream_set_modification"] == (C.c_int, [vp, C.c_int, C.c_double, C.c_double])
    assert S["wc_synth_stream_source_position"] == (C.c_double, [vp, C.c_int])
    assert S["wc_synth_stream_frames_for_push"] == (C.c_int, [vp, C.c_int, C.c_int])
    assert len([n for n in S if not n.startswith("wc_morph_stream_")]) == 33 and len(S) == 33 + len(NEW)
    for symbol, arity in (("wc_synth_stream_create", 5), ("wc_synth_stream_push_device", 8), ("wc_synth_stream_push_coded_device", 9),
                          ("wc_synth_stream_set_speed", 3), ("wc_synth_stream_frames_for_push", 3), ("wc_stream_push_coded_device", 11)):
        assert declared_arity(symbol) == arity
    assert list(inspect.signature(StreamSynthesizer.push_device).parameters) == ["self", "n_frames", "d_f0", "d_sp", "d_ap", "flush", "d_y"]
    assert list(inspect.signature(StreamSynthesizer.set_speed).parameters) == ["self", "stream", "speed"]


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
