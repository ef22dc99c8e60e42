"""CPU tests of the MLPG stream's boundary: include/world_class_mlpg_stream.h declares exactly the symbols of MLPG_STREAM_SIGNATURES
with their arity and types, includes the model features' header and leaves it and its table alone, is part of the build, the mirror
exists with its parameter names, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_mlpg_stream.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_mlpg_stream_emitted": (2, r"long long\s+", C.c_longlong),
    "wc_mlpg_stream_create": (6, r"wc_mlpg_stream\s*\*\s*", C.c_void_p),
    "wc_mlpg_stream_destroy": (1, r"void\s+", None),
    "wc_mlpg_stream_reset": (3, r"int\s+", C.c_int),
    "wc_mlpg_stream_push_device": (8, r"int\s+", C.c_int),
    "wc_mlpg_stream_flush_device": (4, r"int\s+", C.c_int),
    "wc_mlpg_stream_max_frames_per_push": (1, r"int\s+", C.c_int),
    "wc_mlpg_stream_max_frames_per_flush": (1, r"int\s+", C.c_int),
    "wc_mlpg_stream_rows_received": (2, r"long long\s+", C.c_longlong),
    "wc_mlpg_stream_frames_emitted": (2, r"long long\s+", C.c_longlong),
    "wc_mlpg_stream_get_lag": (2, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = MLPG_STREAM_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES
    assert declared_symbols(HEADER) == sorted(MLPG_STREAM_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES as S
    ip, vp, i, ll = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_longlong
    assert S["wc_mlpg_stream_emitted"][1] == [ll, i]
    assert S["wc_mlpg_stream_create"][1] == [i, i, i, i, i, i]
    assert S["wc_mlpg_stream_destroy"][1] == [vp]
    assert S["wc_mlpg_stream_reset"][1] == [vp, i, i]
    assert S["wc_mlpg_stream_push_device"][1] == [vp, ip, i, vp, vp, i, vp, ip]
    assert S["wc_mlpg_stream_flush_device"][1] == [vp, ip, vp, ip]
    for name in ("rows_received", "frames_emitted", "get_lag"):
        assert S["wc_mlpg_stream_" + name][1] == [vp, i]
    assert S["wc_mlpg_stream_max_frames_per_push"][1] == S["wc_mlpg_stream_max_frames_per_flush"][1] == [vp]


def test_the_header_states_its_types_and_includes_the_features():
    src = _source(HEADER)
    assert re.search(r'#include\s+"world_class_features.h"', src)
    assert re.search(r"wc_mlpg_stream_emitted\(long long rows, int lag\)", src)
    assert re.search(r"typedef struct wc_mlpg_stream wc_mlpg_stream;", src)
    assert re.search(r"wc_mlpg_stream_create\(int n_streams, int nd, int n_ap, int orders, int max_rows_per_push, int max_lag\)", src)
    assert re.search(r"wc_mlpg_stream_push_device\(wc_mlpg_stream \*h, const int \*n_rows, int in_format, const void \*d_mean, const void \*d_var,\s+"
                     r"int var_per_frame, double \*d_static, int \*frames_out\)", src)
    assert re.search(r"wc_mlpg_stream_flush_device\(wc_mlpg_stream \*h, const int \*want, double \*d_static, int \*frames_out\)", src)
    whole = open(os.path.join(ROOT, "include", HEADER)).read()
    for word in ("E(T) = max(T - L, 0)", "bit for bit", "A wanted stream with no rows", "Why bounded state suffices", "A reset forgets everything"):
        assert word in whole   # the rule stands in the header


def test_the_features_header_and_its_table_are_unchanged():
    from world_class_amd.features import FEATURES_SIGNATURES
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES
    assert sorted(FEATURES_SIGNATURES) == ["wc_mlpg_device", "wc_model_feature_width", "wc_pack_model_features_device",
                                           "wc_unpack_model_features_device"]
    assert not set(MLPG_STREAM_SIGNATURES) & set(FEATURES_SIGNATURES)
    assert declared_symbols("world_class_features.h") == sorted(FEATURES_SIGNATURES)
    assert "wc_mlpg_stream" not in open(os.path.join(ROOT, "include", "world_class_features.h")).read()


def test_header_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert os.path.join(ROOT, "include", "world_class_features.h") in build.headers()
    assert "wc_mlpg_stream.hip" in build.sources() and "wc_features.hip" in build.sources()
    assert os.path.join(ROOT, "world_class_amd", "csrc", "wc_lag_stream.hpp") in build.headers()


def test_mirror_exists_with_its_parameter_names():
    from world_class_amd import features, mlpg_stream as m
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(m.emitted) == ["rows", "lag"]
    assert sig(m.MlpgStream.__init__) == ["self", "n_streams", "nd", "n_ap", "orders", "max_rows_per_push", "max_lag"]
    assert sig(m.MlpgStream.reset) == ["self", "stream", "lag"]
    assert sig(m.MlpgStream.push_device) == ["self", "n_rows", "d_mean", "d_var", "d_static", "var_per_frame", "in_format"]
    assert sig(m.MlpgStream.flush_device) == ["self", "want", "d_static"]
    for name in ("rows_received", "frames_emitted", "get_lag"):
        assert sig(getattr(m.MlpgStream, name)) == ["self", "stream"]
    assert sig(m.MlpgStream.close) == ["self"]
    defaults = inspect.signature(m.MlpgStream.push_device).parameters
    assert defaults["var_per_frame"].default is False and defaults["in_format"].default == "f64"
    assert m.FORMATS is features.FORMATS and m._check is features._check and m._ints is features._ints and m._opt is features._opt


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
