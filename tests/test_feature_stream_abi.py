"""CPU tests of the feature stream's boundary: include/world_class_feature_stream.h declares exactly the symbols of
FEATURE_STREAM_SIGNATURES with their arity and types, includes the model features' header and leaves it, the MLPG stream's header
and their tables alone, states the rule, is part of the build, the mirror exists with its parameter names, and the tree compiles
for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_feature_stream.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_feature_stream_emitted": (2, r"long long\s+", C.c_longlong),
    "wc_feature_stream_create": (6, r"wc_feature_stream\s*\*\s*", C.c_void_p),
    "wc_feature_stream_destroy": (1, r"void\s+", None),
    "wc_feature_stream_reset": (4, r"int\s+", C.c_int),
    "wc_feature_stream_push_device": (8, r"int\s+", C.c_int),
    "wc_feature_stream_flush_device": (5, r"int\s+", C.c_int),
    "wc_feature_stream_max_frames_per_push": (1, r"int\s+", C.c_int),
    "wc_feature_stream_max_frames_per_flush": (1, r"int\s+", C.c_int),
    "wc_feature_stream_rows_received": (2, r"long long\s+", C.c_longlong),
    "wc_feature_stream_frames_emitted": (2, r"long long\s+", C.c_longlong),
    "wc_feature_stream_get_lag": (2, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.feature_stream import FEATURE_STREAM_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = FEATURE_STREAM_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.feature_stream import FEATURE_STREAM_SIGNATURES
    assert declared_symbols(HEADER) == sorted(FEATURE_STREAM_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.feature_stream import FEATURE_STREAM_SIGNATURES as S
    ip, vp, i, ll, d = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_longlong, C.c_double
    assert S["wc_feature_stream_emitted"][1] == [ll, i]
    assert S["wc_feature_stream_create"][1] == [i, i, i, i, i, i]
    assert S["wc_feature_stream_destroy"][1] == [vp]
    assert S["wc_feature_stream_reset"][1] == [vp, i, i, d]
    assert S["wc_feature_stream_push_device"][1] == [vp, ip, vp, vp, vp, i, vp, ip]
    assert S["wc_feature_stream_flush_device"][1] == [vp, ip, i, vp, ip]
    for name in ("rows_received", "frames_emitted", "get_lag"):
        assert S["wc_feature_stream_" + name][1] == [vp, i]
    assert S["wc_feature_stream_max_frames_per_push"][1] == S["wc_feature_stream_max_frames_per_flush"][1] == [vp]


def test_the_header_states_its_types_the_rule_and_includes_the_features():
    src = _source(HEADER)
    assert re.search(r'#include\s+"world_class_features.h"', src)
    assert re.search(r"wc_feature_stream_emitted\(long long rows, int lag\)", src)
    assert re.search(r"typedef struct wc_feature_stream wc_feature_stream;", src)
    assert re.search(r"wc_feature_stream_create\(int n_streams, int nd, int n_ap, int orders, int max_rows_per_push, int max_lag\)", src)
    assert re.search(r"wc_feature_stream_reset\(wc_feature_stream \*h, int stream, int lag, double lf0_fill\)", src)
    assert re.search(r"wc_feature_stream_push_device\(wc_feature_stream \*h, const int \*n_rows, const double \*d_f0, const double \*d_coded_sp,\s+"
                     r"const double \*d_coded_ap, int out_format, void \*d_rows, int \*frames_out\)", src)
    assert re.search(r"wc_feature_stream_flush_device\(wc_feature_stream \*h, const int \*want, int out_format, void \*d_rows, int \*frames_out\)", src)
    whole = " ".join(open(os.path.join(ROOT, "include", HEADER)).read().replace(" * ", " ").split())
    for word in ("E(T) = max(T - L, 0)", "Pushed row i with i >= L emits row i - L of P_i", "bit for bit", "A wanted stream with no rows",
                 "Why bounded state suffices", "A reset forgets everything", "do not depend on how its rows are cut into pushes",
                 "No stream's outputs depend on another stream", "holds the last voiced log-F0", "With L >= n nothing is emitted before the flush",
                 "its successor counts as 0.0", "whose unvoiced runs are all shorter than L", "a longer run costs a step in log-F0",
                 "the step falls at that frame", "the deltas of its own prefix", "L = 64 covers pauses of 315 ms",
                 "exactly max_lag + max_rows_per_push + 1 rows"):
        assert word in whole, word   # the rule stands in the header
    for point in range(1, 9):
        assert re.search(r"^ \*   %d\. " % point, open(os.path.join(ROOT, "include", HEADER)).read(), re.M), point


def test_the_other_headers_and_their_tables_are_unchanged():
    from world_class_amd.feature_stream import FEATURE_STREAM_SIGNATURES
    from world_class_amd.features import FEATURES_SIGNATURES
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES
    assert sorted(FEATURES_SIGNATURES) == ["wc_mlpg_device", "wc_model_feature_width", "wc_pack_model_features_device",
                                           "wc_unpack_model_features_device"]
    assert len(MLPG_STREAM_SIGNATURES) == 11 and all(s.startswith("wc_mlpg_stream_") for s in MLPG_STREAM_SIGNATURES)
    assert not set(FEATURE_STREAM_SIGNATURES) & (set(FEATURES_SIGNATURES) | set(MLPG_STREAM_SIGNATURES))
    assert declared_symbols("world_class_features.h") == sorted(FEATURES_SIGNATURES)
    assert declared_symbols("world_class_mlpg_stream.h") == sorted(MLPG_STREAM_SIGNATURES)
    for other in ("world_class_features.h", "world_class_mlpg_stream.h"):
        assert "wc_feature_stream" not in open(os.path.join(ROOT, "include", other)).read()


def test_header_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    for header in (HEADER, "world_class_features.h", "world_class_mlpg_stream.h"):
        assert os.path.join(ROOT, "include", header) in build.headers()
    assert "wc_feature_stream.hip" in build.sources() and "wc_features.hip" in build.sources()
    # what the translation units of the model features share is stated once
    shared = open(os.path.join(ROOT, "world_class_amd", "csrc", "wc_features_rows.hpp")).read()
    assert "ft_voiced(double f)" in shared and "ft_column(int c" in shared
    for unit in ("wc_features.hip", "wc_feature_stream.hip"):
        src = open(os.path.join(ROOT, "world_class_amd", "csrc", unit)).read()
        assert '#include "wc_features_rows.hpp"' in src and "bool ft_voiced(" not in src and "void ft_column(" not in src
    # and so is the lagged ledger of the two streams: neither unit defines emitted_of itself
    assert os.path.join(ROOT, "world_class_amd", "csrc", "wc_lag_stream.hpp") in build.headers()
    assert "long long emitted_of(long long rows, int lag)" in open(os.path.join(ROOT, "world_class_amd", "csrc", "wc_lag_stream.hpp")).read()
    for unit in ("wc_mlpg_stream.hip", "wc_feature_stream.hip"):
        src = open(os.path.join(ROOT, "world_class_amd", "csrc", unit)).read()
        assert '#include "wc_lag_stream.hpp"' in src and "long long emitted_of(" not in src


def test_mirror_exists_with_its_parameter_names():
    from world_class_amd import feature_stream as m, features
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(m.emitted) == ["rows", "lag"]
    assert sig(m.FeatureStream.__init__) == ["self", "n_streams", "nd", "n_ap", "orders", "max_rows_per_push", "max_lag"]
    assert sig(m.FeatureStream.reset) == ["self", "stream", "lag", "lf0_fill"]
    assert sig(m.FeatureStream.push_device) == ["self", "n_rows", "d_f0", "d_coded_sp", "d_coded_ap", "d_rows", "out_format"]
    assert sig(m.FeatureStream.flush_device) == ["self", "want", "d_rows", "out_format"]
    for name in ("rows_received", "frames_emitted", "get_lag"):
        assert sig(getattr(m.FeatureStream, name)) == ["self", "stream"]
    assert sig(m.FeatureStream.close) == ["self"]
    assert inspect.signature(m.FeatureStream.push_device).parameters["out_format"].default == "f64"
    assert inspect.signature(m.FeatureStream.flush_device).parameters["out_format"].default == "f64"
    assert inspect.signature(m.FeatureStream.reset).parameters["lf0_fill"].default == 0.0
    assert m.FORMATS is features.FORMATS and m._check is features._check and m._ints is features._ints and m._opt is features._opt


def test_the_entry_checks_the_new_table():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "FEATURE_STREAM_SIGNATURES" in src and "MLPG_STREAM_SIGNATURES" in src


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
