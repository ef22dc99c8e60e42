"""CPU tests of the model features' boundary: include/world_class_features.h declares exactly the symbols of FEATURES_SIGNATURES
with their arity and types, header and translation unit are part of the build, the mirror exists with its parameter names, the other
tables are untouched, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_features.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_model_feature_width": (3, r"int\s+", C.c_int),
    "wc_pack_model_features_device": (11, r"int\s+", C.c_int),
    "wc_mlpg_device": (10, r"int\s+", C.c_int),
    "wc_unpack_model_features_device": (10, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.features import FEATURES_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = FEATURES_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.features import FEATURES_SIGNATURES
    assert declared_symbols(HEADER) == sorted(FEATURES_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.features import FEATURES_SIGNATURES as S
    ip, vp, i, d, ll = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double, C.c_longlong
    assert S["wc_model_feature_width"][1] == [i, i, i]
    assert S["wc_pack_model_features_device"][1] == [i, ip, i, i, i, vp, vp, vp, d, i, vp]
    assert S["wc_mlpg_device"][1] == [i, ip, i, i, i, i, vp, vp, i, vp]
    assert S["wc_unpack_model_features_device"][1] == [ll, i, i, i, i, vp, d, vp, vp, vp]


def test_the_header_states_its_types_formats_and_rule():
    src = _source(HEADER)
    assert re.search(r"wc_model_feature_width\(int nd, int n_ap, int orders\)", src)
    assert re.search(r"wc_pack_model_features_device\(int n_utt, const int \*lengths, int nd, int n_ap, int orders, const double \*d_f0,\s+"
                     r"const double \*d_coded_sp, const double \*d_coded_ap, double lf0_fill, int out_format, void \*d_rows\)", src)
    assert re.search(r"wc_mlpg_device\(int n_utt, const int \*lengths, int nd, int n_ap, int orders, int in_format, const void \*d_mean, "
                     r"const void \*d_var,\s+int var_per_frame, double \*d_static\)", src)
    assert re.search(r"wc_unpack_model_features_device\(long long n_frames, int nd, int n_ap, int orders, int in_format, const void \*d_rows,\s+"
                     r"double vuv_threshold, double \*d_f0, double \*d_coded_sp, double \*d_coded_ap\)", src)
    assert re.search(r"#define\s+WC_FEAT_F64\s+0", src) and re.search(r"#define\s+WC_FEAT_F32\s+1", src)
    whole = open(os.path.join(ROOT, "include", HEADER)).read()
    for word in ("(1 - a) * l(L) + a * l(R)", "0.5 * (x(t+1) - x(t-1))", "(x(t-1) + x(t+1)) - 2.0 * x(t)", "l2(t) = a2(t-2) / d(t-2)",
                 "(a1(t-1) - (l2(t) * d(t-2)) * l1(t-1)) / d(t-1)", "(z(t) / d(t) - l1(t+1) * c(t+1)) - l2(t+2) * c(t+2)", "wc_release_scratch"):
        assert word in whole   # the rule stands in the header


def test_formats_and_width_agree_with_the_rule():
    import features_rule as fr
    from world_class_amd import features as ft
    assert ft.FORMATS["f64"][0] == 0 and ft.FORMATS["f32"][0] == 1
    for nd, n_ap, orders in [(25, 1, 3), (60, 5, 2), (24, 0, 1)]:
        assert fr.width(nd, n_ap, orders) == orders * (nd + 1 + n_ap) + 1


def test_the_other_tables_and_headers_are_unchanged():
    import world_class_amd as w
    from world_class_amd.features import FEATURES_SIGNATURES
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    from world_class_amd.warp import WARP_SIGNATURES
    from world_class_amd.warp_stream import WARP_STREAM_SIGNATURES
    assert len(WARP_SIGNATURES) == 5 and len(VRESAMPLE_SIGNATURES) == 16 and len(RESAMPLE_SIGNATURES) == 15 and len(STREAM_SIGNATURES) == 46
    assert len(WARP_STREAM_SIGNATURES) == 15
    others = set(WARP_SIGNATURES) | set(VRESAMPLE_SIGNATURES) | set(RESAMPLE_SIGNATURES) | set(STREAM_SIGNATURES) | set(WARP_STREAM_SIGNATURES) | set(w.EXPORTED_SYMBOLS)
    assert not set(FEATURES_SIGNATURES) & others
    for header in ("world_class_c.h", "world_class_codec.h", "world_class_io.h"):
        assert not [s for s in declared_symbols(header) if s in FEATURES_SIGNATURES]


def test_header_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert "wc_features.hip" in build.sources()


def test_mirror_exists_with_its_parameter_names():
    from world_class_amd import features as ft
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(ft.width) == ["nd", "n_ap", "orders"]
    assert sig(ft.pack) == ["lengths", "nd", "n_ap", "orders", "d_f0", "d_coded_sp", "d_coded_ap", "d_rows", "lf0_fill", "out_format"]
    assert sig(ft.mlpg) == ["lengths", "nd", "n_ap", "orders", "d_mean", "d_var", "d_static", "var_per_frame", "in_format"]
    assert sig(ft.unpack) == ["n_frames", "nd", "n_ap", "orders", "d_rows", "d_f0", "d_coded_sp", "d_coded_ap", "vuv_threshold", "in_format"]
    assert sig(ft.pack_host) == ["f0s", "coded_sps", "coded_aps", "orders", "lf0_fill", "out_format"]
    assert sig(ft.mlpg_host) == ["means", "variances", "nd", "n_ap", "orders"]
    assert sig(ft.unpack_host) == ["rows", "nd", "n_ap", "orders", "vuv_threshold"]
    assert inspect.signature(ft.pack).parameters["out_format"].default == "f64"
    assert inspect.signature(ft.unpack).parameters["vuv_threshold"].default == 0.5


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported


def test_width_needs_no_device():
    """wc_model_feature_width is a pure host function: the row width, -1 for what the other calls refuse"""
    from world_class_amd import build
    L = C.CDLL(build.build())
    f = L.wc_model_feature_width
    f.restype, f.argtypes = C.c_int, [C.c_int] * 3
    assert f(25, 1, 3) == 82 and f(60, 5, 3) == 199 and f(24, 0, 1) == 26 and f(1, 0, 2) == 5
    assert f(0, 1, 3) == -1 and f(25, -1, 3) == -1 and f(25, 1, 0) == -1 and f(25, 1, 4) == -1
    assert f(2 ** 30, 0, 3) == -1   # a width beyond 31 bits
