"""CPU tests of the global-variance calls' boundary: include/world_class_gv.h declares exactly the symbols of GV_SIGNATURES with their
arity and types and states the rule, header and translation unit are part of the build, the mirror exists with its parameter names
and defaults, the other tables are untouched, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_gv.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_gv_stats_device": (8, r"int\s+", C.c_int),
    "wc_mlpg_gv_device": (17, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.gv import GV_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = GV_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.gv import GV_SIGNATURES
    assert declared_symbols(HEADER) == sorted(GV_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.gv import GV_SIGNATURES as S
    ip, vp, i, d = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double
    assert S["wc_gv_stats_device"][1] == [i, ip, i, i, vp, vp, vp, vp]
    assert S["wc_mlpg_gv_device"][1] == [i, ip, i, i, i, i, vp, vp, i, vp, vp, vp, d, d, d, i, vp]


def test_the_header_states_its_types_and_the_rule():
    src = _source(HEADER)
    assert re.search(r'#include\s+"world_class_features.h"', src)
    assert re.search(r"wc_gv_stats_device\(int n_utt, const int \*lengths, int nd, int n_ap, const double \*d_static, "
                     r"const unsigned char \*d_mask,\s+double \*d_mean_out, double \*d_var_out\)", src)
    assert re.search(r"wc_mlpg_gv_device\(int n_utt, const int \*lengths, int nd, int n_ap, int orders, int in_format, const void \*d_mean, "
                     r"const void \*d_var,\s+int var_per_frame, const double \*d_gv_mean, const double \*d_gv_var, const unsigned char \*d_mask, "
                     r"double w_ml,\s+double w_gv, double step_init, int max_iter, double \*d_static\)", src)
    whole = open(os.path.join(ROOT, "include", HEADER)).read()
    for word in ("for off = 32, 16, 8, 4, 2, 1 every partial becomes p[l] + p[l ^ off]", "starts at +0.0",
                 "mean = SUM m·c / N,  d(t) = m(t) ? c(t) - mean : 0,  v = SUM d·d / N",
                 "((a2(t-2) * c(t-2) + a1(t-1) * c(t-1)) + a0(t) * c(t)) + (a1(t) * c(t+1) + a2(t) * c(t+2))",
                 "pv = 1.0 / gv_var,  omega = w_ml / (double)(orders * n)", "ratio = sqrt(gv_mean / v)", "c(t) = ratio * d(t) + mean",
                 "J = omega * SUM_t c(t) * (r(t) - 0.5 * Ac(t)) - (0.5 * w_gv) * ((e * e) * pv)",
                 "if J < J_prev: step = step * 0.5;  if J > J_prev: step = step * 1.2",
                 "h(t) = omega * a0(t) + (w_gv * (2.0 / (N * N))) * (((N - 1.0) * pv) * e + (2.0 * pv) * (d(t) * d(t)))",
                 "g(t) = (omega * (r(t) - Ac(t)) - ((w_gv * (2.0 / N)) * (pv * e)) * d(t)) / h(t)", "c(t) = c(t) + step * g(t)",
                 "gv_var == +inf", "N < 2", "is not > 0", "0.0 / 0.0", "unmasked frames are never written", "wc_release_scratch"):
        assert word in whole, word   # the rule stands in the header


def test_the_other_tables_and_headers_are_unchanged():
    import world_class_amd as w
    from world_class_amd.feature_stream import FEATURE_STREAM_SIGNATURES
    from world_class_amd.features import FEATURES_SIGNATURES
    from world_class_amd.gv import GV_SIGNATURES
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    from world_class_amd.warp import WARP_SIGNATURES
    from world_class_amd.warp_stream import WARP_STREAM_SIGNATURES
    assert sorted(FEATURES_SIGNATURES) == ["wc_mlpg_device", "wc_model_feature_width", "wc_pack_model_features_device",
                                           "wc_unpack_model_features_device"]
    assert declared_symbols("world_class_features.h") == sorted(FEATURES_SIGNATURES)
    assert len(WARP_SIGNATURES) == 5 and len(VRESAMPLE_SIGNATURES) == 16 and len(RESAMPLE_SIGNATURES) == 15 and len(STREAM_SIGNATURES) == 46
    assert len(WARP_STREAM_SIGNATURES) == 15 and len(MLPG_STREAM_SIGNATURES) == 11
    others = (set(WARP_SIGNATURES) | set(VRESAMPLE_SIGNATURES) | set(RESAMPLE_SIGNATURES) | set(STREAM_SIGNATURES) | set(WARP_STREAM_SIGNATURES)
              | set(FEATURES_SIGNATURES) | set(MLPG_STREAM_SIGNATURES) | set(FEATURE_STREAM_SIGNATURES) | set(w.EXPORTED_SYMBOLS))
    assert not set(GV_SIGNATURES) & others
    for header in ("world_class_c.h", "world_class_codec.h", "world_class_io.h", "world_class_features.h", "world_class_mlpg_stream.h",
                   "world_class_feature_stream.h"):
        assert not [s for s in declared_symbols(header) if s in GV_SIGNATURES]
    assert "_gv_" not in open(os.path.join(ROOT, "include", "world_class_features.h")).read()


def test_header_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert os.path.join(ROOT, "include", "world_class_features.h") in build.headers()
    assert "wc_gv.hip" in build.sources() and "wc_features.hip" in build.sources()


def test_mirror_exists_with_its_parameter_names_and_defaults():
    from world_class_amd import features, gv
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(gv.stats) == ["lengths", "nd", "n_ap", "d_static", "d_mean_out", "d_var_out", "d_mask"]
    assert sig(gv.mlpg_gv) == ["lengths", "nd", "n_ap", "orders", "d_mean", "d_var", "d_gv_mean", "d_gv_var", "d_static", "d_mask", "var_per_frame",
                               "in_format", "w_ml", "w_gv", "step_init", "max_iter"]
    assert sig(gv.scale) == ["lengths", "nd", "n_ap", "d_gv_mean", "d_gv_var", "d_static", "d_mask"]
    assert sig(gv.stats_host) == ["statics", "nd", "n_ap", "masks"]
    assert sig(gv.mlpg_gv_host) == ["means", "variances", "statics", "gv_mean", "gv_var", "nd", "n_ap", "orders", "masks", "w_ml", "w_gv", "step_init",
                                    "max_iter"]
    assert sig(gv.scale_host) == ["statics", "gv_mean", "gv_var", "nd", "n_ap", "masks"]
    for f in (gv.mlpg_gv, gv.mlpg_gv_host):
        d = inspect.signature(f).parameters
        assert (d["w_ml"].default, d["w_gv"].default, d["step_init"].default, d["max_iter"].default) == (1.0, 1.0, 0.1, 5)
    d = inspect.signature(gv.mlpg_gv).parameters
    assert d["d_mask"].default is None and d["var_per_frame"].default is False and d["in_format"].default == "f64"
    assert gv.FORMATS is features.FORMATS and gv._check is features._check and gv._binder is features._binder


def test_the_rule_is_stated_on_top_of_the_features_rule():
    import features_rule as fr
    import gv_rule as gr
    assert gr.fr is fr
    src = inspect.getsource(gr.mlpg_gv)
    assert "fr.mlpg_system" in src


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert {"wc_mlpg_device", "wc_model_feature_width"} <= exported
