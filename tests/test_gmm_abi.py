"""CPU tests of the GMM conversion's boundary: include/world_class_gmm.h declares exactly the symbols of GMM_SIGNATURES with their
arity and types and states the rule, header and translation unit are part of the build, the mirror exists with its parameter names
and defaults, the other tables are untouched, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_gmm.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_gmm_create": (6, r"wc_gmm\s*\*\s*", C.c_void_p),
    "wc_gmm_destroy": (1, r"void\s+", None),
    "wc_gmm_prepared_host": (5, r"int\s+", C.c_int),
    "wc_gmm_convert_device": (13, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.gmm import GMM_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = GMM_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.gmm import GMM_SIGNATURES
    assert declared_symbols(HEADER) == sorted(GMM_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.gmm import GMM_SIGNATURES as S
    dp, vp, i, ll = C.POINTER(C.c_double), C.c_void_p, C.c_int, C.c_longlong
    assert S["wc_gmm_create"][1] == [i, i, i, dp, dp, dp]
    assert S["wc_gmm_destroy"][1] == [vp]
    assert S["wc_gmm_prepared_host"][1] == [vp, dp, dp, dp, dp]
    assert S["wc_gmm_convert_device"][1] == [vp, ll, i, vp, i, i, i, vp, vp, i, i, vp, vp]


def test_the_header_states_its_types_and_the_rule():
    src = _source(HEADER)
    assert re.search(r'#include\s+"world_class_features.h"', src)
    assert re.search(r"typedef struct wc_gmm wc_gmm;", src)
    assert re.search(r"wc_gmm \*wc_gmm_create\(int n_mix, int dx, int dy, const double \*h_weight, const double \*h_mean, const double \*h_cov\)", src)
    assert re.search(r"int wc_gmm_prepared_host\(const wc_gmm \*g, double \*h_c, double \*h_W, double \*h_B, double \*h_cvar\)", src)
    assert re.search(r"int wc_gmm_convert_device\(const wc_gmm \*g, long long n_frames,\s+int in_format, const void \*d_rows_in, int ld_in, int col_in,"
                     r"\s+int out_format, void \*d_mean, void \*d_var, int ld_out, int col_out,\s+int \*d_best, double \*d_loglik\)", src)
    whole = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", HEADER)).read())   # (the comment's lines joined)
    for word in ("Every operation is in double, rounded on its own, with no fma",
                 "s = Sxx(i,j), then s = s - L(i,k) * L(j,k) for k = 0..j-1 ascending", "L(i,j) = s / L(j,j) for j < i, and L(i,i) = sqrt(s)",
                 "W(j,j) = 1.0 / L(j,j)", "s = L(i,j) * W(j,j), then s = s + L(i,k) * W(k,j) for k = j+1..i-1 ascending, and W(i,j) = -s / L(i,i)",
                 "B(j,k) is the sum of Syx(j,i) * W(k,i) over i = 0..k, ascending", "The sum starts at its first product",
                 "s = Syy(j,j), then s = s - B(j,k) * B(j,k) for k ascending",
                 "c = (log(w) - ld) - (0.5 * (double)dx) * 1.8378770664093453", "ld = ld + log L(i,i) ascending", "log is the C library's",
                 "A float input is widened exactly", "A float output is the (float) of the double", "d(k) = x(k) - mux_m(k)",
                 "z(i) is the sum of W_m(i,k) * d(k) over k = 0..i, ascending, starting at its first product",
                 "q is the sum of z(i) * z(i) over i, ascending, in the same form", "ll(m) = c_m - 0.5 * q",
                 "best is the least m whose ll(m) is not NaN and is >= every other ll that is not NaN",
                 "mean(j) = muy_best(j) + s, where s is the sum of B_best(j,k) * z_best(k) over k ascending", "var(j) = cvar_best(j)",
                 "best = -1, mean(j) = 0.0, var(j) = +inf", "Every loop is bounded by n_mix, dx and dy", "never depends on the launch shape",
                 "only the lower triangle (column <= row) is read", "n_mix outside 1..1024", "dx or dy outside 1..192",
                 "the text names the mixture and the row", "Weights need not sum to 1", "n_frames < 0 or > 2^32 - 1", "ld_in < col_in + dx",
                 "ld_out < col_out + dy", "all four outputs NULL", "any output overlapping the input or another output",
                 "n_frames == 0 writes nothing", "wc_release_scratch", "Several host threads", "wc_set_stream"):
        assert word.lower() in whole.lower(), word   # the rule stands in the header


def test_the_other_tables_and_headers_are_unchanged():
    import world_class_amd as w
    from world_class_amd.feature_stream import FEATURE_STREAM_SIGNATURES
    from world_class_amd.features import FEATURES_SIGNATURES
    from world_class_amd.gmm import GMM_SIGNATURES
    from world_class_amd.gv import GV_SIGNATURES
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    from world_class_amd.warp import WARP_SIGNATURES
    from world_class_amd.warp_stream import WARP_STREAM_SIGNATURES
    assert sorted(FEATURES_SIGNATURES) == ["wc_mlpg_device", "wc_model_feature_width", "wc_pack_model_features_device",
                                           "wc_unpack_model_features_device"]
    assert sorted(GV_SIGNATURES) == ["wc_gv_stats_device", "wc_mlpg_gv_device"]
    assert declared_symbols("world_class_features.h") == sorted(FEATURES_SIGNATURES)
    assert declared_symbols("world_class_gv.h") == sorted(GV_SIGNATURES)
    assert len(WARP_SIGNATURES) == 5 and len(VRESAMPLE_SIGNATURES) == 16 and len(RESAMPLE_SIGNATURES) == 15 and len(STREAM_SIGNATURES) == 46
    assert len(WARP_STREAM_SIGNATURES) == 15 and len(MLPG_STREAM_SIGNATURES) == 11
    others = (set(WARP_SIGNATURES) | set(VRESAMPLE_SIGNATURES) | set(RESAMPLE_SIGNATURES) | set(STREAM_SIGNATURES) | set(WARP_STREAM_SIGNATURES)
              | set(FEATURES_SIGNATURES) | set(MLPG_STREAM_SIGNATURES) | set(FEATURE_STREAM_SIGNATURES) | set(GV_SIGNATURES)
              | set(w.EXPORTED_SYMBOLS))
    assert not set(GMM_SIGNATURES) & others
    for header in ("world_class_c.h", "world_class_codec.h", "world_class_io.h", "world_class_features.h", "world_class_mlpg_stream.h",
                   "world_class_feature_stream.h", "world_class_gv.h"):
        assert not [s for s in declared_symbols(header) if s in GMM_SIGNATURES]
    for header in ("world_class_features.h", "world_class_gv.h"):
        assert "_gmm_" not in open(os.path.join(ROOT, "include", header)).read()


def test_header_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert os.path.join(ROOT, "include", "world_class_features.h") in build.headers()
    assert os.path.join(ROOT, "world_class_amd", "csrc", "wc_gmm_plan.hpp") in build.headers()
    assert "wc_gmm.hip" in build.sources() and "wc_features.hip" in build.sources() and "wc_gv.hip" in build.sources()


def test_the_entry_point_loads_the_table():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "wgmm.GMM_SIGNATURES" in src and "from world_class_amd import gmm as wgmm" in src


def test_mirror_exists_with_its_parameter_names_and_defaults():
    from world_class_amd import features, gmm
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(gmm.Gmm.__init__) == ["self", "weight", "mean", "cov", "dx"]
    assert sig(gmm.Gmm.convert) == ["self", "n_frames", "d_rows_in", "ld_in", "d_mean", "d_var", "ld_out", "col_in", "col_out", "d_best", "d_loglik",
                                    "in_format", "out_format"]
    assert sig(gmm.Gmm.convert_host) == ["self", "rows", "col_in", "out_format"]
    assert sig(gmm.Gmm.prepared) == ["self"] and sig(gmm.Gmm.close) == ["self"]
    assert sig(gmm.joint_from_blocks) == ["mux", "muy", "sxx", "syx", "syy"]
    d = inspect.signature(gmm.Gmm.convert).parameters
    assert (d["col_in"].default, d["col_out"].default, d["d_best"].default, d["d_loglik"].default) == (0, 0, None, None)
    assert d["in_format"].default == "f64" and d["out_format"].default == "f64"
    assert gmm.FORMATS is features.FORMATS and gmm._check is features._check and gmm._binder is features._binder


def test_joint_from_blocks_assembles_what_the_rule_reads():
    import gmm_rule as gm
    from test_gmm_rule import random_model
    from world_class_amd import gmm
    weight, mean, cov, _ = random_model(3, 4, 2, 11)
    m2, c2 = gmm.joint_from_blocks(mean[:, :4], mean[:, 4:], cov[:, :4, :4], cov[:, 4:, :4], cov[:, 4:, 4:])
    assert np.array_equal(m2, mean) and np.array_equal(c2, cov)
    m3, c3 = gmm.joint_from_blocks(mean[:, :4], mean[:, 4:], cov[:, :4, :4], cov[:, 4:, :4], np.stack([np.diag(c) for c in cov[:, 4:, 4:]]))
    assert np.array_equal(m3, mean) and np.array_equal(c3, cov)      # (these models' Syy is diagonal)
    a, b = gm.prepare(weight, m2, c2, 4, 2), gm.prepare(weight, mean, cov, 4, 2)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_the_rule_uses_the_c_library_logarithm():
    import gmm_rule as gm
    src = inspect.getsource(gm.prepare)
    assert "math.log" in src and "np.log" not in src


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert {"wc_mlpg_device", "wc_mlpg_gv_device", "wc_model_feature_width"} <= exported
