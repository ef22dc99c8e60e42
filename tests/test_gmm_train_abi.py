"""CPU tests of the GMM training's boundary: include/world_class_gmm_train.h declares exactly the symbols of GMM_TRAIN_SIGNATURES with
their arity and types and states the rule; header, host half and translation unit are part of the build; the mirror exists with its
parameter names; the other tables and world_class_gmm.h are untouched; the tree compiles for gfx950 without a GPU and exports the
symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_gmm_train.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_gmm_trainer_create": (3, r"wc_gmm_trainer\s*\*\s*", C.c_void_p),
    "wc_gmm_trainer_destroy": (1, r"void\s+", None),
    "wc_gmm_trainer_set_model": (4, r"int\s+", C.c_int),
    "wc_gmm_trainer_model_host": (4, r"int\s+", C.c_int),
    "wc_gmm_trainer_posterior_device": (9, r"int\s+", C.c_int),
    "wc_gmm_trainer_accumulate_device": (7, r"int\s+", C.c_int),
    "wc_gmm_trainer_stats_host": (5, r"int\s+", C.c_int),
    "wc_gmm_trainer_update": (4, r"int\s+", C.c_int),
    "wc_gmm_trainer_reset_stats": (1, r"int\s+", C.c_int),
    "wc_gmm_trainer_set_segments_per_launch": (2, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.gmm_train import GMM_TRAIN_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = GMM_TRAIN_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.gmm_train import GMM_TRAIN_SIGNATURES
    assert declared_symbols(HEADER) == sorted(GMM_TRAIN_SIGNATURES) == sorted(NEW)


def test_argument_types_and_the_info_record():
    from world_class_amd.gmm_train import GMM_TRAIN_SIGNATURES as S, TrainInfo
    dp, vp, i, ll, ip = C.POINTER(C.c_double), C.c_void_p, C.c_int, C.c_longlong, C.POINTER(TrainInfo)
    assert S["wc_gmm_trainer_create"][1] == [i, i, i]
    assert S["wc_gmm_trainer_destroy"][1] == [vp]
    assert S["wc_gmm_trainer_set_model"][1] == [vp, dp, dp, dp] == S["wc_gmm_trainer_model_host"][1]
    assert S["wc_gmm_trainer_posterior_device"][1] == [vp, ll, i, vp, i, i, vp, vp, vp]
    assert S["wc_gmm_trainer_accumulate_device"][1] == [vp, ll, i, vp, i, i, vp]
    assert S["wc_gmm_trainer_stats_host"][1] == [vp, dp, dp, dp, ip]
    assert S["wc_gmm_trainer_update"][1] == [vp, C.c_double, dp, ip]
    assert S["wc_gmm_trainer_reset_stats"][1] == [vp] and S["wc_gmm_trainer_set_segments_per_launch"][1] == [vp, i]
    assert [(n, t) for n, t in TrainInfo._fields_] == [("loglik", C.c_double), ("n_live", ll), ("n_dropped", ll), ("n_starved", i), ("n_kept", i)]
    src = re.sub(r"\s+", " ", _source(HEADER))
    assert "typedef struct { double loglik; long long n_live, n_dropped; int n_starved, n_kept; } wc_gmm_train_info;" in src
    assert C.sizeof(TrainInfo) == 32


def test_the_header_states_its_types_and_the_rule():
    src = _source(HEADER)
    assert re.search(r'#include\s+"world_class_gmm.h"', src)
    assert re.search(r"typedef struct wc_gmm_trainer wc_gmm_trainer;", src)
    assert re.search(r"wc_gmm_trainer \*wc_gmm_trainer_create\(int n_mix, int dx, int dy\)", src)
    assert re.search(r"int wc_gmm_trainer_accumulate_device\(wc_gmm_trainer \*t, long long n_frames, int format, const void \*d_rows, int ld, int col,"
                     r"\s+const unsigned char \*d_mask\)", src)
    assert re.search(r"int wc_gmm_trainer_update\(wc_gmm_trainer \*t, double min_occupancy, const double \*h_var_floor, wc_gmm_train_info \*info\)", src)
    whole = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", HEADER)).read())   # (the comment's lines joined)
    for word in ("Every operation is in double, rounded on its own, with no fma",
                 "that rule with dx := D and Sxx := the joint covariance",
                 "ll(t, m) is THE rule of convert on the joint row with that W, mux := mean and c",
                 "top is the greatest ll that is not NaN", "A frame whose mask byte is 0 is masked",
                 "A frame that is not masked and has no finite top is dropped and counted",
                 "gamma(m) = 0.0 for every m and frame_ll = 0.0, and the statistics do not read their rows",
                 "e(m) = exp(ll(m) - top), and 0.0 where ll(m) is NaN", "s is the sum of e(m) over m ascending, starting at its first term",
                 "gamma(m) = e(m) / s", "frame_ll = top + log(s)", "exp and log are the device library's",
                 "d(i) = z_t(i) - mean_m(i), centred on the model in force", "g = gamma(t, m) * d(i)", "N_m sums gamma(t, m)", "S1_m(i) sums g",
                 "S2_m(i, j), j <= i, sums g * d(j)", "LL sums frame_ll", "segments of 1024 from the call's first frame",
                 "every sum runs over the live frames ascending and starts at its first term", "an empty sum is +0.0",
                 "folded into the totals ascending, total = total + partial", "Totals start at +0.0 after create, update and reset",
                 "A mixture with !(N_m >= min_occupancy) is starved", "w = N_m / (double)n_live", "delta(i) = S1(i) / N_m",
                 "mean(i) = mean(i) + delta(i)", "cov(i, j) = S2(i, j) / N_m - delta(i) * delta(j)", "raised to h_var_floor[i]",
                 "The upper triangle is mirrored", "keeps its three old values and is counted in n_kept", "loglik = LL",
                 "Weights need not sum to 1", "depends neither on the launch shape nor on how many segments a launch takes",
                 "multiples of 1024 equals the one call bit for bit", "any other cut equals the rule for that cut",
                 "Every loop is bounded by n_mix, D and the segment", "No atomics and no matrix instructions",
                 "n_mix outside 1..1024", "D outside 2..192", "before a model is set", "a format outside {0, 1}", "a negative column",
                 "ld < col + D", "n_frames < 0 or > 2^32 - 1", "both outputs of posterior NULL", "min_occupancy not finite or < 1",
                 "a floor that is negative or not finite", "update with n_live == 0", "g < 0", "n_frames == 0 does nothing",
                 "wc_release_scratch", "wc_set_stream", "the convention of world_class_gv.h"):
        assert word.lower() in whole.lower(), word   # the rule stands in the header


def test_the_other_tables_and_headers_are_unchanged():
    import world_class_amd as w
    from world_class_amd.features import FEATURES_SIGNATURES
    from world_class_amd.gmm import GMM_SIGNATURES
    from world_class_amd.gmm_train import GMM_TRAIN_SIGNATURES
    from world_class_amd.gv import GV_SIGNATURES
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES
    from world_class_amd.resample import RESAMPLE_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.vresample import VRESAMPLE_SIGNATURES
    from world_class_amd.warp import WARP_SIGNATURES
    from world_class_amd.warp_stream import WARP_STREAM_SIGNATURES
    assert sorted(GMM_SIGNATURES) == ["wc_gmm_convert_device", "wc_gmm_create", "wc_gmm_destroy", "wc_gmm_prepared_host"]
    assert declared_symbols("world_class_gmm.h") == sorted(GMM_SIGNATURES)
    assert sorted(GV_SIGNATURES) == ["wc_gv_stats_device", "wc_mlpg_gv_device"] and len(FEATURES_SIGNATURES) == 4
    assert len(WARP_SIGNATURES) == 5 and len(VRESAMPLE_SIGNATURES) == 16 and len(RESAMPLE_SIGNATURES) == 15 and len(STREAM_SIGNATURES) == 46
    assert len(WARP_STREAM_SIGNATURES) == 15 and len(MLPG_STREAM_SIGNATURES) == 11
    others = (set(WARP_SIGNATURES) | set(VRESAMPLE_SIGNATURES) | set(RESAMPLE_SIGNATURES) | set(STREAM_SIGNATURES) | set(WARP_STREAM_SIGNATURES)
              | set(FEATURES_SIGNATURES) | set(MLPG_STREAM_SIGNATURES) | set(GV_SIGNATURES) | set(GMM_SIGNATURES) | set(w.EXPORTED_SYMBOLS))
    assert not set(GMM_TRAIN_SIGNATURES) & others
    for header in ("world_class_c.h", "world_class_features.h", "world_class_gv.h", "world_class_gmm.h"):
        assert not [s for s in declared_symbols(header) if s in GMM_TRAIN_SIGNATURES]
        assert "_trainer_" not in open(os.path.join(ROOT, "include", header)).read()


def test_header_host_half_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    csrc = os.path.join(ROOT, "world_class_amd", "csrc")
    assert os.path.join(ROOT, "include", HEADER) in build.headers() and os.path.join(ROOT, "include", "world_class_gmm.h") in build.headers()
    for hpp in ("wc_gmm_train_plan.hpp", "wc_gmm_plan.hpp", "wc_gmm_ll.hpp"):
        assert os.path.join(csrc, hpp) in build.headers()
    assert "wc_gmm_train.hip" in build.sources() and "wc_gmm.hip" in build.sources()
    plan = open(os.path.join(csrc, "wc_gmm_train_plan.hpp")).read()
    assert "#include <hip" not in plan and "__global__" not in plan and "__device__" not in plan     # the host half is plain C++
    hip = open(os.path.join(csrc, "wc_gmm_train.hip")).read()
    assert "atomic" not in hip.replace("No atomics", "").lower() and "mfma" not in hip.lower()


def test_the_entry_point_loads_the_table():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "wgmm_train.GMM_TRAIN_SIGNATURES" in src and "from world_class_amd import gmm_train as wgmm_train" in src


def test_mirror_exists_with_its_parameter_names_and_defaults():
    from world_class_amd import features, gmm_train as gt
    sig = lambda f: list(inspect.signature(f).parameters)
    T = gt.GmmTrainer
    assert sig(T.__init__) == ["self", "n_mix", "dx", "dy"]
    assert sig(T.set_model) == ["self", "weight", "mean", "cov"] and sig(T.model) == ["self"]
    assert sig(T.posterior) == ["self", "n_frames", "d_rows", "ld", "d_post", "d_frame_ll", "col", "d_mask", "format"]
    assert sig(T.accumulate) == ["self", "n_frames", "d_rows", "ld", "col", "d_mask", "format"]
    assert sig(T.stats) == ["self"] and sig(T.update) == ["self", "min_occupancy", "var_floor"] and sig(T.reset_stats) == ["self"]
    assert sig(T.fit)[:5] == ["self", "d_rows", "n", "ld", "iters"] and sig(T.to_gmm) == ["self"] and sig(T.close) == ["self"]
    assert sig(T.set_segments_per_launch) == ["self", "g"]
    assert sig(gt.initial_model) == ["rows", "n_mix", "seed"]
    d = inspect.signature(T.accumulate).parameters
    assert (d["col"].default, d["d_mask"].default, d["format"].default) == (0, None, "f64")
    assert gt.FORMATS is features.FORMATS and gt._check is features._check and gt._binder is features._binder


def test_initial_model_is_seeded_frames_the_global_diagonal_and_equal_weights():
    from world_class_amd import gmm_train as gt
    rows = np.random.default_rng(4).normal(size=(50, 3)) * [1.0, 2.0, 3.0]
    w, mean, cov = gt.initial_model(rows, 5, 9)
    w2, mean2, cov2 = gt.initial_model(rows, 5, 9)
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2) and np.array_equal(w, w2) and (w == 0.2).all()
    assert all(any(np.array_equal(mu, r) for r in rows) for mu in mean) and len({tuple(mu) for mu in mean}) == 5
    assert np.array_equal(cov[0], np.diag(rows.var(axis=0))) and all(np.array_equal(c, cov[0]) for c in cov)
    assert not np.array_equal(gt.initial_model(rows, 5, 10)[1], mean)
    with pytest.raises(ValueError):
        gt.initial_model(rows, 51, 0)


def test_the_rule_uses_the_c_library_exp_and_log():
    import gmm_train_rule as tr
    src = inspect.getsource(tr.posteriors) + inspect.getsource(tr.constant)
    assert "math.exp" in src and "math.log" in src and "np.exp" not in src and "np.log" not in src


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert {"wc_gmm_create", "wc_gmm_convert_device", "wc_mlpg_device"} <= exported
