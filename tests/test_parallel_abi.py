"""CPU tests of the boundary of the parallel-corpus calls: include/world_class_parallel.h declares exactly the symbols of
PARALLEL_SIGNATURES with their arity and types and states the rule; header, host half and translation unit are part of the build; the
mirror exists with its parameter names; the other tables and headers are untouched; the tree compiles for gfx950 without a GPU and
exports the symbols."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_parallel.h"
NEW = {"wc_joint_rows_device": 22, "wc_speech_mask_device": 9, "wc_path_distortion_device": 19}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.parallel import PARALLEL_SIGNATURES
    assert declared_arity(symbol, r"int\s+", header=HEADER) == NEW[symbol]
    res, args = PARALLEL_SIGNATURES[symbol]
    assert res is C.c_int and len(args) == NEW[symbol]


def test_the_table_is_the_header():
    from world_class_amd.parallel import PARALLEL_SIGNATURES
    assert declared_symbols(HEADER) == sorted(PARALLEL_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.parallel import PARALLEL_SIGNATURES as S
    vp, i, ip, d = C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_double
    assert S["wc_joint_rows_device"][1] == [i, ip, ip, i, vp, i, i, i, i, vp, i, i, i, vp, vp, vp, vp, i, vp, i, i, vp]
    assert S["wc_speech_mask_device"][1] == [i, ip, i, vp, i, i, d, d, vp]
    assert S["wc_path_distortion_device"][1] == [i, ip, ip, i, vp, i, i, i, vp, i, i, i, vp, vp, vp, vp, vp, vp, vp]


def test_the_header_states_its_declarations_and_the_rule():
    src = re.sub(r"\s+", " ", _source(HEADER))
    assert re.search(r'#include\s+"world_class_gmm_train.h"', _source(HEADER))
    for decl in ("int wc_joint_rows_device(int n_pairs, const int *a_length, const int *b_length, int a_format, const void *d_rows_a, int ld_a, "
                 "int col_a, int dx, int b_format, const void *d_rows_b, int ld_b, int col_b, int dy, const int *d_path_length, const int *d_path, "
                 "const unsigned char *d_mask_a, const unsigned char *d_mask_b, int out_format, void *d_joint, int ld_out, int col_out, "
                 "unsigned char *d_joint_mask);",
                 "int wc_speech_mask_device(int n_utt, const int *lengths, int format, const void *d_rows, int ld, int col, double margin, "
                 "double floor, unsigned char *d_mask);",
                 "int wc_path_distortion_device(int n_pairs, const int *a_length, const int *b_length, int a_format, const void *d_rows_a, int ld_a, "
                 "int col_a, int b_format, const void *d_rows_b, int ld_b, int col_b, int dims, const int *d_path_length, const int *d_path, "
                 "const unsigned char *d_mask_a, const unsigned char *d_mask_b, double *d_sum, long long *d_count, double *d_cell);"):
        assert decl in src, decl
    whole = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", HEADER)).read())   # (the comment's lines joined)
    for word in ("A_u = sum_{v<u} a_length[v]", "cap_u = a + b - 1", "P_u = sum_{v<u} cap_v", "K' = K if 0 <= K <= cap_u, else K' = 0",
                 "on the path iff s < K', 0 <= i < a and 0 <= j < b", "a NULL mask means every frame counts", "the convention of world_class_gv.h",
                 "an entry that is not on the path is never used as an index", "A float read is widened exactly",
                 "a float written is the (float) of the double", "same format to same format copies the bits",
                 "one row and one mask byte per slot, so the host never needs K", "those dx + dy columns are +0.0 and the mask byte is 0",
                 "Every other column of every output row is left exactly as it was", "d_joint_mask may be NULL; d_joint may not",
                 "wc_gmm_trainer_accumulate_device(t, sum cap, out_format, d_joint, ld_out, col_out, d_joint_mask)",
                 "top is the greatest value of the column that is finite", "v >= top - margin (one rounded subtraction) and v >= floor",
                 "With no finite value in the utterance every byte is 0", "margin = +inf and floor = -inf are allowed",
                 "Nothing crosses an utterance boundary", "A maximum is exact, so the launch shape cannot change a byte",
                 "out[i] = (re * w.x - im * w.y) / normalization", "One decibel is ln(10) / 10 units of c0", "0.23025850929940458",
                 "every difference, product and sum rounded on its own, no fma, the square root correctly rounded",
                 "the local cost of wc_align_features_device, word for word", "d_count[u] is the number of live slots",
                 "the sum starts at its first term and is +0.0 for none", "The sum is strictly sequential on purpose",
                 "e(s) for slots on the path, whether live or not, and +0.0 for the others", "Values that are not finite travel through",
                 "The value of d_sum does not depend on the launch shape", "equals the alignment's d_cost[u] bit for bit at every length",
                 "mcd_db = (10 / ln 10) * sqrt(2) * sum / count", "only enqueue, on wc_set_stream's stream",
                 "refuse before anything is enqueued or written", "n_pairs / n_utt < 0", "a length below 1 for a pair",
                 "a negative utterance length", "a format outside {0, 1}", "a negative column", "dx, dy or dims < 1", "dx + dy > 384",
                 "an ld smaller than col plus the width read or written", "more than 2^31 - 1 slots, or 2^32 - 1 frames, in all",
                 "margin or floor NaN; margin < 0", "all three outputs of the distortion call NULL",
                 "an output that overlaps an input or another output", "n_pairs == 0 / n_utt == 0 write nothing", "No atomics"):
        assert word.lower() in whole.lower(), word   # the rule stands in the header


def test_the_decibel_follows_from_the_codecs_line():
    """the line the header quotes stands in the codec, with the weight and the normalisation the derivation uses"""
    from world_class_amd import parallel
    codec = open(os.path.join(ROOT, "world_class_amd", "csrc", "wc_codec.hip")).read()
    assert "out[i] = (re * w.x - im * w.y) / normalization;" in codec and "const double normalization = sqrt((double)MD);" in codec
    assert "2.0 * std::cos(i * kPiH / fft_size) / std::sqrt((double)fft_size)" in codec and "w[0].x /= std::sqrt(2.0);" in codec
    for fft_size in (512, 1024, 2048):          # c0 = sum * w[0].x / normalization = sum / (fft_size / 2): the mean over the mel axis
        w0, norm = 2.0 / math.sqrt(fft_size) / math.sqrt(2.0), math.sqrt(fft_size / 2)
        assert abs(w0 / norm - 1.0 / (fft_size / 2)) < 1e-18
    assert parallel.DB_IN_C0 == math.log(10.0) / 10.0


def test_the_other_tables_and_headers_are_unchanged():
    import world_class_amd as w
    from world_class_amd.features import FEATURES_SIGNATURES
    from world_class_amd.filter import FILTER_SIGNATURES
    from world_class_amd.filter_stream import FILTER_STREAM_SIGNATURES
    from world_class_amd.gmm import GMM_SIGNATURES
    from world_class_amd.gmm_train import GMM_TRAIN_SIGNATURES
    from world_class_amd.gv import GV_SIGNATURES
    from world_class_amd.io import IO_SIGNATURES
    from world_class_amd.parallel import PARALLEL_SIGNATURES
    assert len(GMM_TRAIN_SIGNATURES) == 10 and len(GMM_SIGNATURES) == 4 and len(GV_SIGNATURES) == 2 and len(FEATURES_SIGNATURES) == 4
    assert declared_symbols("world_class_gmm_train.h") == sorted(GMM_TRAIN_SIGNATURES)
    others = (set(FEATURES_SIGNATURES) | set(FILTER_SIGNATURES) | set(FILTER_STREAM_SIGNATURES) | set(GMM_SIGNATURES) | set(GMM_TRAIN_SIGNATURES)
              | set(GV_SIGNATURES) | set(IO_SIGNATURES) | set(w.EXPORTED_SYMBOLS))
    assert not set(PARALLEL_SIGNATURES) & others
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header.endswith(".h") and header != HEADER:
            text = open(os.path.join(ROOT, "include", header)).read()
            assert not [s for s in PARALLEL_SIGNATURES if s in text], header


def test_header_host_half_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    csrc = os.path.join(ROOT, "world_class_amd", "csrc")
    assert os.path.join(ROOT, "include", HEADER) in build.headers() and os.path.join(csrc, "wc_parallel_plan.hpp") in build.headers()
    assert "wc_parallel.hip" in build.sources()
    plan = open(os.path.join(csrc, "wc_parallel_plan.hpp")).read()
    assert "#include <hip" not in plan and "__global__" not in plan and "__device__" not in plan     # the host half is plain C++
    hip = open(os.path.join(csrc, "wc_parallel.hip")).read()
    assert "atomic" not in hip.replace("No atomics", "").lower() and "asm" not in hip.lower()


def test_the_entry_point_loads_the_table():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "wparallel.PARALLEL_SIGNATURES" in src and "from world_class_amd import parallel as wparallel" in src


def test_mirror_exists_with_its_parameter_names_and_defaults():
    from world_class_amd import features, parallel as p
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(p.joint_rows) == ["a_lengths", "b_lengths", "d_rows_a", "ld_a", "dx", "d_rows_b", "ld_b", "dy", "d_path_length", "d_path", "d_joint",
                                 "ld_out", "d_joint_mask", "col_a", "col_b", "col_out", "d_mask_a", "d_mask_b", "a_format", "b_format", "out_format"]
    assert sig(p.speech_mask) == ["lengths", "d_rows", "ld", "d_mask", "col", "margin", "floor", "format"]
    assert sig(p.path_distortion) == ["a_lengths", "b_lengths", "d_rows_a", "ld_a", "d_rows_b", "ld_b", "dims", "d_path_length", "d_path", "d_sum",
                                      "d_count", "d_cell", "col_a", "col_b", "d_mask_a", "d_mask_b", "a_format", "b_format"]
    assert sig(p.joint_rows_host)[:6] == ["a_lengths", "b_lengths", "rows_a", "rows_b", "path_length", "path"] and sig(p.mcd_db) == ["total", "count"]
    assert sig(p.fit_parallel)[:12] == ["a_lengths", "b_lengths", "nd", "n_ap", "orders", "d_f0_a", "d_sp_a", "d_ap_a", "d_f0_b", "d_sp_b", "d_ap_b",
                                        "n_mix"]
    d = inspect.signature(p.fit_parallel).parameters
    assert (d["rounds"].default, d["iters"].default, d["margin_db"].default, d["floor"].default) == (1, 5, 40.0, -math.inf)
    d = inspect.signature(p.speech_mask).parameters
    assert (d["col"].default, d["margin"].default, d["floor"].default, d["format"].default) == (0, math.inf, -math.inf, "f64")
    assert p.FORMATS is features.FORMATS and p._check is features._check and p._binder is features._binder
    assert p.mcd_db(3.0, 2) == (10.0 / math.log(10.0)) * math.sqrt(2.0) * 3.0 / 2.0 and p.slots([3, 1], [2, 9]) == 4 + 9
    src = inspect.getsource(p.fit_parallel)
    assert "torch" not in src and "numpy" not in src.replace("numpy.", "")          # the loop runs on the library's calls


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert {"wc_gmm_trainer_accumulate_device", "wc_align_features_device", "wc_pack_model_features_device"} <= exported
