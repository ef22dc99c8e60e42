"""CPU tests of the frame filter's boundary: include/world_class_filter.h declares exactly the symbols of FILTER_SIGNATURES with their
arity and types and states the rule, header and translation unit are part of the build, the minimum-phase forms are stated once,
the mirror exists with its parameter names and defaults, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_filter.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_frame_filter_create": (3, r"wc_frame_filter\s*\*\s*", C.c_void_p),
    "wc_frame_filter_destroy": (1, r"void\s+", None),
    "wc_frame_filter_segments": (2, r"int\s+", C.c_int),
    "wc_frame_filter_run_device": (8, r"int\s+", C.c_int),
    "wc_frame_filter_run_coded_device": (10, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.filter import FILTER_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = FILTER_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.filter import FILTER_SIGNATURES
    assert declared_symbols(HEADER) == sorted(FILTER_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.filter import FILTER_SIGNATURES as S, KINDS
    ip, vp, i, d = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double
    assert S["wc_frame_filter_create"][1] == [i, i, d]
    assert S["wc_frame_filter_destroy"][1] == [vp]
    assert S["wc_frame_filter_segments"][1] == [vp, i]
    assert S["wc_frame_filter_run_device"][1] == [vp, i, vp, ip, i, vp, ip, vp]
    assert S["wc_frame_filter_run_coded_device"][1] == [vp, i, vp, ip, vp, vp, i, i, ip, vp]
    src = _source(HEADER)
    assert re.search(r"#define\s+WC_FILTER_POWER\s+0\b", src) and re.search(r"#define\s+WC_FILTER_LOG\s+1\b", src)
    assert KINDS == {"power": 0, "log": 1}


def test_the_header_states_its_types_and_the_rule():
    src = _source(HEADER)
    assert re.search(r'#include\s+"world_class_c.h"', src)
    assert re.search(r"typedef struct wc_frame_filter wc_frame_filter;", src)
    assert re.search(r"wc_frame_filter \*wc_frame_filter_create\(int fs, int fft_size, double frame_period_ms\)", src)
    assert re.search(r"int wc_frame_filter_segments\(const wc_frame_filter \*f, int x_length\)", src)
    assert re.search(r"int wc_frame_filter_run_device\(wc_frame_filter \*f, int n_utt, const double \*d_x, const int \*x_length, int kind,"
                     r"\s+const double \*d_rows, const int \*f_length, double \*d_y\)", src)
    assert re.search(r"int wc_frame_filter_run_coded_device\(wc_frame_filter \*f, int n_utt, const double \*d_x, const int \*x_length,"
                     r"\s+const double \*d_coded_to, const double \*d_coded_from, int number_of_dimensions,"
                     r"\s+int skip_energy, const int \*f_length, double \*d_y\)", src)
    whole = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", HEADER)).read())   # (the comment's lines joined)
    for word in ("Everything is in double", "h = frame_period_ms * fs / 1000.0",
                 "c_t = (long long)floor(((double)t * frame_period_ms) * (double)fs / 1000.0 + 0.5)",
                 "S is the least count with c_{S-1} >= n - 1", "uses row min(t, f_length - 1)", "the last row is held",
                 "Rows from S on are not read", "up = (double)(k - c_t) / (double)(c_{t+1} - c_t)",
                 "It enters segment t+1 with weight up and segment t with weight 1.0 - up", "k == c_t enters segment t with weight 1.0",
                 "a_t = (t ? c_{t-1} + 1 : 0) to b_t = min(n - 1, c_{t+1} - 1), with L_t = b_t - a_t + 1",
                 "s_t[j] = x[a_t + j] * w, placed at j = 0..L_t-1 of N points and zero behind",
                 "as tests/minimum_phase_rule.py states it", "with e^{+i} transforms", "R = forward(s_t)[0..N/2] * M_t",
                 "extended by Hermitian symmetry", "r_t[j] = Re(sum_k R[k] e^{-2 pi i jk/N}) / N", "wrap included",
                 "the rule is the circular one", "decayed within N - L_t samples",
                 "If a value of ls_t is not finite, the whole row r_t is NaN", "judged after the log, so a gain <= 0, NaN or infinite counts",
                 "y[k] = 0.0, then y[k] += r_t[k - a_t] for every segment with a_t <= k < a_t + N, t ascending", "No atomics",
                 "Every sample of y is written", "depends neither on the launch shape nor on which utterances share a batch",
                 "d[i] = to[i] - from[i]", "from == NULL means d = to", "with skip_energy != 0, d[0] = 0.0",
                 "exactly as wc_decode_spectral_envelope_device writes them", "equals those two public calls bit for bit",
                 "y[0 .. a_t) depends only on x[0 .. c_t) and rows < t", "ls = log(g) / 2", "taken as they are",
                 "only enqueue, on wc_set_stream's stream", "d_y == d_x is allowed", "any other overlap is refused",
                 "segments x fft_size doubles", "grows on demand and goes with it",
                 "Every refusal happens before anything is allocated, enqueued or written", "512, 1024, 2048 or 4096", "fs <= 0",
                 "h not finite or < 1", "2 * ceil(h) - 1 > fft_size / 2", "takes 16 ms frames and refuses 16.0625 ms", "n_utt < 0",
                 "a negative length", "x_length[u] > 0 with f_length[u] < 1", "a kind outside {0, 1}", "NULL arrays with work to do",
                 "d_y overlapping anything but d_x exactly", "number_of_dimensions outside 1..fft_size/2", "a NULL d_coded_to",
                 "x_length[u] == 0 writes nothing for that utterance"):
        assert word.lower() in whole.lower(), word   # the rule stands in the header


def test_the_other_tables_and_headers_are_unchanged():
    import world_class_amd as w
    from world_class_amd.codec import CODEC_SIGNATURES
    from world_class_amd.filter import FILTER_SIGNATURES
    from world_class_amd.gmm import GMM_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.warp import WARP_SIGNATURES
    assert len(GMM_SIGNATURES) == 4 and len(WARP_SIGNATURES) == 5 and len(STREAM_SIGNATURES) == 46
    assert not set(FILTER_SIGNATURES) & (set(GMM_SIGNATURES) | set(WARP_SIGNATURES) | set(STREAM_SIGNATURES) | set(CODEC_SIGNATURES)
                                         | set(w.EXPORTED_SYMBOLS))
    for header in ("world_class_c.h", "world_class_codec.h", "world_class_io.h", "world_class_warp.h", "world_class_gmm.h"):
        assert not [s for s in declared_symbols(header) if s in FILTER_SIGNATURES]


def test_header_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert os.path.join(ROOT, "world_class_amd", "csrc", "wc_minphase.hpp") in build.headers()
    assert "wc_filter.hip" in build.sources() and "wc_synthesis.hip" in build.sources()


def test_the_minimum_phase_forms_are_stated_once():
    csrc = os.path.join(ROOT, "world_class_amd", "csrc")
    hpp = open(os.path.join(csrc, "wc_minphase.hpp")).read()
    for form in ("minimum_phase_lds", "minimum_phase_wave", "minimum_phase_wave8"):
        assert len(re.findall(r"__device__ __forceinline__ void %s\(" % form, hpp)) == 1
        for unit in ("wc_synthesis.hip", "wc_filter.hip"):
            src = open(os.path.join(csrc, unit)).read()
            assert '#include "wc_minphase.hpp"' in src and form + "(" in src.replace("<N, T>", "")   # used there ...
            assert not re.search(r"__device__ __forceinline__ void %s\(" % form, src)                 # ... and defined in the header alone


def test_the_development_option_is_read_through_the_options_header():
    src = open(os.path.join(ROOT, "world_class_amd", "csrc", "wc_filter.hip")).read()
    assert '#include "wc_options.hpp"' in src and 'opt_is("WC_FILTER_KERNEL", "block")' in src and "getenv" not in src


def test_the_entry_point_loads_the_table():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "wfilter.FILTER_SIGNATURES" in src and "from world_class_amd import filter as wfilter" in src


def test_mirror_exists_with_its_parameter_names_and_defaults():
    from world_class_amd import _binding, filter as ff
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(ff.FrameFilter.__init__) == ["self", "fs", "fft_size", "frame_period_ms"]
    assert sig(ff.FrameFilter.segments) == ["self", "x_length"]
    assert sig(ff.FrameFilter.run) == ["self", "d_x", "x_lengths", "d_rows", "f_lengths", "d_y", "kind"]
    assert sig(ff.FrameFilter.run_coded) == ["self", "d_x", "x_lengths", "d_coded_to", "d_coded_from", "number_of_dimensions", "f_lengths", "d_y",
                                             "skip_energy"]
    assert sig(ff.FrameFilter.filter) == ["self", "x", "rows", "kind"]
    assert sig(ff.FrameFilter.filter_coded) == ["self", "x", "coded_to", "coded_from", "skip_energy"]
    assert sig(ff.FrameFilter.close) == ["self"] and issubclass(ff.FrameFilter, _binding._Handle)
    d = inspect.signature(ff.FrameFilter.__init__).parameters
    assert d["frame_period_ms"].default == 5.0
    assert inspect.signature(ff.FrameFilter.run).parameters["kind"].default == "power"
    d = inspect.signature(ff.FrameFilter.filter_coded).parameters
    assert d["coded_from"].default is None and d["skip_energy"].default is False
    assert ff._check is _binding._check and ff._binder is _binding._binder


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert {"wc_synthesis_compute_device", "wc_decode_spectral_envelope_device", "wc_debug_minimum_phase"} <= exported
