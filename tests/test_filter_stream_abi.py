"""CPU tests of the filter streams' boundary: include/world_class_filter_stream.h declares exactly the symbols of
FILTER_STREAM_SIGNATURES with their arity and types and states the rule, the other tables are unchanged, the new source and headers are
part of the build, wc_filter_stream.hip defines no segment kernel of its own and reaches those of wc_filter.hip through the one launch
function, the mirror exists with its parameter names, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_vresample_abi import ROOT, _source, declared_arity, declared_symbols

HEADER = "world_class_filter_stream.h"
CSRC = os.path.join(ROOT, "world_class_amd", "csrc")
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_filter_stream_segments_done": (4, r"long long\s+", C.c_longlong),
    "wc_filter_stream_committed": (3, r"long long\s+", C.c_longlong),
    "wc_filter_stream_create": (7, r"wc_filter_stream\s*\*\s*", C.c_void_p),
    "wc_filter_stream_destroy": (1, r"void\s+", None),
    "wc_filter_stream_reset": (2, r"int\s+", C.c_int),
    "wc_filter_stream_push_device": (8, r"int\s+", C.c_int),
    "wc_filter_stream_push_coded_device": (11, r"int\s+", C.c_int),
    "wc_filter_stream_samples_received": (2, r"long long\s+", C.c_longlong),
    "wc_filter_stream_rows_received": (2, r"long long\s+", C.c_longlong),
    "wc_filter_stream_segments_done_of": (2, r"long long\s+", C.c_longlong),
    "wc_filter_stream_samples_committed": (2, r"long long\s+", C.c_longlong),
    "wc_filter_stream_pending_samples": (2, r"int\s+", C.c_int),
    "wc_filter_stream_pending_rows": (2, r"int\s+", C.c_int),
}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.filter_stream import FILTER_STREAM_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result, header=HEADER) == arity
    res, args = FILTER_STREAM_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity


def test_the_table_is_the_header():
    from world_class_amd.filter_stream import FILTER_STREAM_SIGNATURES
    assert declared_symbols(HEADER) == sorted(FILTER_STREAM_SIGNATURES) == sorted(NEW)


def test_argument_types():
    from world_class_amd.filter_stream import FILTER_STREAM_SIGNATURES as S
    ip, vp, i, d, ll = C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_double, C.c_longlong
    assert S["wc_filter_stream_segments_done"][1] == [i, d, ll, ll] and S["wc_filter_stream_committed"][1] == [i, d, ll]
    assert S["wc_filter_stream_create"][1] == [i, i, d, i, i, i, i]
    assert S["wc_filter_stream_destroy"][1] == [vp] and S["wc_filter_stream_reset"][1] == [vp, i]
    assert S["wc_filter_stream_push_device"][1] == [vp, ip, vp, ip, vp, ip, vp, ip]
    assert S["wc_filter_stream_push_coded_device"][1] == [vp, ip, vp, ip, vp, vp, i, i, ip, vp, ip]
    for name in ("samples_received", "rows_received", "segments_done_of", "samples_committed", "pending_samples", "pending_rows"):
        assert S["wc_filter_stream_" + name][1] == [vp, i]


def test_the_header_states_its_types_and_the_rule():
    src = _source(HEADER)
    assert re.search(r'#include\s+"world_class_filter.h"', src)
    assert re.search(r"typedef struct wc_filter_stream wc_filter_stream;", src)
    assert re.search(r"long long wc_filter_stream_segments_done\(int fs, double frame_period_ms, long long n, long long rows\)", src)
    assert re.search(r"long long wc_filter_stream_committed\(int fs, double frame_period_ms, long long segments_done\)", src)
    assert re.search(r"wc_filter_stream \*wc_filter_stream_create\(int fs, int fft_size, double frame_period_ms, int kind, int n_streams,"
                     r"\s+int max_pending_samples, int max_pending_rows\)", src)
    assert re.search(r"int wc_filter_stream_push_device\(wc_filter_stream \*h, const int \*n_samples, const double \*d_x, const int \*n_rows,"
                     r"\s+const double \*d_rows, const int \*flush, double \*d_y, int \*samples_out\)", src)
    assert re.search(r"int wc_filter_stream_push_coded_device\(wc_filter_stream \*h, const int \*n_samples, const double \*d_x, const int \*n_rows,"
                     r"\s+const double \*d_coded_to, const double \*d_coded_from, int number_of_dimensions,"
                     r"\s+int skip_energy, const int \*flush, double \*d_y, int \*samples_out\)", src)
    whole = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", HEADER)).read())   # (the comment's lines joined)
    for word in ("T(n, F) is the largest T with 0 <= T <= F and c_T <= n",
                 "Segment t is done when row t is in and every sample below c_{t+1} is in",
                 "A stream never holds a row before the flush: it cannot know that no further row comes",
                 "C(T) = T ? c_{T-1} + 1 : 0, which is a_T", "host arithmetic on counts alone", "Either count may be 0",
                 "rows may run ahead of samples, and samples ahead of rows", "It computes segments T_before .. T_after - 1",
                 "writes y[C_before .. C_after)", "samples_out[u] = C_after - C_before is filled before the call returns",
                 "is a flag per stream in the push", "It takes that push's samples and rows first",
                 "computes the remaining segments T .. S - 1 as the whole call does at n_total = n",
                 "b_t = min(n - 1, c_{t+1} - 1) and row min(t, F - 1)", "the last row is held, and rows from S on are not read",
                 "It writes y[C .. n)", "Afterwards the stream has ended until its reset", "A flush with n > 0 and F == 0 is refused",
                 "A flush with n == 0 writes nothing", "a flush flag for a stream that has ended does nothing",
                 "For any cut into pushes, the concatenated outputs, flush included, equal one whole call on (x[0..n), rows[0..F), kind), bit for bit",
                 "wc_frame_filter_run_device for a plain-push stream", "wc_frame_filter_run_coded_device for a coded-push stream",
                 "turns the N samples from its a_t into NaN and nothing else, across push borders too",
                 "No stream's outputs depend on another stream or on the launch shape",
                 "at most 2 ceil(h) - 2 samples behind its newest sample", "78 at hop 40, 1022 at hop 512, 128 at the tie hop 64.49999999999999",
                 "forms y[k] from 0.0 by adding r_t[k - a_t] with t ascending", "a tail of N partial sums behind C",
                 "Later segments add onto the tail, so the additions and their order are the whole call's",
                 "a window of pending samples x[a_T .. n) and a window of pending rows T .. F - 1",
                 "A push is accepted if, for every stream, pending-before plus pushed fits both",
                 "the new window is assembled before any segment is consumed", "samples_out[u] <= max_pending_samples",
                 "d_y holds n_streams x max_pending_samples doubles, packed by samples_out",
                 "a stream whose sample window is full is waiting for rows, so a push of rows alone is accepted and no state is a dead end",
                 "Tails and windows are kept in pairs", "a refused or failed push leaves every stream as it was",
                 "Counters are 64-bit on the host", "past 2^31 - 1 samples is refused", "A reset clears the tail",
                 "a stream after a reset behaves as a fresh one", "the pending rows are kept decoded", "kind must be WC_FILTER_POWER",
                 "A push only enqueues, on wc_set_stream's stream",
                 "one asynchronous copy of the records and a number of launches that does not depend on the number of streams",
                 "no device-to-host copy and no synchronisation", "segments of this push x fft_size doubles",
                 "Each happens before anything is enqueued, and every stream stays as it was",
                 "everything wc_frame_filter_create refuses", "a kind outside {0, 1}", "n_streams < 1", "max_pending_samples < 2 ceil(h)",
                 "max_pending_rows < 1", "byte counts that leave 63 bits", "a NULL handle, n_samples, n_rows or samples_out",
                 "a negative count", "a count that does not fit the windows", "samples or rows for a stream that has ended",
                 "NULL arrays with work to do", "d_y overlapping any input", "a flush with n > 0 and F == 0", "the 2^31 - 1 limit",
                 "number_of_dimensions outside 1 .. fft_size/2", "a NULL d_coded_to", "a handle whose kind is WC_FILTER_LOG"):
        assert word.lower() in whole.lower(), word   # the rule stands in the header


def test_the_rule_file_and_the_plan_speak_the_refusals_alike():
    import filter_stream_rule as fsr
    plan = open(os.path.join(CSRC, "wc_filter_stream_plan.hpp")).read()
    for text in (fsr.NEGATIVE, fsr.ENDED, fsr.NO_FIT, fsr.TOO_LONG, fsr.NO_ROW):
        assert '"%s"' % text in plan


def test_the_other_tables_and_headers_are_unchanged():
    import world_class_amd as w
    from world_class_amd.codec import CODEC_SIGNATURES
    from world_class_amd.filter import FILTER_SIGNATURES
    from world_class_amd.filter_stream import FILTER_STREAM_SIGNATURES
    from world_class_amd.gmm import GMM_SIGNATURES
    from world_class_amd.mlpg_stream import MLPG_STREAM_SIGNATURES
    from world_class_amd.stream import STREAM_SIGNATURES
    from world_class_amd.warp import WARP_SIGNATURES
    assert len(FILTER_SIGNATURES) == 5 and len(GMM_SIGNATURES) == 4 and len(WARP_SIGNATURES) == 5 and len(STREAM_SIGNATURES) == 46
    assert len(MLPG_STREAM_SIGNATURES) == 11
    assert not set(FILTER_STREAM_SIGNATURES) & (set(FILTER_SIGNATURES) | set(GMM_SIGNATURES) | set(WARP_SIGNATURES) | set(STREAM_SIGNATURES)
                                                | set(CODEC_SIGNATURES) | set(MLPG_STREAM_SIGNATURES) | set(w.EXPORTED_SYMBOLS))
    for header in ("world_class_c.h", "world_class_codec.h", "world_class_io.h", "world_class_filter.h", "world_class_stream.h"):
        assert not [s for s in declared_symbols(header) if s in FILTER_STREAM_SIGNATURES]


def test_headers_and_translation_unit_are_part_of_the_build():
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()
    assert os.path.join(CSRC, "wc_filter_stream_plan.hpp") in build.headers()
    assert "wc_filter_stream.hip" in build.sources() and "wc_filter.hip" in build.sources()


def test_the_segment_kernels_are_stated_once_and_shared_through_one_launch():
    stream, batch = (open(os.path.join(CSRC, f)).read() for f in ("wc_filter_stream.hip", "wc_filter.hip"))
    internal = open(os.path.join(CSRC, "wc_internal.hpp")).read()
    code = re.sub(r"//[^\n]*", "", stream)
    assert not re.search(r"filter_segment\w*_kernel", code) and "__global__" in code   # kernels of its own, but no segment kernel
    assert len(re.findall(r"__global__[^;{]*\bfilter_segment_wave_kernel\(", batch)) == 1
    assert len(re.findall(r"__global__[^;{]*\bfilter_segment_kernel\(", batch)) == 1
    assert len(re.findall(r"\bint filter_segments_launch\(Device \*dev, hipStream_t s, int fft_size, bool block, const FfArgs &a\);", internal)) == 1
    assert len(re.findall(r"\bint filter_segments_launch\(", batch)) == 1 and "filter_segments_launch(" in code
    assert len(re.findall(r"filter_segments_launch\(dev, s, N, f->block, a\)", batch)) == 1                # the batch goes through it too
    assert re.search(r"struct FfUtt \{[^}]*\bt0;", internal) and "struct FfUtt" not in batch and "struct FfUtt" not in code
    assert re.search(r"FfUtt\{xo, ro, so, x_length\[u\], f_length\[u\], S, 0\}", batch)                      # the batch passes t0 = 0
    # the centres: one expression, in the plan header, for the host and for both translation units
    plan = open(os.path.join(CSRC, "wc_filter_stream_plan.hpp")).read()
    assert len(re.findall(r"long long ff_centre\(", plan)) == 1 and not re.search(r"long long ff_centre\(", batch + stream)
    for unit in (batch, stream):
        assert '#include "wc_filter_stream_plan.hpp"' in unit
    assert "hip" not in re.sub(r"//[^\n]*", "", plan).replace("__HIPCC__", "").lower()     # plain C++
    assert "atomic" not in code.lower() and "hipMemcpyDeviceToHost" not in code and "Synchronize" not in code
    assert 'opt_is("WC_FILTER_KERNEL", "block")' in stream and "getenv" not in stream


def test_the_entry_point_loads_the_table():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "wfilter_stream.FILTER_STREAM_SIGNATURES" in src and "from world_class_amd import filter_stream as wfilter_stream" in src


def test_mirror_exists_with_its_parameter_names_and_defaults():
    from world_class_amd import _binding, filter_stream as fs
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(fs.FilterStream.__init__) == ["self", "fs", "fft_size", "frame_period_ms", "kind", "n_streams", "max_pending_samples", "max_pending_rows"]
    assert sig(fs.FilterStream.reset) == ["self", "stream"]
    assert sig(fs.FilterStream.push) == ["self", "n_samples", "d_x", "n_rows", "d_rows", "d_y", "flush"]
    assert sig(fs.FilterStream.push_coded) == ["self", "n_samples", "d_x", "n_rows", "d_coded_to", "d_coded_from", "number_of_dimensions", "d_y",
                                               "skip_energy", "flush"]
    assert sig(fs.FilterStream.push_host) == ["self", "xs", "rows", "flush"]
    assert sig(fs.FilterStream.push_coded_host) == ["self", "xs", "coded_to", "coded_from", "skip_energy", "flush"]
    for name in ("samples_received", "rows_received", "segments_done", "samples_committed", "pending_samples", "pending_rows"):
        assert sig(getattr(fs.FilterStream, name)) == ["self", "stream"]
    assert sig(fs.segments_done) == ["fs", "frame_period_ms", "n", "rows"] and sig(fs.committed) == ["fs", "frame_period_ms", "segments"]
    assert issubclass(fs.FilterStream, _binding._Handle) and sig(fs.FilterStream.close) == ["self"]
    assert fs.pack_rows is _binding.pack_rows and fs.split_rows is _binding.split_rows and fs.uploaded is _binding.uploaded
    assert fs._check is _binding._check and fs._binder is _binding._binder


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
    assert {"wc_frame_filter_run_device", "wc_frame_filter_run_coded_device", "wc_decode_spectral_envelope_device"} <= exported
