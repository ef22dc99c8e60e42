"""CPU tests of the device-side feature coder's boundary: the three headers declare wc_code_features_device,
wc_pipeline_run_coded_device and wc_stream_push_coded_device, the Python signature tables list them with the arity of the
declarations, the mirror methods exist, and the tree compiles for gfx950 without a GPU and exports the symbols."""
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wc_code_features_device": "world_class_codec.h", "wc_pipeline_run_coded_device": "world_class_c.h",
       "wc_stream_push_coded_device": "world_class_stream.h"}


def declared_arity(header, symbol):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + symbol + r"\s*\(([^)]*)\)\s*;", src)
    assert m, "%s does not declare int %s(...)" % (header, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


def tables():
    import world_class_amd as w
    from world_class_amd import codec, stream
    return {"wc_code_features_device": codec.CODEC_SIGNATURES, "wc_pipeline_run_coded_device": w._SIGNATURES,
            "wc_stream_push_coded_device": stream.STREAM_SIGNATURES}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity(symbol):
    import ctypes as C
    n = declared_arity(NEW[symbol], symbol)
    assert n == {"wc_code_features_device": 8, "wc_pipeline_run_coded_device": 11, "wc_stream_push_coded_device": 11}[symbol]
    res, args = tables()[symbol][symbol]
    assert res is C.c_int and len(args) == n


def test_mirror_methods_exist():
    from world_class_amd import Pipeline, codec
    from world_class_amd.stream import StreamAnalyzer
    assert list(inspect.signature(codec.code_features_device).parameters) == [
        "fs", "fft_size", "n_frames", "number_of_dimensions", "d_sp", "d_ap", "d_coded_sp", "d_coded_ap"]
    p = list(inspect.signature(Pipeline.run_coded_device).parameters)
    assert p[:9] == ["self", "d_x", "x_lengths", "d_tpos", "d_f0", "d_coded_sp", "number_of_dimensions", "d_coded_ap", "d_y"] and p[9] == "rng_pos"
    assert callable(StreamAnalyzer.push_coded_device)
    q = inspect.signature(StreamAnalyzer.push_coded).parameters
    assert list(q)[:2] == ["self", "chunks"] and q["number_of_dimensions"].default == 60 and q["flush"].default is None
    assert "coded" in inspect.signature(StreamAnalyzer.run_whole).parameters


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    assert "wc_code_features.hip" in build.sources()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
