"""CPU tests of the per-frame modification's boundary: the headers declare wc_modify_parameters_frames_device,
wc_decode_features_modified_device, wc_synthesis_compute_coded_modified_device and wc_synth_stream_set_modification, the Python
signature tables list them with the arity of the declarations, the mirror functions exist with their parameter names, and the
tree compiles for gfx950 without a GPU and exports the symbols."""
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wc_modify_parameters_frames_device": ("world_class_io.h", 7), "wc_decode_features_modified_device": ("world_class_codec.h", 9),
       "wc_synthesis_compute_coded_modified_device": ("world_class_c.h", 11), "wc_synth_stream_set_modification": ("world_class_stream.h", 4)}


def declared_arity(header, symbol):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + symbol + r"\s*\(([^)]*)\)\s*;", src)
    assert m, "%s does not declare int %s(...)" % (header, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


def tables():
    import world_class_amd as w
    from world_class_amd import codec, io, stream
    return {"wc_modify_parameters_frames_device": io.IO_SIGNATURES, "wc_decode_features_modified_device": codec.CODEC_SIGNATURES,
            "wc_synthesis_compute_coded_modified_device": w._SIGNATURES, "wc_synth_stream_set_modification": stream.STREAM_SIGNATURES}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity(symbol):
    import ctypes as C
    header, arity = NEW[symbol]
    assert declared_arity(header, symbol) == arity
    res, args = tables()[symbol][symbol]
    assert res is C.c_int and len(args) == arity


def test_the_batch_symbol_is_in_exported_symbols():
    import world_class_amd as w
    assert "wc_synthesis_compute_coded_modified_device" in w.EXPORTED_SYMBOLS


def test_mirror_functions_exist_with_their_parameter_names():
    from world_class_amd import Synthesis, codec, io
    from world_class_amd.stream import StreamSynthesizer
    p = inspect.signature(io.modify_parameters_frames_device).parameters
    assert list(p) == ["fs", "fft_size", "n_frames", "d_f0", "d_sp", "d_f0_scale", "d_spectral_ratio"]
    assert p["d_f0_scale"].default is None and p["d_spectral_ratio"].default is None
    assert list(inspect.signature(codec.decode_features_modified_device).parameters) == [
        "fs", "fft_size", "n_frames", "number_of_dimensions", "d_coded_sp", "d_coded_ap", "d_spectral_ratio", "d_sp", "d_ap"]
    p = inspect.signature(Synthesis.compute_coded_modified_device).parameters
    assert list(p) == ["self", "d_f0", "f0_lengths", "d_coded_sp", "number_of_dimensions", "d_coded_ap", "d_spectral_ratio", "out_lengths",
                       "d_out", "rng_pos"]
    assert p["rng_pos"].default is None
    p = inspect.signature(StreamSynthesizer.set_modification).parameters
    assert list(p) == ["self", "stream", "f0_scale", "spectral_ratio"]
    assert p["f0_scale"].default == 1.0 and p["spectral_ratio"].default == 0.0


def test_existing_signatures_are_unchanged():
    from world_class_amd import Synthesis, codec, io
    from world_class_amd.stream import StreamSynthesizer
    assert list(inspect.signature(io.modify_parameters_device).parameters) == ["fs", "fft_size", "n_frames", "d_f0", "d_sp", "f0_scale", "spectral_ratio"]
    assert list(inspect.signature(codec.decode_features_device).parameters) == [
        "fs", "fft_size", "n_frames", "number_of_dimensions", "d_coded_sp", "d_coded_ap", "d_sp", "d_ap"]
    assert list(inspect.signature(Synthesis.compute_coded_device).parameters) == [
        "self", "d_f0", "f0_lengths", "d_coded_sp", "number_of_dimensions", "d_coded_ap", "out_lengths", "d_out", "rng_pos"]
    assert list(inspect.signature(StreamSynthesizer.push_coded_device).parameters) == [
        "self", "n_frames", "d_f0", "d_coded_sp", "number_of_dimensions", "d_coded_ap", "flush", "d_y"]
    assert list(inspect.signature(StreamSynthesizer.push_device).parameters) == ["self", "n_frames", "d_f0", "d_sp", "d_ap", "flush", "d_y"]


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
