"""CPU tests of voice morphing's boundary: the headers declare wc_morph_parameters_device and
wc_synthesis_compute_coded_morphed_device with 21 arguments each, the Python signature tables list them with that arity, the mirror
functions exist with their parameter names, the existing signatures are unchanged, and the tree compiles for gfx950 without a GPU
and exports both symbols."""
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"wc_morph_parameters_device": ("world_class_io.h", 21), "wc_synthesis_compute_coded_morphed_device": ("world_class_c.h", 21)}


def declared_arity(header, symbol):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + symbol + r"\s*\(([^)]*)\)\s*;", src)
    assert m, "%s does not declare int %s(...)" % (header, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


def tables():
    import world_class_amd as w
    from world_class_amd import io
    return {"wc_morph_parameters_device": io.IO_SIGNATURES, "wc_synthesis_compute_coded_morphed_device": w._SIGNATURES}


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity(symbol):
    import ctypes as C
    header, arity = NEW[symbol]
    assert declared_arity(header, symbol) == arity
    res, args = tables()[symbol][symbol]
    assert res is C.c_int and len(args) == arity


def test_the_batch_symbol_is_in_exported_symbols():
    import world_class_amd as w
    assert "wc_synthesis_compute_coded_morphed_device" in w.EXPORTED_SYMBOLS


def test_mirror_functions_exist_with_their_parameter_names():
    from world_class_amd import Synthesis, io
    p = inspect.signature(io.morph_parameters_device).parameters
    assert list(p) == ["fs", "fft_size", "a_lengths", "d_f0_a", "d_sp_a", "d_ap_a", "b_lengths", "d_f0_b", "d_sp_b", "d_ap_b", "out_lengths",
                       "d_position_a", "d_position_b", "d_weight", "d_f0_weight", "d_ratio_a", "d_ratio_b", "d_f0_out", "d_sp_out", "d_ap_out"]
    assert all(p[k].default is None for k in ("d_f0_weight", "d_ratio_a", "d_ratio_b", "d_f0_out", "d_sp_out", "d_ap_out"))
    assert p["d_weight"].default is inspect.Parameter.empty
    p = inspect.signature(io.morph_parameters).parameters
    assert list(p) == ["a", "b", "position_a", "position_b", "weight", "fs", "fft_size", "f0_weight", "ratio_a", "ratio_b"]
    assert all(p[k].default is None for k in ("f0_weight", "ratio_a", "ratio_b"))
    p = inspect.signature(Synthesis.compute_coded_morphed_device).parameters
    assert list(p) == ["self", "d_f0_a", "a_lengths", "d_coded_sp_a", "d_coded_ap_a", "d_f0_b", "b_lengths", "d_coded_sp_b", "d_coded_ap_b",
                       "number_of_dimensions", "frames_out", "d_position_a", "d_position_b", "d_weight", "d_f0_weight", "d_ratio_a", "d_ratio_b",
                       "out_lengths", "d_out", "rng_pos"]
    assert p["rng_pos"].default is None


def test_existing_signatures_are_unchanged():
    from world_class_amd import Synthesis, codec, io
    assert list(inspect.signature(io.retime_parameters_device).parameters) == [
        "fs", "fft_size", "in_lengths", "d_f0_in", "d_sp_in", "d_ap_in", "out_lengths", "d_position", "d_f0_scale", "d_spectral_ratio", "d_f0_out",
        "d_sp_out", "d_ap_out"]
    assert list(inspect.signature(io.retime_parameters).parameters) == ["f0", "sp", "ap", "position", "fs", "fft_size", "f0_scale", "spectral_ratio"]
    assert list(inspect.signature(io.time_map).parameters) == ["n_frames", "speed"]
    assert list(inspect.signature(io.modify_parameters_frames_device).parameters) == [
        "fs", "fft_size", "n_frames", "d_f0", "d_sp", "d_f0_scale", "d_spectral_ratio"]
    assert list(inspect.signature(codec.decode_features_device).parameters) == [
        "fs", "fft_size", "n_frames", "number_of_dimensions", "d_coded_sp", "d_coded_ap", "d_sp", "d_ap"]
    assert list(inspect.signature(Synthesis.compute_device).parameters) == ["self", "d_f0", "f0_lengths", "d_sp", "d_ap", "out_lengths", "d_out", "rng_pos"]
    assert list(inspect.signature(Synthesis.compute_coded_device).parameters) == [
        "self", "d_f0", "f0_lengths", "d_coded_sp", "number_of_dimensions", "d_coded_ap", "out_lengths", "d_out", "rng_pos"]
    assert list(inspect.signature(Synthesis.compute_coded_retimed_device).parameters) == [
        "self", "d_f0", "f0_lengths", "d_coded_sp", "number_of_dimensions", "d_coded_ap", "frames_out", "d_position", "d_f0_scale",
        "d_spectral_ratio", "out_lengths", "d_out", "rng_pos"]
    for header, symbol, arity in (("world_class_io.h", "wc_modify_parameters_frames_device", 7), ("world_class_io.h", "wc_retime_parameters_device", 14),
                                  ("world_class_c.h", "wc_synthesis_compute_coded_device", 10), ("world_class_c.h", "wc_synthesis_compute_coded_modified_device", 11),
                                  ("world_class_c.h", "wc_synthesis_compute_coded_retimed_device", 14), ("world_class_c.h", "wc_synthesis_compute_device", 9)):
        assert declared_arity(header, symbol) == arity


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
