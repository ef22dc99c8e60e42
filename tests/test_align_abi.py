"""CPU tests of feature alignment's boundary: the header declares wc_align_features_device with 14 arguments, the Python signature
table lists it with that arity, the two mirror functions exist with their parameter names, the existing io signatures are unchanged,
and the tree compiles for gfx950 without a GPU and exports the symbol."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL, HEADER, ARITY = "wc_align_features_device", "world_class_io.h", 14


def declared_arity(header, symbol):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + symbol + r"\s*\(([^)]*)\)\s*;", src)
    assert m, "%s does not declare int %s(...)" % (header, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_and_table_lists_with_matching_arity():
    import ctypes as C
    from world_class_amd import io
    assert declared_arity(HEADER, SYMBOL) == ARITY
    res, args = io.IO_SIGNATURES[SYMBOL]
    assert res is C.c_int and len(args) == ARITY
    assert [a is C.c_int for a in args] == [True, False, False, False, False, True, True, True, True] + [False] * 5


def test_mirror_functions_exist_with_their_parameter_names():
    from world_class_amd import io
    p = inspect.signature(io.align_features_device).parameters
    assert list(p) == ["a_lengths", "d_feat_a", "b_lengths", "d_feat_b", "dims", "dim_begin", "dim_end", "band", "d_cost", "d_path_length",
                       "d_path", "d_b_on_a", "d_a_on_b"]
    assert all(p[k].default is None for k in ("d_path", "d_b_on_a", "d_a_on_b"))
    assert p["d_path_length"].default is inspect.Parameter.empty
    p = inspect.signature(io.align_features).parameters
    assert list(p) == ["feat_a", "feat_b", "dim_begin", "dim_end", "band"]
    assert (p["dim_begin"].default, p["dim_end"].default, p["band"].default) == (1, None, 0)


def test_existing_io_signatures_are_unchanged():
    from world_class_amd import io
    assert list(inspect.signature(io.retime_parameters_device).parameters) == [
        "fs", "fft_size", "in_lengths", "d_f0_in", "d_sp_in", "d_ap_in", "out_lengths", "d_position", "d_f0_scale", "d_spectral_ratio", "d_f0_out",
        "d_sp_out", "d_ap_out"]
    assert list(inspect.signature(io.retime_parameters).parameters) == ["f0", "sp", "ap", "position", "fs", "fft_size", "f0_scale", "spectral_ratio"]
    assert list(inspect.signature(io.time_map).parameters) == ["n_frames", "speed"]
    assert list(inspect.signature(io.modify_parameters_frames_device).parameters) == [
        "fs", "fft_size", "n_frames", "d_f0", "d_sp", "d_f0_scale", "d_spectral_ratio"]
    assert list(inspect.signature(io.morph_parameters_device).parameters) == [
        "fs", "fft_size", "a_lengths", "d_f0_a", "d_sp_a", "d_ap_a", "b_lengths", "d_f0_b", "d_sp_b", "d_ap_b", "out_lengths", "d_position_a",
        "d_position_b", "d_weight", "d_f0_weight", "d_ratio_a", "d_ratio_b", "d_f0_out", "d_sp_out", "d_ap_out"]
    assert list(inspect.signature(io.morph_parameters).parameters) == [
        "a", "b", "position_a", "position_b", "weight", "fs", "fft_size", "f0_weight", "ratio_a", "ratio_b"]
    for symbol, arity in (("wc_modify_parameters_frames_device", 7), ("wc_retime_parameters_device", 14), ("wc_morph_parameters_device", 21)):
        assert declared_arity(HEADER, symbol) == arity
        assert len(io.IO_SIGNATURES[symbol][1]) == arity


def test_tree_compiles_for_gfx950_and_exports_the_symbol():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert SYMBOL in set(re.findall(r" T (wc_[a-z0-9_]+)", out))
