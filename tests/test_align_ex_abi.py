"""CPU tests of extended feature alignment's boundary: the header declares wc_align_features_ex_device with 19 arguments and the two
flags, the Python signature table lists it with that arity, the two mirror functions exist with their parameter names and
defaults, the mirrors of the plain call are unchanged, and the tree compiles for gfx950 without a GPU and exports the symbol."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL, OLD_SYMBOL, HEADER, ARITY = "wc_align_features_ex_device", "wc_align_features_device", "world_class_io.h", 19


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
    assert [a is C.c_int for a in args] == [True, False, False, False, False] + [True] * 6 + [False] * 8
    assert declared_arity(HEADER, OLD_SYMBOL) == 14 and len(io.IO_SIGNATURES[OLD_SYMBOL][1]) == 14


def test_header_defines_the_flags_and_python_exports_them():
    from world_class_amd import io
    src = open(os.path.join(ROOT, "include", HEADER)).read()
    defs = dict(re.findall(r"^#define\s+(WC_ALIGN_OPEN_\w+)\s+(\d+)", src, flags=re.M))
    assert defs == {"WC_ALIGN_OPEN_BEGIN": "1", "WC_ALIGN_OPEN_END": "2"}
    assert (io.ALIGN_OPEN_BEGIN, io.ALIGN_OPEN_END) == (1, 2)


def test_mirror_functions_exist_with_their_parameter_names_and_defaults():
    from world_class_amd import io
    p = inspect.signature(io.align_features_ex_device).parameters
    assert list(p) == ["a_lengths", "d_feat_a", "b_lengths", "d_feat_b", "dims", "dim_begin", "dim_end", "band", "step_pattern", "flags", "d_cost",
                       "d_path_length", "d_path", "d_b_on_a", "d_a_on_b", "d_span", "d_timeline_a", "d_timeline_b"]
    assert all(p[k].default is None for k in ("d_path", "d_b_on_a", "d_a_on_b", "d_span", "d_timeline_a", "d_timeline_b"))
    assert all(p[k].default is inspect.Parameter.empty for k in ("step_pattern", "flags", "d_cost", "d_path_length"))
    p = inspect.signature(io.align_features_ex).parameters
    assert list(p) == ["feat_a", "feat_b", "dim_begin", "dim_end", "band", "step_pattern", "open_begin", "open_end"]
    assert [p[k].default for k in list(p)[2:]] == [1, None, 0, 0, False, False]


def test_the_mirrors_of_the_plain_call_are_unchanged():
    from world_class_amd import io
    p = inspect.signature(io.align_features_device).parameters
    assert list(p) == ["a_lengths", "d_feat_a", "b_lengths", "d_feat_b", "dims", "dim_begin", "dim_end", "band", "d_cost", "d_path_length",
                       "d_path", "d_b_on_a", "d_a_on_b"]
    assert all(p[k].default is None for k in ("d_path", "d_b_on_a", "d_a_on_b"))
    p = inspect.signature(io.align_features).parameters
    assert list(p) == ["feat_a", "feat_b", "dim_begin", "dim_end", "band"]
    assert (p["dim_begin"].default, p["dim_end"].default, p["band"].default) == (1, None, 0)


def test_tree_compiles_for_gfx950_and_exports_the_symbol():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert SYMBOL in exported and OLD_SYMBOL in exported
