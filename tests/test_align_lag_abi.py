"""CPU tests of the boundary of the alignment streams' settled positions: include/world_class_align_lag.h (which
world_class_stream.h includes just below world_class_align_window.h) declares exactly the five wc_align_stream_* calls of the lag
with their arities, ALIGN_LAG_SIGNATURES lists them with that arity and their result types, is bound with the other three tables
and shares no symbol with them (whose sizes stay 46, 7 and 2), the mirror methods exist with their parameter names, and the tree
compiles for gfx950 without a GPU and exports the five symbols."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "world_class_align_lag.h"
# symbol: (arity, what the header declares in front of it, the table's result type)
NEW = {
    "wc_align_stream_reserve_lag": (2, r"int\s+", C.c_int),
    "wc_align_stream_set_lag": (3, r"int\s+", C.c_int),
    "wc_align_stream_get_lag": (2, r"int\s+", C.c_int),
    "wc_align_stream_push_settled_device": (6, r"int\s+", C.c_int),
    "wc_align_stream_tail_device": (3, r"int\s+", C.c_int),
}


def _source(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_arity(symbol, result, header=HEADER):
    m = re.search(r"^\s*" + result + symbol + r"\s*\(([^)]*)\)\s*;", _source(header), flags=re.M)
    assert m, "%s does not declare %s(...) with that result" % (header, symbol)
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("symbol", sorted(NEW))
def test_header_declares_and_table_lists_with_matching_arity_and_result(symbol):
    from world_class_amd.stream import ALIGN_LAG_SIGNATURES
    arity, result, ctype = NEW[symbol]
    assert declared_arity(symbol, result) == arity
    res, args = ALIGN_LAG_SIGNATURES[symbol]
    assert res is ctype and len(args) == arity and args[0] is C.c_void_p  # (the handle)


def test_the_table_is_the_header_and_disjoint_from_the_other_three():
    from world_class_amd.stream import ALIGN_LAG_SIGNATURES, ALIGN_STREAM_SIGNATURES, ALIGN_WINDOW_SIGNATURES, STREAM_SIGNATURES
    declared = sorted(set(re.findall(r"\b(wc_[a-z0-9_]+)\s*\(", _source(HEADER))))
    assert declared == sorted(ALIGN_LAG_SIGNATURES) == sorted(NEW)
    assert not set(ALIGN_LAG_SIGNATURES) & (set(STREAM_SIGNATURES) | set(ALIGN_STREAM_SIGNATURES) | set(ALIGN_WINDOW_SIGNATURES))
    assert len(STREAM_SIGNATURES) == 46 and len(ALIGN_STREAM_SIGNATURES) == 7 and len(ALIGN_WINDOW_SIGNATURES) == 2


def test_the_stream_header_includes_it_below_the_windows():
    lines = [l.strip() for l in _source("world_class_stream.h").splitlines() if l.strip().startswith("#include")]
    assert '#include "%s"' % HEADER in lines
    assert lines.index('#include "%s"' % HEADER) == lines.index('#include "world_class_align_window.h"') + 1
    from world_class_amd import build
    assert os.path.join(ROOT, "include", HEADER) in build.headers()


def test_argument_types_and_binding():
    from world_class_amd import stream
    ip, vp = C.POINTER(C.c_int), C.c_void_p
    S = stream.ALIGN_LAG_SIGNATURES
    assert S["wc_align_stream_reserve_lag"][1] == [vp, C.c_int]
    assert S["wc_align_stream_set_lag"][1] == [vp, C.c_int, C.c_int]
    assert S["wc_align_stream_get_lag"][1] == [vp, C.c_int]
    assert S["wc_align_stream_push_settled_device"][1] == [vp, ip, vp, vp, vp, vp]
    assert S["wc_align_stream_tail_device"][1] == [vp, ip, vp]
    L = stream._lib()
    for name, (res, args) in S.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_mirror_methods_exist_with_their_parameter_names():
    from world_class_amd.stream import AlignStream
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(AlignStream.reserve_lag) == ["self", "max_lag"]
    assert names(AlignStream.set_lag) == ["self", "stream", "lag"]
    assert names(AlignStream.get_lag) == ["self", "stream"]
    assert names(AlignStream.push_settled_device) == ["self", "n_rows", "d_feat", "d_position", "d_cost", "d_settled"]
    assert names(AlignStream.push_settled) == ["self", "rows"]
    assert names(AlignStream.tail) == ["self", "streams"]
    assert inspect.signature(AlignStream.tail).parameters["streams"].default is None
    assert names(AlignStream.push_device) == ["self", "n_rows", "d_feat", "d_position", "d_cost"] and names(AlignStream.push) == ["self", "rows"]


def test_tree_compiles_for_gfx950_and_exports_the_symbols():
    from world_class_amd import build
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = set(re.findall(r" T (wc_[a-z0-9_]+)", out))
    assert set(NEW) <= exported
