"""world_class_amd/_binding.py without a device and without the library: the row packing, the handle base against a fake library, the
binder over fake tables, and the twelve handle classes of the mirror."""
import types

import numpy as np
import pytest

import world_class_amd as w
from world_class_amd import _binding as B
from world_class_amd import gmm, gmm_train, stream

# ---- pack_rows / split_rows ---------------------------------------------------------------------------------------------------


def _parts(counts, width, dtype, empty):
    rng = np.random.default_rng(len(counts) * 1000 + width)
    out = []
    for k in counts:
        if k == 0:
            out.append(None if empty == "none" else np.zeros((0, width), dtype=dtype))
        else:
            out.append(rng.integers(-30000, 30000, size=(k, width)).astype(dtype))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
@pytest.mark.parametrize("width", [1, 3, 513])
@pytest.mark.parametrize("counts", [[0, 3, 0, 1], [0, 0], [5]])
def test_pack_and_split_round_trip(counts, width, dtype):
    parts = _parts(counts, width, dtype, "none")
    got_counts, flat = B.pack_rows(parts, width, dtype=dtype)
    same_counts, same = B.pack_rows(_parts(counts, width, dtype, "zero-length"), width, dtype=dtype)
    assert got_counts == counts == same_counts and np.array_equal(flat.ravel(), same.ravel())  # (None and a zero-length entry are one thing)
    assert flat.dtype == dtype and flat.flags.c_contiguous
    if sum(counts) == 0:
        # (one row of zeros; width 1 with nothing but None is a push of vectors, with [0, 1] arrays one of rows)
        assert flat.shape == ((1,) if width == 1 else (1, width)) and same.shape == (1, width) and not flat.any()
        assert B.pack_rows(parts, width, dtype=dtype, placeholder=False) == (counts, None)
        assert [p.shape for p in B.split_rows(flat, counts, width)] == [(0, width)] * len(counts)
        return
    assert flat.shape == (sum(counts), width)
    assert B.pack_rows(parts, width, dtype=dtype, placeholder=False)[1].shape == flat.shape
    back = B.split_rows(flat, counts, width)
    assert len(back) == len(counts)
    for k, p, b in zip(counts, parts, back):
        assert b.shape == (k, width) and b.dtype == dtype
        assert np.array_equal(b, p if k else np.zeros((0, width)))
    # the same values as one flat staging array that is longer than what the push wrote
    staging = np.concatenate([flat.ravel(), np.full(7, 99, dtype=dtype)])
    for b, c in zip(back, B.split_rows(staging, counts, width)):
        assert np.array_equal(b, c)


def test_vectors_of_width_1_stay_vectors():
    counts, flat = B.pack_rows([np.arange(3.0), None, [], [7.0]], 1)
    assert counts == [3, 0, 0, 1] and flat.shape == (4,) and flat.tolist() == [0.0, 1.0, 2.0, 7.0]
    assert B.pack_rows([None, []], 1)[1].shape == (1,)
    assert B.pack_rows([np.zeros((2, 1))], 1)[1].shape == (2, 1)
    assert [v.tolist() for v in B.split_rows(flat, counts)] == [[0.0, 1.0, 2.0], [], [], [7.0]]


def test_a_vector_of_whole_rows_is_taken_as_rows():
    counts, flat = B.pack_rows([np.arange(6.0), np.zeros(0)], 3)
    assert counts == [2, 0] and flat.tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]


@pytest.mark.parametrize("bad", [np.zeros((2, 4)), np.zeros((3, 4)), np.zeros(4)])
def test_a_row_of_another_width_raises(bad):
    with pytest.raises(ValueError):
        B.pack_rows([np.zeros((1, 3)), bad], 3)


def test_split_rows_returns_copies_and_ignores_the_rest():
    flat = np.arange(12.0)
    vectors = B.split_rows(flat, [2, 0, 3])
    rows = B.split_rows(flat, [1, 2], 3)
    want_vectors, want_rows = [[0.0, 1.0], [], [2.0, 3.0, 4.0]], [[[0.0, 1.0, 2.0]], [[3.0, 4.0, 5.0], [6.0, 7.0, 8.0]]]
    assert [v.tolist() for v in vectors] == want_vectors and [v.tolist() for v in rows] == want_rows
    flat[:] = -1.0  # (the next push writes the staging array again)
    assert [v.tolist() for v in vectors] == want_vectors and [v.tolist() for v in rows] == want_rows
    assert all(not np.shares_memory(v, flat) for v in vectors + rows)
    with pytest.raises(ValueError):
        B.split_rows(np.arange(5.0), [1, 1], 3)  # (fewer values than the counts name)


# ---- _Handle against a fake library -------------------------------------------------------------------------------------------


def _fake(create=7, destroy=None):
    destroyed = []

    def fake_destroy(h):
        destroyed.append(h)
        if destroy is not None:
            raise destroy

    L = types.SimpleNamespace(wc_fake_create=lambda *a: create, wc_fake_destroy=fake_destroy)

    class Fake(B._Handle):
        _lib = staticmethod(lambda: L)
        _sym = "wc_fake"

        def __init__(self):
            self._create(1, 2)

    return Fake, destroyed


def test_close_close_del_destroys_once():
    Fake, destroyed = _fake()
    h = Fake()
    assert h._h == 7 and h._fn("_create") is h._lib().wc_fake_create
    h.close()
    assert h._h is None and destroyed == [7]
    h.close()
    h.__del__()
    assert h._h is None and destroyed == [7]


def test_a_destroy_that_raises_passes_close_and_not_del():
    Fake, destroyed = _fake(destroy=OSError("gone"))
    h = Fake()
    with pytest.raises(OSError):
        h.close()
    h.__del__()  # (swallowed)
    assert destroyed == [7, 7]


def test_a_create_that_returns_null_raises(monkeypatch):
    monkeypatch.setattr(w, "last_error", lambda: "no such thing")
    Fake, destroyed = _fake(create=0)
    with pytest.raises(w.WorldClassError, match="no such thing"):
        Fake()
    assert destroyed == []


# ---- _binder over fake tables -------------------------------------------------------------------------------------------------


def test_binder_binds_every_entry_of_every_table_once(monkeypatch):
    names = ["a", "b", "c"]
    L = types.SimpleNamespace(**{n: types.SimpleNamespace(restype="unset", argtypes="unset") for n in names})
    loads = []
    monkeypatch.setattr(B, "lib", lambda: loads.append(1) or L)
    first, second = {"a": (int, [int]), "b": (None, [])}, {"c": (float, [int, float])}
    get = B._binder(first, second)
    assert not loads and L.a.restype == "unset"  # (nothing happens before the first use)
    assert get() is L
    for n, (res, args) in {**first, **second}.items():
        assert getattr(L, n).restype is res and getattr(L, n).argtypes is args
    for n in names:
        getattr(L, n).restype = "touched"
    assert get() is L and [getattr(L, n).restype for n in names] == ["touched"] * 3
    one = B._binder(second)
    assert one() is L and L.c.restype is float and L.a.restype == "touched"


def test_binder_raises_for_a_symbol_the_library_lacks(monkeypatch):
    monkeypatch.setattr(B, "lib", lambda: types.SimpleNamespace(a=types.SimpleNamespace()))
    with pytest.raises(AttributeError):
        B._binder({"a": (None, [])}, {"missing": (None, [])})()


# ---- the handle classes of the mirror -----------------------------------------------------------------------------------------

_STREAM_TABLES = (stream.STREAM_SIGNATURES, stream.ALIGN_STREAM_SIGNATURES, stream.ALIGN_WINDOW_SIGNATURES, stream.ALIGN_LAG_SIGNATURES,
                  stream.TRACK_MORPH_SIGNATURES, stream.TRACK_MORPH_CODED_SIGNATURES)
_STREAM_SYMBOLS = {name for table in _STREAM_TABLES for name in table}
# the class, the classes that carry its symbol prefix (itself, but for the base of the two track-morph classes), its module's symbols
HANDLES = [(w.CheapTrick, None, w._SIGNATURES), (w.D4C, None, w._SIGNATURES), (w.Synthesis, None, w._SIGNATURES),
           (w.Harvest, None, w._SIGNATURES), (w.Pipeline, None, w._SIGNATURES), (gmm.Gmm, None, gmm.GMM_SIGNATURES),
           (gmm_train.GmmTrainer, None, gmm_train.GMM_TRAIN_SIGNATURES), (stream.StreamAnalyzer, None, _STREAM_SYMBOLS),
           (stream.StreamSynthesizer, None, _STREAM_SYMBOLS), (stream.MorphStream, None, _STREAM_SYMBOLS),
           (stream.AlignStream, None, _STREAM_SYMBOLS), (stream._TrackMorphBase, (stream.TrackMorph, stream.CodedTrackMorph), _STREAM_SYMBOLS)]


@pytest.mark.parametrize("cls,concrete,symbols", HANDLES, ids=[h[0].__name__ for h in HANDLES])
def test_every_handle_class_derives_from_the_base_and_names_its_symbols(cls, concrete, symbols):
    assert issubclass(cls, B._Handle) and "__del__" not in vars(cls)
    assert cls.close is not None and cls.__del__ is B._Handle.__del__
    for c in concrete or (cls,):
        assert issubclass(c, cls) and "__del__" not in vars(c)
        assert c._sym and c._lib is not None
        create, destroy = c._sym + c._kind + "_create", c._sym + c._kind + "_destroy"
        assert create in symbols and destroy in symbols


def test_the_moved_names_stay_importable_from_resample():
    from world_class_amd import resample
    for name in ("_binder", "_Handle", "_LagStream", "_lag_emitted", "_count", "IN_FORMATS", "OUT_FORMATS"):
        assert getattr(resample, name) is getattr(B, name)
    assert stream._opt is w._opt
    from world_class_amd import codec, io
    assert codec._rows is w._rows and io._rows is w._rows


def test_the_stream_tables_keep_their_sizes():
    assert [len(t) for t in _STREAM_TABLES] == [46, 7, 2, 5, 13, 14]
