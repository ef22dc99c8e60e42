"""What every module of the mirror shares, stated once: the binder of a module's signature tables, the handle base (create, close,
__del__), what the two lagged row streams share, the sample formats, and the packing of per-stream rows around a push.

The import cycle with the package is cut on the package's side: world_class_amd/__init__.py defines lib, _check, _handle, _ints and
DeviceArray above the line that imports this module, so the import below finds them in the half-initialised package."""
import contextlib
import ctypes as C

import numpy as np

from . import DeviceArray, _check, _handle, _ints, lib

IN_FORMATS = {"f64": (0, np.float64), "i16": (1, np.int16), "f32": (2, np.float32)}
OUT_FORMATS = {"f64": (0, np.float64), "i16": (1, np.int16)}


def _binder(*signatures):
    """the library with a module's signatures (one table or several) bound on first use"""
    done = []

    def get():
        L = lib()
        if not done:
            for table in signatures:
                for name, (res, args) in table.items():
                    fn = getattr(L, name)
                    fn.restype = res
                    fn.argtypes = args
            done.append(True)
        return L

    return get


def _count(n):
    if n < 0:
        _check(int(n))
    return int(n)


class _Handle:
    """a handle of the library: _lib is its module's binder, _sym the prefix of its symbols, _kind what follows the prefix in the
    names of its create and destroy (nothing, for most)"""
    _lib = None
    _sym = None
    _kind = ""
    _h = None

    def _fn(self, name):
        return getattr(self._lib(), self._sym + name)

    def _create(self, *args):
        self._h = _handle(self._fn(self._kind + "_create")(*args))

    def close(self):
        if self._h:
            self._fn(self._kind + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _LagStream(_Handle):
    """what the two lagged row streams share (csrc/wc_lag_stream.hpp): MlpgStream and FeatureStream"""
    _kind = "_stream"
    n_streams = 0

    @property
    def max_frames_per_push(self):
        return int(self._fn("_stream_max_frames_per_push")(self._h))

    @property
    def max_frames_per_flush(self):
        return int(self._fn("_stream_max_frames_per_flush")(self._h))

    def _counts(self, counts):
        if len(counts) != self.n_streams:
            raise ValueError("one entry per stream")
        return _ints(counts), (C.c_int * self.n_streams)()

    def rows_received(self, stream):
        return int(self._fn("_stream_rows_received")(self._h, int(stream)))

    def frames_emitted(self, stream):
        return int(self._fn("_stream_frames_emitted")(self._h, int(stream)))

    def get_lag(self, stream):
        return int(self._fn("_stream_get_lag")(self._h, int(stream)))


def _lag_emitted(binder, symbol, doc):
    """a module's emitted(rows, lag), bound to its library symbol"""
    def emitted(rows, lag):
        n = int(getattr(binder(), symbol)(int(rows), int(lag)))
        if n < 0:
            raise ValueError("rows and lag must not be negative")
        return n

    emitted.__doc__ = doc
    return emitted


def pack_rows(parts, width, dtype=np.float64, placeholder=True):
    """parts[u]: None, empty, or k_u rows of `width` values -> (counts, flat): counts[u] = k_u, flat the C-contiguous concatenation
    [sum, width] ([sum] where width is 1 and the parts came as vectors).  Nothing at all: one row of zeros (placeholder) or None"""
    rows = []
    for p in parts:
        a = np.zeros(0, dtype=dtype) if p is None else np.asarray(p, dtype=dtype)
        if a.size and a.ndim == 2 and a.shape[1] != width:
            raise ValueError(f"rows of {width} values")
        rows.append(a.reshape(-1, width))  # (raises for a vector that is no whole number of rows)
    counts = [len(a) for a in rows]
    vector = width == 1 and all(p is None or np.ndim(p) < 2 for p in parts)
    if sum(counts):
        flat = np.concatenate(rows)
    elif placeholder:
        flat = np.zeros((1, width), dtype=dtype)
    else:
        return counts, None
    return counts, flat.reshape(-1) if vector else flat


def split_rows(flat, counts, width=None):
    """the first sum(counts) rows of flat (width given: rows of `width` of its values) cut by counts: one copy per stream, since the
    caller's staging array is written again by the next push"""
    tot = int(sum(counts))
    flat = np.asarray(flat)
    rows = flat[:tot] if width is None else flat.reshape(-1)[:tot * width].reshape(tot, width)
    return [rows[e - c:e].copy() for c, e in zip(counts, np.cumsum(counts))]


@contextlib.contextmanager
def uploaded(*host_arrays, dtype=np.float64):
    """the host arrays as DeviceArrays (None stays None), freed on exit -- on an error as well"""
    held = []
    try:
        for a in host_arrays:
            held.append(None if a is None else DeviceArray.from_host(a, dtype=dtype))
        yield tuple(held)
    finally:
        for d in held:
            if d is not None:
                d.free()
