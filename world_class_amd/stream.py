"""Chunked Harvest + CheapTrick, and chunked Synthesis, for many concurrent streams: Python mirror of include/world_class_stream.h (the semantics
are stated there; the reference itself has no streaming mode, reference src/harvest.cpp:431-440, :676-703 are non-causal)."""
import ctypes as C

import numpy as np

from . import DeviceArray, _check, _ints, _opt, _ptr, lib
from ._binding import IN_FORMATS, _binder, _count, _Handle, pack_rows, split_rows, uploaded

_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

STREAM_SIGNATURES = {
    "wc_stream_create": (_vp, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]),
    "wc_stream_destroy": (None, [_vp]),
    "wc_stream_set_incremental": (C.c_int, [_vp, C.c_int]),
    "wc_stream_get_fft_size": (C.c_int, [_vp]),
    "wc_stream_chunk_samples": (C.c_int, [_vp]),
    "wc_stream_max_frames_per_push": (C.c_int, [_vp]),
    "wc_stream_reset": (C.c_int, [_vp, C.c_int]),
    "wc_stream_push_device": (C.c_int, [_vp, _vp, _ip, _ip, _vp, _vp, _vp, _ip]),
    "wc_stream_push_device_fmt": (C.c_int, [_vp, _vp, C.c_int, _ip, _ip, _vp, _vp, _vp, _ip]),
    "wc_stream_rng_position": (C.c_ulonglong, [_vp, C.c_int]),
    "wc_stream_set_rng_position": (C.c_int, [_vp, C.c_int, C.c_ulonglong]),
    "wc_stream_frames_committed": (C.c_longlong, [_vp, C.c_int]),
    "wc_stream_samples_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_stream_set_aperiodicity": (C.c_int, [_vp, C.c_double]),
    "wc_stream_push_device_ex": (C.c_int, [_vp, _vp, C.c_int, _ip, _ip, _vp, _vp, _vp, _vp, _ip]),
    "wc_stream_push_coded_device": (C.c_int, [_vp, _vp, C.c_int, _ip, _ip, _vp, _vp, _vp, C.c_int, _vp, _ip]),
    "wc_stream_d4c_rng_position": (C.c_ulonglong, [_vp, C.c_int]),
    "wc_stream_set_d4c_rng_position": (C.c_int, [_vp, C.c_int, C.c_ulonglong]),
    "wc_synth_stream_create": (_vp, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]),
    "wc_synth_stream_destroy": (None, [_vp]),
    "wc_synth_stream_max_samples_per_push": (C.c_int, [_vp]),
    "wc_synth_stream_reset": (C.c_int, [_vp, C.c_int]),
    "wc_synth_stream_push_device": (C.c_int, [_vp, _ip, _ip, _vp, _vp, _vp, _vp, _ip]),
    "wc_synth_stream_push_coded_device": (C.c_int, [_vp, _ip, _ip, _vp, _vp, C.c_int, _vp, _vp, _ip]),
    "wc_synth_stream_set_modification": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "wc_synth_stream_rng_position": (C.c_ulonglong, [_vp, C.c_int]),
    "wc_synth_stream_set_rng_position": (C.c_int, [_vp, C.c_int, C.c_ulonglong]),
    "wc_synth_stream_frames_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_synth_stream_samples_committed": (C.c_longlong, [_vp, C.c_int]),
    "wc_synth_stream_set_speed": (C.c_int, [_vp, C.c_int, C.c_double]),
    "wc_synth_stream_source_position": (C.c_double, [_vp, C.c_int]),
    "wc_synth_stream_frames_synthesised": (C.c_longlong, [_vp, C.c_int]),
    "wc_synth_stream_frames_for_push": (C.c_int, [_vp, C.c_int, C.c_int]),
    "wc_morph_stream_create": (_vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wc_morph_stream_destroy": (None, [_vp]),
    "wc_morph_stream_reset": (C.c_int, [_vp, C.c_int]),
    "wc_morph_stream_set_speeds": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "wc_morph_stream_set_weight": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "wc_morph_stream_set_ratios": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "wc_morph_stream_frames_for_push": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "wc_morph_stream_push_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp, _ip, _vp, _vp, _vp, _vp, _vp, _vp, _ip]),
    "wc_morph_stream_push_coded_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp, _ip, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _ip]),
    "wc_morph_stream_source_position": (C.c_double, [_vp, C.c_int, C.c_int]),
    "wc_morph_stream_frames_received": (C.c_longlong, [_vp, C.c_int, C.c_int]),
    "wc_morph_stream_backlog": (C.c_int, [_vp, C.c_int, C.c_int]),
    "wc_morph_stream_frames_formed": (C.c_longlong, [_vp, C.c_int]),
}
# the alignment streams (include/world_class_align_stream.h, which world_class_stream.h includes): a table of their own, bound with
# the one above
ALIGN_STREAM_SIGNATURES = {
    "wc_align_stream_create": (_vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wc_align_stream_destroy": (None, [_vp]),
    "wc_align_stream_set_track_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "wc_align_stream_reset": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "wc_align_stream_push_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp]),
    "wc_align_stream_rows_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_align_stream_track_length": (C.c_int, [_vp, C.c_int]),
}
# the search window of an alignment stream (include/world_class_align_window.h, included just below the header above): again a
# table of its own
ALIGN_WINDOW_SIGNATURES = {
    "wc_align_stream_set_window": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wc_align_stream_get_window": (C.c_int, [_vp, C.c_int, _ip, _ip, _ip, _ip]),
}
ALIGN_WINDOW_MONOTONE = 1
# settled positions from a lagged backtrack (include/world_class_align_lag.h, included below the window's header): a fourth table
ALIGN_LAG_SIGNATURES = {
    "wc_align_stream_reserve_lag": (C.c_int, [_vp, C.c_int]),
    "wc_align_stream_set_lag": (C.c_int, [_vp, C.c_int, C.c_int]),
    "wc_align_stream_get_lag": (C.c_int, [_vp, C.c_int]),
    "wc_align_stream_push_settled_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp, _vp]),
    "wc_align_stream_tail_device": (C.c_int, [_vp, _ip, _vp]),
}
# track-morph streams (include/world_class_track_morph.h, included below the lag's header): a fifth table
TRACK_MORPH_SIGNATURES = {
    "wc_track_morph_create": (_vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wc_track_morph_destroy": (None, [_vp]),
    "wc_track_morph_set_track_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "wc_track_morph_reset": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "wc_track_morph_set_weight": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "wc_track_morph_set_ratios": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "wc_track_morph_push_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ip]),
    "wc_track_morph_flush_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp, _vp, _ip]),
    "wc_track_morph_frames_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_track_morph_frames_formed": (C.c_longlong, [_vp, C.c_int]),
    "wc_track_morph_pending": (C.c_int, [_vp, C.c_int]),
    "wc_track_morph_get_delay": (C.c_int, [_vp, C.c_int]),
    "wc_track_morph_track_length": (C.c_int, [_vp, C.c_int]),
}
# coded track-morph streams (include/world_class_track_morph_coded.h, a header of its own that the stream header does not include):
# a sixth table
TRACK_MORPH_CODED_SIGNATURES = {
    "wc_track_morph_coded_create": (_vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wc_track_morph_coded_destroy": (None, [_vp]),
    "wc_track_morph_coded_set_track_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "wc_track_morph_coded_reset": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "wc_track_morph_coded_set_weight": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "wc_track_morph_coded_set_ratios": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "wc_track_morph_coded_push_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ip]),
    "wc_track_morph_coded_flush_device": (C.c_int, [_vp, _ip, _vp, _vp, _vp, _vp, _ip]),
    "wc_track_morph_coded_frames_received": (C.c_longlong, [_vp, C.c_int]),
    "wc_track_morph_coded_frames_formed": (C.c_longlong, [_vp, C.c_int]),
    "wc_track_morph_coded_pending": (C.c_int, [_vp, C.c_int]),
    "wc_track_morph_coded_get_delay": (C.c_int, [_vp, C.c_int]),
    "wc_track_morph_coded_track_length": (C.c_int, [_vp, C.c_int]),
    "wc_track_morph_coded_device_bytes": (C.c_longlong, [_vp]),
}
_lib = _binder(STREAM_SIGNATURES, ALIGN_STREAM_SIGNATURES, ALIGN_WINDOW_SIGNATURES, ALIGN_LAG_SIGNATURES, TRACK_MORPH_SIGNATURES,
               TRACK_MORPH_CODED_SIGNATURES)


class _StreamHandle(_Handle):
    """a handle of this module: close frees the staging arrays of its numpy front-ends as well (_staging names them; _out where a
    class says nothing else, None before the front-ends' first call)"""
    _lib = staticmethod(_lib)
    _out = None

    def _staging(self):
        return self._out or ()

    def _rows_out(self, formed):
        """(f0, sp, ap) per stream: the full rows staged in _out by a push that formed formed[u] frames"""
        f0, sp, ap = (split_rows(d.to_host(), formed, w) for d, w in zip(self._out, (None, self.bins, self.bins)))
        return list(zip(f0, sp, ap))

    def close(self):
        super().close()
        for d in self._staging():
            if d is not None:
                d.free()


class StreamAnalyzer(_StreamHandle):
    """n_streams concurrent streams; every push appends `chunk_ms` of samples per stream and returns the frames it commits
    (absolute times, F0, spectrogram rows), `lookahead_ms` behind the newest sample."""
    _sym = "wc_stream"

    def __init__(self, fs, n_streams, frame_period=1.0, chunk_ms=200, lookback_ms=400, lookahead_ms=400, harvest_f0_floor=71.0,
                 harvest_f0_ceil=800.0, q1=-0.15, cheaptrick_f0_floor=71.0, fft_size=0, context_ms=0, aperiodicity=False, d4c_threshold=0.85):
        self.fs, self.n_streams, self.frame_period = fs, n_streams, float(frame_period)
        self._create(fs, n_streams, float(frame_period), chunk_ms, lookback_ms, lookahead_ms, harvest_f0_floor, harvest_f0_ceil, q1,
                     cheaptrick_f0_floor, fft_size)
        if context_ms:  # incremental mode: Harvest's front on the newest chunk + 2 context only (see the header)
            _check(self._fn("_set_incremental")(self._h, context_ms))
        self.aperiodicity = bool(aperiodicity)
        if self.aperiodicity:  # D4C on the committed frames, with its own noise position per stream (see the header)
            _check(self._fn("_set_aperiodicity")(self._h, float(d4c_threshold)))
        self.fft_size = self._fn("_get_fft_size")(self._h)
        self.bins = self.fft_size // 2 + 1
        self.chunk_samples = self._fn("_chunk_samples")(self._h)
        self.max_frames = self._fn("_max_frames_per_push")(self._h)
        self.latency_ms = lookahead_ms + chunk_ms
        cap = n_streams * self.max_frames
        self._d_t, self._d_f, self._d_sp = DeviceArray(cap), DeviceArray(cap), DeviceArray(cap * self.bins)
        self._d_ap = DeviceArray(cap * self.bins) if self.aperiodicity else None
        self._d_csp = self._d_cap = None  # coded rows of push_coded: allocated on its first call

    def _staging(self):
        return self._d_t, self._d_f, self._d_sp, self._d_ap, self._d_csp, self._d_cap

    def _chunks(self, chunks):
        """the chunks of one push -> (chunk_format, samples per stream, their upload: a context that frees it).  The sample format
        is that of the first chunk with samples -- int16 and float32 go up as they are, anything else as float64 -- and the others
        must agree (resample._in_format, which falls back to float64 on a mix, is the converters' rule, not this one)"""
        filled = [np.asarray(c) for c in chunks if len(c)]  # (idle streams pass empty chunks of any type)
        dt = filled[0].dtype if filled and filled[0].dtype in (np.int16, np.float32) else np.dtype(np.float64)
        assert all(c.dtype == dt or dt == np.float64 for c in filled), "chunks of one push share a sample format"
        fmt = next(number for number, kind in IN_FORMATS.values() if kind == dt)
        n_new, flat = pack_rows(chunks, 1, dtype=dt)  # (nothing pushed: one sample of zeros goes up, not NULL)
        return fmt, n_new, uploaded(flat, dtype=dt)

    def _committed(self, counts, **rows):
        """per stream a dict of the frames a push committed: tpos, f0 and, per name in rows, (staging array or None, width)"""
        cut = dict(tpos=split_rows(self._d_t.to_host(), counts), f0=split_rows(self._d_f.to_host(), counts))
        cut.update({name: split_rows(d.to_host(), counts, width) for name, (d, width) in rows.items() if d is not None})
        return [dict(zip(cut, per_stream)) for per_stream in zip(*cut.values())]

    def push_device(self, d_chunk, n_new=None, flush=None, d_tpos=None, d_f0=None, d_sp=None, chunk_format=0, d_ap=None):
        """device pointers in and out (packed layouts of the header); chunk_format 0 = float64, 1 = int16 PCM, 2 = float32;
        d_ap: aperiodicity rows (streams created with aperiodicity=True); returns frames committed per stream"""
        n = self.n_streams
        out = (C.c_int * n)()
        nn = _ints(n_new) if n_new is not None else None
        fl = _ints(flush) if flush is not None else None
        t = _ptr(d_tpos if d_tpos is not None else self._d_t)
        f = _ptr(d_f0 if d_f0 is not None else self._d_f)
        sp = _ptr(d_sp if d_sp is not None else self._d_sp)
        if self.aperiodicity:
            _check(self._fn("_push_device_ex")(self._h, _ptr(d_chunk), chunk_format, nn, fl, t, f, sp,
                                                   _ptr(d_ap if d_ap is not None else self._d_ap), out))
        else:
            _check(self._fn("_push_device_fmt")(self._h, _ptr(d_chunk), chunk_format, nn, fl, t, f, sp, out))
        return list(out)

    def push(self, chunks, flush=None):
        """chunks: list of n_streams float64 arrays (length chunk_samples; empty = idle; shorter only with flush[u]).
        Returns a list of dicts (tpos, f0, sp) with the frames committed for every stream."""
        fmt, n_new, up = self._chunks(chunks)
        with up as (d,):  # (freed on an error as well, as push_coded always did)
            counts = self.push_device(d, n_new, flush, chunk_format=fmt)
            return self._committed(counts, sp=(self._d_sp, self.bins), ap=(self._d_ap, self.bins))

    def push_coded_device(self, d_chunk, d_coded_sp, number_of_dimensions, d_coded_ap=None, n_new=None, flush=None, d_tpos=None, d_f0=None,
                          chunk_format=0):
        """push_device with the committed frames coded on the device: d_coded_sp takes number_of_dimensions doubles per frame,
        d_coded_ap (streams created with aperiodicity=True, else None) number_of_aperiodicities(fs); returns frames per stream"""
        n = self.n_streams
        out = (C.c_int * n)()
        nn = _ints(n_new) if n_new is not None else None
        fl = _ints(flush) if flush is not None else None
        t = _ptr(d_tpos if d_tpos is not None else self._d_t)
        f = _ptr(d_f0 if d_f0 is not None else self._d_f)
        _check(self._fn("_push_coded_device")(self._h, _ptr(d_chunk), chunk_format, nn, fl, t, f, _ptr(d_coded_sp), int(number_of_dimensions),
                                                  None if d_coded_ap is None else _ptr(d_coded_ap), out))
        return list(out)

    def push_coded(self, chunks, number_of_dimensions=60, flush=None):
        """push with coded results: a list of dicts (tpos, f0, csp, and cap when aperiodicity is on) per stream"""
        from .codec import number_of_aperiodicities
        nd, n_ap = int(number_of_dimensions), number_of_aperiodicities(self.fs) if self.aperiodicity else 0
        cap = self.n_streams * self.max_frames
        if self._d_csp is None or self._d_csp.n < cap * nd:
            self._d_csp = DeviceArray(cap * nd)
        if self.aperiodicity and self._d_cap is None:
            self._d_cap = DeviceArray(cap * max(n_ap, 1))
        fmt, n_new, up = self._chunks(chunks)
        with up as (d,):
            counts = self.push_coded_device(d, self._d_csp, nd, self._d_cap, n_new, flush, chunk_format=fmt)
            return self._committed(counts, csp=(self._d_csp, nd), cap=(self._d_cap, n_ap))

    def reset(self, stream):
        _check(self._fn("_reset")(self._h, stream))

    def rng_position(self, stream):
        return int(self._fn("_rng_position")(self._h, stream))

    def set_rng_position(self, stream, position):
        _check(self._fn("_set_rng_position")(self._h, stream, int(position)))

    def d4c_rng_position(self, stream):
        return int(self._fn("_d4c_rng_position")(self._h, stream))

    def set_d4c_rng_position(self, stream, position):
        _check(self._fn("_set_d4c_rng_position")(self._h, stream, int(position)))

    def frames_committed(self, stream):
        return int(self._fn("_frames_committed")(self._h, stream))

    def run_whole(self, xs, coded=None):
        """convenience for tests: stream whole signals chunk by chunk (all streams in lockstep, ragged ends flushed) and return the
        concatenated per-stream results; coded = a number of dimensions: through push_coded (csp / cap instead of sp / ap)"""
        assert len(xs) == self.n_streams
        cs = self.chunk_samples
        keys = ("csp", "cap") if coded else ("sp", "ap")
        acc = [dict(tpos=[], f0=[], **{keys[0]: []}, **({keys[1]: []} if self.aperiodicity else {})) for _ in xs]
        done = [False] * len(xs)
        pos = 0
        while not all(done):
            chunks, flush = [], []
            for u, x in enumerate(xs):
                if done[u]:
                    chunks.append(np.zeros(0))
                    flush.append(0)
                    continue
                last = pos + cs >= len(x)
                chunks.append(x[pos:pos + cs])
                flush.append(1 if last else 0)
                done[u] = last
            for u, r in enumerate(self.push_coded(chunks, coded, flush) if coded else self.push(chunks, flush)):
                for k in acc[u]:
                    acc[u][k].append(r[k])
            pos += cs
        return [{k: np.concatenate(v) for k, v in a.items()} for a in acc]


class StreamSynthesizer(_StreamHandle):
    """n_streams concurrent synthesis streams: every push appends up to `max_frames` frames (f0, spectrogram and aperiodicity rows)
    per stream and returns the samples that no later frame can change -- those of one whole-utterance Synthesis over all frames."""
    _sym = "wc_synth_stream"

    def __init__(self, fs, fft_size, frame_period=5.0, n_streams=1, max_frames=200):
        self.fs, self.fft_size, self.frame_period, self.n_streams, self.max_frames = fs, fft_size, float(frame_period), n_streams, max_frames
        self.bins = fft_size // 2 + 1
        self._create(fs, fft_size, float(frame_period), n_streams, max_frames)
        self.max_samples = self._fn("_max_samples_per_push")(self._h)
        self._d_y = DeviceArray(n_streams * self.max_samples)

    def _staging(self):
        return (self._d_y,)

    def push_device(self, n_frames, d_f0, d_sp, d_ap, flush=None, d_y=None):
        """device pointers in and out (packed layouts of the header); returns the samples committed per stream"""
        out = (C.c_int * self.n_streams)()
        _check(self._fn("_push_device")(self._h, _ints(n_frames), _ints(flush) if flush is not None else None, _ptr(d_f0),
                                                  _ptr(d_sp), _ptr(d_ap), _ptr(d_y if d_y is not None else self._d_y), out))
        return list(out)

    def push_coded_device(self, n_frames, d_f0, d_coded_sp, number_of_dimensions, d_coded_ap, flush=None, d_y=None):
        """as push_device with coded rows (number_of_dimensions mel-cepstral coefficients and the band aperiodicities per frame)"""
        out = (C.c_int * self.n_streams)()
        _check(self._fn("_push_coded_device")(self._h, _ints(n_frames), _ints(flush) if flush is not None else None, _ptr(d_f0),
                                                        _ptr(d_coded_sp), int(number_of_dimensions), _ptr(d_coded_ap),
                                                        _ptr(d_y if d_y is not None else self._d_y), out))
        return list(out)

    def push(self, f0s, sps, aps, flush=None):
        """f0s / sps / aps: per stream the new frames (empty = idle).  Returns the committed samples of every stream."""
        return self._push(f0s, sps, aps, flush, self.bins, self.bins, self.push_device)

    def push_coded(self, f0s, csps, caps, flush=None):
        """push with coded rows: csps[u] (frames x number_of_dimensions), caps[u] (frames x number_of_aperiodicities(fs))"""
        from .codec import number_of_aperiodicities
        nd = next((np.shape(v)[1] for v in csps if len(v)), 1)  # (the width of the first entry with rows, else 1: pack_rows holds the others to it)
        return self._push(f0s, csps, caps, flush, nd, number_of_aperiodicities(self.fs),
                          lambda n, f, a, b, fl: self.push_coded_device(n, f, a, nd, b, fl))

    def _push(self, f0s, sps, aps, flush, w_sp, w_ap, run):
        n_frames, f0 = pack_rows(f0s, 1)  # (nothing pushed: one row of zeros each goes up, not NULL)
        with uploaded(f0, pack_rows(sps, w_sp)[1], pack_rows(aps, w_ap)[1]) as d:
            counts = run(n_frames, *d, flush)
            return split_rows(self._d_y.to_host(), counts)

    def reset(self, stream):
        _check(self._fn("_reset")(self._h, stream))

    def set_modification(self, stream, f0_scale=1.0, spectral_ratio=0.0):
        """pitch and formant shift of the frames that later coded pushes give this stream ((1.0, 0.0) = none, also after reset);
        push_device takes no frames for a stream with a setting"""
        _check(self._fn("_set_modification")(self._h, int(stream), float(f0_scale), float(spectral_ratio)))

    def set_speed(self, stream, speed):
        """speed of the stream (1.0 = none, also after reset): the frames pushed from now on are source frames, and the stream
        synthesises the frames at pos[k] = pos[k-1] + speed source frames (the rule of the header).  Refused for a retimed stream
        while floor(source_position + speed) < frames_received - 1 (one source row is carried); a stream with a modification setting
        that is to change speed mid-stream calls this (1.0 will do) before its first frame"""
        _check(self._fn("_set_speed")(self._h, int(stream), float(speed)))

    def source_position(self, stream):
        """position in source frames of the newest synthesis frame formed (NaN before the first)"""
        return float(self._fn("_source_position")(self._h, int(stream)))

    def frames_synthesised(self, stream):
        """synthesis frames formed so far (frames_received counts the source frames pushed)"""
        return int(self._fn("_frames_synthesised")(self._h, int(stream)))

    def frames_for_push(self, stream, n_frames):
        """synthesis frames a push of n_frames source frames would form at the current setting (at most max_frames + 1)"""
        return _count(self._fn("_frames_for_push")(self._h, int(stream), int(n_frames)))

    def rng_position(self, stream):
        return int(self._fn("_rng_position")(self._h, stream))

    def set_rng_position(self, stream, position):
        _check(self._fn("_set_rng_position")(self._h, stream, int(position)))

    def frames_received(self, stream):
        return int(self._fn("_frames_received")(self._h, stream))

    def samples_committed(self, stream):
        return int(self._fn("_samples_committed")(self._h, stream))

    def run_whole(self, params, pattern, on_push=None):
        """convenience for tests: params[u] = (f0, sp, ap) of a whole utterance; pattern[u] = list of frame counts per push (cycled;
        0 = an idle push), the last push of a stream flushes it.  Returns the concatenated samples per stream."""
        n = self.n_streams
        assert len(params) == n and len(pattern) == n
        pos, k, done = [0] * n, [0] * n, [False] * n
        acc = [[] for _ in range(n)]
        while not all(done):
            f0s, sps, aps, flush = [], [], [], []
            for u, (f0, sp, ap) in enumerate(params):
                c = 0 if done[u] else min(pattern[u][k[u] % len(pattern[u])], self.max_frames, len(f0) - pos[u])
                k[u] += 1
                last = not done[u] and pos[u] + c >= len(f0)
                f0s.append(f0[pos[u]:pos[u] + c])
                sps.append(sp[pos[u]:pos[u] + c])
                aps.append(ap[pos[u]:pos[u] + c])
                flush.append(1 if last else 0)
                pos[u] += c
            for u, y in enumerate(self.push(f0s, sps, aps, flush)):
                acc[u].append(y)
                if on_push is not None:
                    on_push(u, len(y))
            for u in range(n):
                done[u] = done[u] or bool(flush[u])
        return [np.concatenate(a) for a in acc]


class MorphStream(_StreamHandle):
    """n_streams concurrent morph streams in front of a StreamSynthesizer: every push appends up to `max_frames` source frames of
    voice A and of voice B per stream and returns the morphed frames (f0, spectrogram and aperiodicity rows) that both voices' rows
    now allow -- those of one whole-utterance io.morph_parameters_device pair at the stream's positions (the rule of the header)."""
    _sym = "wc_morph_stream"

    def __init__(self, fs, fft_size, n_streams=1, max_frames=200, max_backlog=16):
        self.fs, self.fft_size, self.n_streams, self.max_frames, self.max_backlog = fs, fft_size, n_streams, max_frames, max_backlog
        self.bins = fft_size // 2 + 1
        self._create(fs, fft_size, n_streams, max_frames, max_backlog)
        self._out = None  # the outputs of the numpy front-ends: allocated on their first call

    def push_device(self, n_a, d_f0_a, d_sp_a, d_ap_a, n_b, d_f0_b, d_sp_b, d_ap_b, d_f0_out, d_sp_out, d_ap_out):
        """device pointers in and out (packed layouts of the header); returns the frames formed per stream"""
        out = (C.c_int * self.n_streams)()
        _check(self._fn("_push_device")(self._h, self._counts(n_a), _opt(d_f0_a), _opt(d_sp_a), _opt(d_ap_a), self._counts(n_b), _opt(d_f0_b),
                                                  _opt(d_sp_b), _opt(d_ap_b), _opt(d_f0_out), _opt(d_sp_out), _opt(d_ap_out), out))
        return list(out)

    def push_coded_device(self, n_a, d_f0_a, d_coded_sp_a, d_coded_ap_a, n_b, d_f0_b, d_coded_sp_b, d_coded_ap_b, number_of_dimensions, d_f0_out,
                          d_sp_out, d_ap_out):
        """as push_device with coded rows (number_of_dimensions mel-cepstral coefficients and the band aperiodicities per frame);
        the frames come out as full rows"""
        out = (C.c_int * self.n_streams)()
        _check(self._fn("_push_coded_device")(self._h, self._counts(n_a), _opt(d_f0_a), _opt(d_coded_sp_a), _opt(d_coded_ap_a),
                                                        self._counts(n_b), _opt(d_f0_b), _opt(d_coded_sp_b), _opt(d_coded_ap_b), int(number_of_dimensions),
                                                        _opt(d_f0_out), _opt(d_sp_out), _opt(d_ap_out), out))
        return list(out)

    def _counts(self, n):
        if len(n) != self.n_streams:
            raise ValueError("one frame count per stream")
        return _ints(n)

    def push(self, a, b):
        """a[u] / b[u]: (f0, sp rows, ap rows) with the new frames of voice A / B of stream u (empty = none).  Returns per stream
        (f0, sp, ap) of the frames formed."""
        return self._push(a, b, self.bins, self.bins, self.push_device)

    def push_coded(self, a, b):
        """push with coded rows: a[u] / b[u] = (f0, frames x number_of_dimensions, frames x number_of_aperiodicities(fs))"""
        from .codec import number_of_aperiodicities
        nd = next((np.shape(v[1])[1] for v in list(a) + list(b) if len(v[0])), 1)  # (of the first entry with rows, else 1)
        return self._push(a, b, nd, number_of_aperiodicities(self.fs),
                          lambda na, fa, xa, ya, nb, fb, xb, yb, *outs: self.push_coded_device(na, fa, xa, ya, nb, fb, xb, yb, nd, *outs))

    def _push(self, a, b, w_sp, w_ap, run):
        if self._out is None:
            cap = self.n_streams * self.max_frames
            self._out = (DeviceArray(cap), DeviceArray(cap * self.bins), DeviceArray(cap * self.bins))
        counts, up = [], []
        for voice in (a, b):  # (a voice with nothing pushed: one row of zeros each goes up, not NULL)
            n, f0 = pack_rows([v[0] for v in voice], 1)
            counts.append(n)
            up += [f0, pack_rows([v[1] for v in voice], w_sp)[1], pack_rows([v[2] for v in voice], w_ap)[1]]
        with uploaded(*up) as d:
            return self._rows_out(run(counts[0], *d[:3], counts[1], *d[3:], *self._out))

    def set_speeds(self, stream, speed_a, speed_b):
        """source frames of voice A / B per formed frame (1.0 after create and reset): any finite speed > 0 at any time"""
        _check(self._fn("_set_speeds")(self._h, int(stream), float(speed_a), float(speed_b)))

    def set_weight(self, stream, weight, f0_weight=None):
        """the blend of the frames formed from the next push on: 0 = voice A, 1 = voice B; f0_weight None: the weight"""
        _check(self._fn("_set_weight")(self._h, int(stream), float(weight), float(weight if f0_weight is None else f0_weight)))

    def set_ratios(self, stream, ratio_a, ratio_b):
        """spectral ratio per voice (0 = none), applied to that voice's log envelope in front of the blend"""
        _check(self._fn("_set_ratios")(self._h, int(stream), float(ratio_a), float(ratio_b)))

    def reset(self, stream):
        _check(self._fn("_reset")(self._h, int(stream)))

    def frames_for_push(self, stream, n_a, n_b):
        """frames a push of n_a and n_b source frames would form at the current speeds (at most max_frames + 1)"""
        return _count(self._fn("_frames_for_push")(self._h, int(stream), int(n_a), int(n_b)))

    def source_position(self, stream, source):
        """position in voice `source` (0 = A, 1 = B) of the newest frame formed (NaN before the first)"""
        return float(self._fn("_source_position")(self._h, int(stream), int(source)))

    def frames_received(self, stream, source):
        return int(self._fn("_frames_received")(self._h, int(stream), int(source)))

    def backlog(self, stream, source):
        """rows of voice `source` the stream keeps for later frames"""
        return int(self._fn("_backlog")(self._h, int(stream), int(source)))

    def frames_formed(self, stream):
        return int(self._fn("_frames_formed")(self._h, int(stream)))


class AlignStream(_StreamHandle):
    """n_streams concurrent alignment streams over n_tracks resident tracks of coded rows (dims doubles, compared over
    dim_begin <= c < dim_end): every push appends up to `max_rows_per_push` rows of a live voice per stream and returns, per pushed
    row, its position in the stream's track and the cost so far -- d_cost and span[1] of one whole-utterance
    io.align_features_ex_device pair (the rows so far, the track) at step pattern 0 with an open end (the rule of the header)."""
    _sym = "wc_align_stream"

    def __init__(self, dims, n_streams, n_tracks, max_track_frames, max_rows_per_push, dim_begin=1, dim_end=None):
        self.dims, self.n_streams, self.n_tracks = int(dims), int(n_streams), int(n_tracks)
        self.max_track_frames, self.max_rows_per_push = int(max_track_frames), int(max_rows_per_push)
        self.dim_begin, self.dim_end = int(dim_begin), int(dims if dim_end is None else dim_end)
        self._create(self.dims, self.dim_begin, self.dim_end, self.n_streams, self.n_tracks, self.max_track_frames, self.max_rows_per_push)
        self._out = None  # the outputs of push: allocated on its first call
        self._settled = None  # the third output of push_settled: allocated on its first call

    def _staging(self):
        return (self._out or ()) + (self._settled,)

    def set_track_device(self, track, m, d_feat):
        """m rows of a device array into the slot (stream-ordered; refused while a stream that has received rows follows it)"""
        _check(self._fn("_set_track_device")(self._h, int(track), int(m), _opt(d_feat)))

    def set_track(self, track, feat):
        feat = np.ascontiguousarray(feat, dtype=np.float64)
        if feat.ndim != 2 or feat.shape[1] != self.dims:
            raise ValueError("a track is an (m, dims) array")
        with uploaded(feat) as (d,):
            self.set_track_device(track, feat.shape[0], d)
            _check(lib().wc_synchronize())

    def reset(self, stream, track, open_begin=False):
        """attach the stream to a track that has been set; its row count returns to zero"""
        _check(self._fn("_reset")(self._h, int(stream), int(track), 1 if open_begin else 0))

    def set_window(self, stream, width, back, hop=1, monotone=False):
        """a search window of `width` columns that starts `back` columns behind the position and moves every `hop` rows, on a stream
        that has been reset and has no rows yet (the rule of world_class_align_window.h); monotone: the position never falls.
        width 0 (back 0, hop 1) removes it; so does every reset"""
        _check(self._fn("_set_window")(self._h, int(stream), int(width), int(back), int(hop), ALIGN_WINDOW_MONOTONE if monotone else 0))

    def get_window(self, stream):
        """(width, back, hop, monotone); (0, 0, 1, False) where no window is set"""
        v = [C.c_int() for _ in range(4)]
        _check(self._fn("_get_window")(self._h, int(stream), *[C.byref(x) for x in v]))
        return v[0].value, v[1].value, v[2].value, bool(v[3].value & ALIGN_WINDOW_MONOTONE)

    def reserve_lag(self, max_lag):
        """the ring of choices behind set_lag: one byte per cell, max_lag + max_rows_per_push rows of max_track_frames per stream
        (the rule of world_class_align_lag.h); once per handle"""
        _check(self._fn("_reserve_lag")(self._h, int(max_lag)))

    def set_lag(self, stream, lag):
        """push_settled reports where the row `lag` frames ago lies on the path behind the newest row; on a stream that has been
        reset and has no rows yet, 0 <= lag <= max_lag of reserve_lag.  0 removes the lag; so does every reset"""
        _check(self._fn("_set_lag")(self._h, int(stream), int(lag)))

    def get_lag(self, stream):
        """the stream's lag (0: none); -1 for a bad index"""
        return int(self._fn("_get_lag")(self._h, int(stream)))

    def push_device(self, n_rows, d_feat, d_position, d_cost):
        """device pointers in and out (packed layouts of the header): one position and one cost per pushed row"""
        if len(n_rows) != self.n_streams:
            raise ValueError("one row count per stream")
        _check(self._fn("_push_device")(self._h, _ints(n_rows), _opt(d_feat), _opt(d_position), _opt(d_cost)))

    def push_settled_device(self, n_rows, d_feat, d_position, d_cost, d_settled):
        """push_device with one more output packed the same way: per pushed row, where the row `lag` frames ago lies on the path
        behind it (the position itself for a stream without a lag)"""
        if len(n_rows) != self.n_streams:
            raise ValueError("one row count per stream")
        _check(self._fn("_push_settled_device")(self._h, _ints(n_rows), _opt(d_feat), _opt(d_position), _opt(d_cost), _opt(d_settled)))

    def _push(self, rows, n_out):
        if len(rows) != self.n_streams:
            raise ValueError("one entry per stream")
        counts, flat = pack_rows(rows, self.dims, placeholder=False)  # (nothing pushed: NULL goes down, no placeholder)
        cap = self.n_streams * self.max_rows_per_push
        if self._out is None:
            self._out = (DeviceArray(cap), DeviceArray(cap))
        if n_out == 3 and self._settled is None:
            self._settled = DeviceArray(cap)
        outs = self._out + ((self._settled,) if n_out == 3 else ())
        with uploaded(flat) as (d,):
            if n_out == 3:
                self.push_settled_device(counts, d, *outs)
            else:
                self.push_device(counts, d, *outs)
            got = [o.to_host() if flat is not None else np.zeros(0) for o in outs]  # (one position and so on per pushed row)
        return list(zip(*(split_rows(g, counts) for g in got)))

    def push(self, rows):
        """rows[u]: a (k_u, dims) array with the new rows of stream u, or None.  Returns per stream (position, cost), k_u doubles
        each."""
        return self._push(rows, 2)

    def push_settled(self, rows):
        """push with the settled positions: per stream (position, cost, settled), k_u doubles each"""
        return self._push(rows, 3)

    def tail(self, streams=None):
        """the flush: per stream in `streams` (None: every stream that has a lag and rows) the K = min(lag + 1, rows received)
        half-integers of the newest row's path in the stream's last K rows, ascending.  Returns one array per stream of the
        handle, None for a stream that was not asked for.  Changes no state"""
        if streams is None:
            streams = [u for u in range(self.n_streams) if self.get_lag(u) > 0 and self.rows_received(u) > 0]
        want = [0] * self.n_streams
        for u in streams:
            want[int(u)] = 1
        ks = [min(self.get_lag(u) + 1, self.rows_received(u)) if want[u] else 0 for u in range(self.n_streams)]
        d = DeviceArray(max(sum(ks), 1))
        try:
            _check(self._fn("_tail_device")(self._h, _ints(want), _ptr(d)))
            got = d.to_host()
        finally:
            d.free()
        return [part if want[u] else None for u, part in enumerate(split_rows(got, ks))]

    def tail_device(self, want, d_tail):
        """the flush into a device array: per stream with want[u] != 0, K = min(lag + 1, rows received) doubles packed in stream
        order (the layout TrackMorph.flush_device takes).  Changes no state"""
        if len(want) != self.n_streams:
            raise ValueError("one flag per stream")
        _check(self._fn("_tail_device")(self._h, _ints([1 if v else 0 for v in want]), _opt(d_tail)))

    def rows_received(self, stream):
        return int(self._fn("_rows_received")(self._h, int(stream)))

    def track_length(self, track):
        return int(self._fn("_track_length")(self._h, int(track)))


class _TrackMorphBase(_StreamHandle):
    """What TrackMorph and CodedTrackMorph share: everything but the row widths.  `_sym` names the handle's C symbols; a class
    sets n_streams, max_frames, max_delay, bins and _h (_create) in its __init__ and keeps the methods that name its rows."""

    def reset(self, stream, track, delay=0):
        """attach the stream to a track that has been set, `delay` rows behind the newest (the lag of the alignment stream whose
        settled positions it is given); counts, weights and ratios return to zero"""
        _check(self._fn("_reset")(self._h, int(stream), int(track), int(delay)))

    def set_weight(self, stream, weight, f0_weight=None):
        """the blend of the frames formed from the next push on: 0 = the live voice, 1 = the track; f0_weight None: the weight"""
        _check(self._fn("_set_weight")(self._h, int(stream), float(weight), float(weight if f0_weight is None else f0_weight)))

    def set_ratios(self, stream, ratio_a, ratio_b):
        """spectral ratio of the live voice / of the track (0 = none), applied to that log envelope in front of the blend"""
        _check(self._fn("_set_ratios")(self._h, int(stream), float(ratio_a), float(ratio_b)))

    def _counts(self, n):
        if len(n) != self.n_streams:
            raise ValueError("one entry per stream")
        return _ints(n)

    def _push_device(self, n_a, *d):
        out = (C.c_int * self.n_streams)()
        _check(self._fn("_push_device")(self._h, self._counts(n_a), *(_opt(x) for x in d), out))
        return list(out)

    def flush_device(self, want, d_tail, d_f0_out, d_sp_out, d_ap_out):
        """the rows that still wait, at the positions of AlignStream's tail_device for the same `want` (one flag per stream); the
        wanted streams have ended afterwards.  Returns the frames formed per stream"""
        out = (C.c_int * self.n_streams)()
        _check(self._fn("_flush_device")(self._h, self._counts([1 if v else 0 for v in want]), _opt(d_tail), _opt(d_f0_out), _opt(d_sp_out),
                                       _opt(d_ap_out), out))
        return list(out)

    def _run(self, ins, run):
        if self._out is None:
            cap = self.n_streams * max(self.max_frames, self.max_delay)
            self._out = (DeviceArray(cap), DeviceArray(cap * self.bins), DeviceArray(cap * self.bins))
        with uploaded(*ins) as d:
            return self._rows_out(run(*d, *self._out))

    def _push(self, rows, positions, sp_width, ap_width):
        """push for rows of the two widths"""
        if len(rows) != self.n_streams or len(positions) != self.n_streams:
            raise ValueError("one entry per stream")
        # (nothing pushed: one row of zeros each goes up, not NULL)
        counts, f0 = pack_rows([np.ravel(v[0]) for v in rows], 1)
        n_pos, pos = pack_rows([np.ravel(p) for p in positions], 1)
        if n_pos != counts:
            raise ValueError("one position per pushed row")
        sp, ap = (pack_rows([v[k] for v in rows], w)[1] for k, w in ((1, sp_width), (2, ap_width)))
        return self._run((f0, sp, ap, pos), lambda *a: self.push_device(counts, *a))

    def _set_track(self, track, f0, sp, ap):
        """set_track for rows whose shapes the class has checked"""
        with uploaded(f0, sp, ap) as d:
            self.set_track_device(track, len(f0), *d)
            _check(lib().wc_synchronize())

    def flush(self, tails, streams=None):
        """tails[u]: what AlignStream.tail returns for stream u (K = min(delay + 1, rows received) doubles; None: not wanted);
        streams None: every stream with an entry.  Returns per stream (f0, sp, ap) of the frames formed, empty where not wanted"""
        if len(tails) != self.n_streams:
            raise ValueError("one entry per stream")
        if streams is None:
            streams = [u for u in range(self.n_streams) if tails[u] is not None]
        want = [0] * self.n_streams
        for u in streams:
            want[int(u)] = 1
        ks = [min(self.get_delay(u) + 1, self.frames_received(u)) if want[u] else 0 for u in range(self.n_streams)]
        got, tail = pack_rows([np.ravel(tails[u]) if want[u] else None for u in range(self.n_streams)], 1)
        if got != ks:
            raise ValueError("min(delay + 1, rows received) tail positions per wanted stream")
        return self._run((tail,), lambda *a: self.flush_device(want, *a))

    def frames_received(self, stream):
        return int(self._fn("_frames_received")(self._h, int(stream)))

    def frames_formed(self, stream):
        return int(self._fn("_frames_formed")(self._h, int(stream)))

    def pending(self, stream):
        """rows of the live voice the stream keeps for frames still to be formed"""
        return int(self._fn("_pending")(self._h, int(stream)))

    def get_delay(self, stream):
        return int(self._fn("_get_delay")(self._h, int(stream)))

    def track_length(self, track):
        return int(self._fn("_track_length")(self._h, int(track)))


class TrackMorph(_TrackMorphBase):
    """n_streams concurrent track-morph streams in front of a StreamSynthesizer, over n_tracks resident tracks of full rows: every
    push appends up to `max_frames` rows of a live voice per stream with one position in the stream's track per row -- device
    memory, such as d_settled of AlignStream.push_settled_device -- and returns the morphed frames (f0, spectrogram and aperiodicity
    rows) those positions allow, `delay` rows behind the newest: those of one whole-utterance io.morph_parameters_device pair (the
    rows so far, the track) at position_a = the frame's index (the rule of include/world_class_track_morph.h)."""

    _sym = "wc_track_morph"

    def __init__(self, fs, fft_size, n_streams, n_tracks, max_track_frames, max_frames=200, max_delay=0):
        self.fs, self.fft_size, self.n_streams, self.n_tracks = int(fs), int(fft_size), int(n_streams), int(n_tracks)
        self.max_track_frames, self.max_frames, self.max_delay = int(max_track_frames), int(max_frames), int(max_delay)
        self.bins = self.fft_size // 2 + 1
        self._create(self.fs, self.fft_size, self.n_streams, self.n_tracks, self.max_track_frames, self.max_frames, self.max_delay)
        self._out = None  # the outputs of the numpy front-ends: allocated on their first call

    def set_track_device(self, track, m, d_f0_b, d_sp_b, d_ap_b):
        """m full rows of device arrays into the slot (stream-ordered; refused while a stream that has received rows is attached)"""
        _check(self._fn("_set_track_device")(self._h, int(track), int(m), _opt(d_f0_b), _opt(d_sp_b), _opt(d_ap_b)))

    def set_track(self, track, f0, sp, ap):
        f0 = np.ascontiguousarray(f0, dtype=np.float64).ravel()
        sp, ap = (np.ascontiguousarray(v, dtype=np.float64) for v in (sp, ap))
        if sp.shape != (len(f0), self.bins) or ap.shape != sp.shape:
            raise ValueError("a track is m F0 values and two (m, fft_size / 2 + 1) arrays")
        self._set_track(track, f0, sp, ap)

    def push_device(self, n_a, d_f0_a, d_sp_a, d_ap_a, d_position_b, d_f0_out, d_sp_out, d_ap_out):
        """device pointers in and out (packed layouts of the header), one position per pushed row; returns the frames formed per
        stream"""
        return self._push_device(n_a, d_f0_a, d_sp_a, d_ap_a, d_position_b, d_f0_out, d_sp_out, d_ap_out)

    def push(self, rows, positions):
        """rows[u]: (f0, sp rows, ap rows) with the new rows of the live voice of stream u (empty = none); positions[u]: one
        position in the track per row.  Returns per stream (f0, sp, ap) of the frames formed."""
        return self._push(rows, positions, self.bins, self.bins)


class CodedTrackMorph(_TrackMorphBase):
    """TrackMorph with its tracks, its ring and its live rows held as coded features (include/world_class_track_morph_coded.h):
    `number_of_dimensions` doubles of the coded spectral envelope and GetNumberOfAperiodicities(fs) band aperiodicities per row, as
    codec.code_features_device writes them -- the arrays an AlignStream takes.  The frames it returns are full rows (f0, spectrogram
    and aperiodicity rows) and equal, bit for bit, those of a TrackMorph fed codec.decode_features_device of the same coded rows."""

    _sym = "wc_track_morph_coded"

    def __init__(self, fs, fft_size, number_of_dimensions, n_streams, n_tracks, max_track_frames, max_frames=200, max_delay=0):
        self.fs, self.fft_size, self.number_of_dimensions = int(fs), int(fft_size), int(number_of_dimensions)
        self.n_streams, self.n_tracks = int(n_streams), int(n_tracks)
        self.max_track_frames, self.max_frames, self.max_delay = int(max_track_frames), int(max_frames), int(max_delay)
        self.bins = self.fft_size // 2 + 1
        self._create(self.fs, self.fft_size, self.number_of_dimensions, self.n_streams, self.n_tracks, self.max_track_frames, self.max_frames,
                     self.max_delay)
        self.n_ap = int(lib().GetNumberOfAperiodicities(self.fs))
        self._out = None  # the outputs of the numpy front-ends: allocated on their first call

    def set_track_device(self, track, m, d_f0_b, d_coded_sp_b, d_coded_ap_b):
        """m coded rows of device arrays and their F0 into the slot (stream-ordered; refused while a stream that has received rows
        is attached)"""
        _check(self._fn("_set_track_device")(self._h, int(track), int(m), _opt(d_f0_b), _opt(d_coded_sp_b), _opt(d_coded_ap_b)))

    def set_track(self, track, f0, csp, cap):
        f0 = np.ascontiguousarray(f0, dtype=np.float64).ravel()
        csp, cap = (np.ascontiguousarray(v, dtype=np.float64) for v in (csp, cap))
        if csp.shape != (len(f0), self.number_of_dimensions) or cap.shape != (len(f0), self.n_ap):
            raise ValueError("a coded track is m F0 values, an (m, number_of_dimensions) and an (m, number of aperiodicities) array")
        self._set_track(track, f0, csp, cap)

    def push_device(self, n_a, d_f0_a, d_coded_sp_a, d_coded_ap_a, d_position_b, d_f0_out, d_sp_out, d_ap_out):
        """device pointers in (coded rows) and out (full rows), packed as the header says, one position per pushed row; returns the
        frames formed per stream"""
        return self._push_device(n_a, d_f0_a, d_coded_sp_a, d_coded_ap_a, d_position_b, d_f0_out, d_sp_out, d_ap_out)

    def push(self, rows, positions):
        """rows[u]: (f0, coded sp rows, coded ap rows) with the new rows of the live voice of stream u (empty = none); positions[u]:
        one position in the track per row.  Returns per stream (f0, sp, ap) of the frames formed, full rows."""
        return self._push(rows, positions, self.number_of_dimensions, self.n_ap)

    def device_bytes(self):
        """what the handle allocated on the device: tracks + ring + scratch + records (the header's formula)"""
        return int(self._fn("_device_bytes")(self._h))
