"""Synthesis stage wrapper (reference include/synthesis.hpp:29-51) over the C-ABI."""
import ctypes as C

import numpy as np

from . import (_c, _check, _Handle, _ints, _opt, _p, _ptr, _ptr_array, _rng_arg, _row_tables, _rows, lib,
               synthesis_out_length)


class Synthesis(_Handle):
    """Synthesis(fs, fft_size, frame_period_ms); compute(f0, spectrogram, aperiodicity, out_length)"""
    _lib = staticmethod(lib)
    _sym = "wc_synthesis"

    def __init__(self, fs, fft_size, frame_period=5.0):
        self.fs, self.fft_size, self.frame_period = fs, fft_size, frame_period
        self.bins = fft_size // 2 + 1
        self._create(fs, fft_size, frame_period)

    def out_length(self, f0_length):
        return synthesis_out_length(f0_length, self.frame_period, self.fs)  # reference test/test.cpp:362-363

    def compute(self, f0, spectrogram, aperiodicity, out_length=None, out=None):
        f = _c(f0)
        sp, ap = _c(spectrogram), _c(aperiodicity)
        if sp.shape != (len(f), self.bins) or ap.shape != (len(f), self.bins):
            raise ValueError(f"Synthesis.compute: spectrogram and aperiodicity must be ({len(f)}, {self.bins})")
        if out_length is None:
            out_length = self.out_length(len(f)) if out is None else len(out)
        if out is None:
            out = np.zeros(out_length)
        elif not isinstance(out, np.ndarray) or out.dtype != np.float64 or out.ndim != 1 or not out.flags.c_contiguous or len(out) < out_length:
            raise ValueError(f"Synthesis.compute: out must be a contiguous float64 vector of at least {out_length} samples")
        _check(lib().wc_synthesis_compute(self._h, _p(f), len(f), _rows(sp), _rows(ap), out_length, _p(out)))
        return out

    def compute_device(self, d_f0, f0_lengths, d_sp, d_ap, out_lengths, d_out, rng_pos=None):
        n = len(f0_lengths)
        arr, arg = _rng_arg(rng_pos, n)
        _check(lib().wc_synthesis_compute_device(self._h, n, _ptr(d_f0), _ints(f0_lengths), _ptr(d_sp), _ptr(d_ap),
                                                 _ints(out_lengths), _ptr(d_out), arg))
        return list(arr) if arr is not None else None

    def compute_batch(self, f0s, sps, aps, out_lengths=None, rng_pos=None):
        fl = [len(v) for v in f0s]
        if out_lengths is None:
            out_lengths = [self.out_length(n) for n in fl]
        fs_, sps, aps = [_c(v) for v in f0s], [_c(v) for v in sps], [_c(v) for v in aps]
        if not (len(fs_) == len(sps) == len(aps) == len(out_lengths)) or len(fs_) == 0:
            raise ValueError("Synthesis.compute_batch: f0s, sps, aps (and out_lengths) must be non-empty lists of the same length")
        for u, (f, sp, ap) in enumerate(zip(fs_, sps, aps)):
            if sp.shape != (len(f), self.bins) or ap.shape != (len(f), self.bins):
                raise ValueError(f"Synthesis.compute_batch: utterance {u}: spectrogram and aperiodicity must be ({len(f)}, {self.bins})")
        ys = [np.zeros(n) for n in out_lengths]
        stab, keep1 = _row_tables(sps)
        atab, keep2 = _row_tables(aps)
        arr, arg = _rng_arg(rng_pos, len(fl))
        _check(lib().wc_synthesis_compute_batch(self._h, len(fl), _ptr_array(fs_), _ints(fl), self.fft_size, stab, atab, _ints(out_lengths),
                                                _ptr_array(ys), arg))
        return (ys, list(arr)) if rng_pos is not None else ys

    def _coded_device(self, call, d_f0, f0_lengths, d_coded_sp, number_of_dimensions, d_coded_ap, extra, out_lengths, d_out, rng_pos):
        """the three coded device calls: the same arguments with `extra` between the coded rows and the output"""
        n = len(f0_lengths)
        arr, arg = _rng_arg(rng_pos, n)
        _check(call(self._h, n, _ptr(d_f0), _ints(f0_lengths), _ptr(d_coded_sp), int(number_of_dimensions), _ptr(d_coded_ap), *extra,
                    _ints(out_lengths), _ptr(d_out), arg))
        return list(arr) if arr is not None else None

    def compute_coded_device(self, d_f0, f0_lengths, d_coded_sp, number_of_dimensions, d_coded_ap, out_lengths, d_out, rng_pos=None):
        """wc_synthesis_compute_coded_device: device pointers, coded rows packed like d_f0"""
        return self._coded_device(lib().wc_synthesis_compute_coded_device, d_f0, f0_lengths, d_coded_sp, number_of_dimensions, d_coded_ap, (),
                                  out_lengths, d_out, rng_pos)

    def compute_coded_modified_device(self, d_f0, f0_lengths, d_coded_sp, number_of_dimensions, d_coded_ap, d_spectral_ratio, out_lengths, d_out,
                                      rng_pos=None):
        """wc_synthesis_compute_coded_modified_device: compute_coded_device with a spectral ratio per frame, packed like d_f0
        (0 = that frame as it is; None = compute_coded_device)"""
        return self._coded_device(lib().wc_synthesis_compute_coded_modified_device, d_f0, f0_lengths, d_coded_sp, number_of_dimensions, d_coded_ap,
                                  (_opt(d_spectral_ratio),), out_lengths, d_out, rng_pos)

    def compute_coded_retimed_device(self, d_f0, f0_lengths, d_coded_sp, number_of_dimensions, d_coded_ap, frames_out, d_position, d_f0_scale,
                                     d_spectral_ratio, out_lengths, d_out, rng_pos=None):
        """wc_synthesis_compute_coded_retimed_device: compute_coded_device along a time map -- frames_out[u] output frames per
        utterance at d_position (in source frames, io.time_map builds one), an F0 scale and a spectral ratio per output frame (None
        = none); out_lengths refer to frames_out"""
        return self._coded_device(lib().wc_synthesis_compute_coded_retimed_device, d_f0, f0_lengths, d_coded_sp, number_of_dimensions, d_coded_ap,
                                  (_ints(frames_out), _ptr(d_position), _opt(d_f0_scale), _opt(d_spectral_ratio)), out_lengths, d_out, rng_pos)

    def compute_coded_morphed_device(self, d_f0_a, a_lengths, d_coded_sp_a, d_coded_ap_a, d_f0_b, b_lengths, d_coded_sp_b, d_coded_ap_b,
                                     number_of_dimensions, frames_out, d_position_a, d_position_b, d_weight, d_f0_weight, d_ratio_a, d_ratio_b,
                                     out_lengths, d_out, rng_pos=None):
        """wc_synthesis_compute_coded_morphed_device: two voices from coded features, blended frame by frame as by
        io.morph_parameters_device -- frames_out[u] output frames per utterance at d_position_a / d_position_b with d_weight
        (d_f0_weight, d_ratio_a, d_ratio_b: None = none) -- and synthesised; out_lengths refer to frames_out"""
        n = len(frames_out)
        if not (len(a_lengths) == len(b_lengths) == n):
            raise ValueError("Synthesis.compute_coded_morphed_device: a_lengths, b_lengths and frames_out must have one entry per utterance each")
        arr, arg = _rng_arg(rng_pos, n)
        _check(lib().wc_synthesis_compute_coded_morphed_device(
            self._h, n, _ptr(d_f0_a), _ints(a_lengths), _ptr(d_coded_sp_a), _ptr(d_coded_ap_a), _ptr(d_f0_b), _ints(b_lengths), _ptr(d_coded_sp_b),
            _ptr(d_coded_ap_b), int(number_of_dimensions), _ints(frames_out), _ptr(d_position_a), _ptr(d_position_b), _ptr(d_weight),
            _opt(d_f0_weight), _opt(d_ratio_a), _opt(d_ratio_b), _ints(out_lengths), _ptr(d_out), arg))
        return list(arr) if arr is not None else None

    def _coded_args(self, f0, csp, cap, what):
        from .codec import number_of_aperiodicities
        f, csp, cap = _c(f0), _c(csp), _c(cap)
        if csp.ndim != 2 or csp.shape[0] != len(f) or cap.shape != (len(f), number_of_aperiodicities(self.fs)):
            raise ValueError(f"{what}: coded_sp must be ({len(f)}, number_of_dimensions), coded_ap ({len(f)}, {number_of_aperiodicities(self.fs)})")
        return f, csp, cap

    def compute_coded(self, f0, coded_sp, coded_ap, out_length=None):
        """one utterance from coded features (f0, mel-cepstrum, band aperiodicity) through the device call; the noise continues
        from the process-global position, as compute() does"""
        from . import DeviceArray, rng_get_position, rng_set_position
        f, csp, cap = self._coded_args(f0, coded_sp, coded_ap, "Synthesis.compute_coded")
        if out_length is None:
            out_length = self.out_length(len(f))
        d = [DeviceArray.from_host(a) for a in (f, csp, cap)]
        d_out = DeviceArray(out_length)
        try:
            pos = self.compute_coded_device(d[0], [len(f)], d[1], csp.shape[1], d[2], [out_length], d_out, [rng_get_position()])
            rng_set_position(pos[0])
            return d_out.to_host()
        finally:
            for a in d + [d_out]:
                a.free()

    def compute_batch_coded(self, f0s, csps, caps, out_lengths=None, y_pcm16=False, rng_pos=None):
        """wc_synthesis_run_batch_host_coded: ragged host arrays in, one waveform per utterance out (int16 with y_pcm16)"""
        if not (len(f0s) == len(csps) == len(caps)) or len(f0s) == 0:
            raise ValueError("Synthesis.compute_batch_coded: f0s, csps, caps must be non-empty lists of the same length")
        args = [self._coded_args(f, a, b, f"Synthesis.compute_batch_coded: utterance {u}") for u, (f, a, b) in enumerate(zip(f0s, csps, caps))]
        nd = args[0][1].shape[1]
        if any(a[1].shape[1] != nd for a in args):
            raise ValueError("Synthesis.compute_batch_coded: every coded_sp must have the same number_of_dimensions")
        fl = [len(a[0]) for a in args]
        if out_lengths is None:
            out_lengths = [self.out_length(n) for n in fl]
        if len(out_lengths) != len(fl):
            raise ValueError("Synthesis.compute_batch_coded: out_lengths must have one entry per utterance")
        ys = [np.zeros(n, dtype=np.int16 if y_pcm16 else np.float64) for n in out_lengths]
        arr, arg = _rng_arg(rng_pos, len(fl))
        _check(lib().wc_synthesis_run_batch_host_coded(self._h, len(fl), _ptr_array([a[0] for a in args]), _ints(fl),
                                                       _ptr_array([a[1] for a in args]), nd, _ptr_array([a[2] for a in args]),
                                                       _ints(out_lengths), _ptr_array(ys), 1 if y_pcm16 else 0, arg))
        return (ys, list(arr)) if rng_pos is not None else ys
