"""Python mirror of include/world_class_codec.h: the reference's feature codec (include/codec.hpp) on the GPU."""
import ctypes as C

import numpy as np

from . import _check, _opt, _ptr, _rows
from ._binding import _binder

_dp = C.POINTER(C.c_double)
_rows_t = C.POINTER(_dp)

CODEC_SIGNATURES = {
    "GetNumberOfAperiodicities": (C.c_int, [C.c_int]),
    "CodeAperiodicity": (None, [_rows_t, C.c_int, C.c_int, C.c_int, _rows_t]),
    "DecodeAperiodicity": (None, [_rows_t, C.c_int, C.c_int, C.c_int, _rows_t]),
    "CodeSpectralEnvelope": (None, [_rows_t, C.c_int, C.c_int, C.c_int, C.c_int, _rows_t]),
    "DecodeSpectralEnvelope": (None, [_rows_t, C.c_int, C.c_int, C.c_int, C.c_int, _rows_t]),
    "wc_code_spectral_envelope_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    "wc_decode_spectral_envelope_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    "wc_code_aperiodicity_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    "wc_decode_aperiodicity_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    "wc_decode_features_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "wc_decode_features_modified_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    "wc_code_features_device": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_L = _binder(CODEC_SIGNATURES)


def number_of_aperiodicities(fs):
    return _L().GetNumberOfAperiodicities(int(fs))


def code_spectral_envelope(sp, fs, fft_size, number_of_dimensions):
    sp = np.ascontiguousarray(sp, dtype=np.float64)
    out = np.full((sp.shape[0], number_of_dimensions), np.nan)
    _L().CodeSpectralEnvelope(_rows(sp), sp.shape[0], int(fs), int(fft_size), int(number_of_dimensions), _rows(out))
    return out


def decode_spectral_envelope(coded, fs, fft_size):
    coded = np.ascontiguousarray(coded, dtype=np.float64)
    out = np.full((coded.shape[0], fft_size // 2 + 1), np.nan)
    _L().DecodeSpectralEnvelope(_rows(coded), coded.shape[0], int(fs), int(fft_size), coded.shape[1], _rows(out))
    return out


def code_aperiodicity(ap, fs, fft_size):
    ap = np.ascontiguousarray(ap, dtype=np.float64)
    out = np.full((ap.shape[0], number_of_aperiodicities(fs)), np.nan)
    _L().CodeAperiodicity(_rows(ap), ap.shape[0], int(fs), int(fft_size), _rows(out))
    return out


def decode_aperiodicity(coded, fs, fft_size):
    coded = np.ascontiguousarray(coded, dtype=np.float64)
    out = np.full((coded.shape[0], fft_size // 2 + 1), np.nan)
    _L().DecodeAperiodicity(_rows(coded), coded.shape[0], int(fs), int(fft_size), _rows(out))
    return out


def code_spectral_envelope_device(fs, fft_size, n_frames, number_of_dimensions, d_sp, d_coded):
    _check(_L().wc_code_spectral_envelope_device(int(fs), int(fft_size), int(n_frames), int(number_of_dimensions), _ptr(d_sp), _ptr(d_coded)))


def decode_spectral_envelope_device(fs, fft_size, n_frames, number_of_dimensions, d_coded, d_sp):
    _check(_L().wc_decode_spectral_envelope_device(int(fs), int(fft_size), int(n_frames), int(number_of_dimensions), _ptr(d_coded), _ptr(d_sp)))


def code_aperiodicity_device(fs, fft_size, n_frames, d_ap, d_coded):
    _check(_L().wc_code_aperiodicity_device(int(fs), int(fft_size), int(n_frames), _ptr(d_ap), _ptr(d_coded)))


def decode_aperiodicity_device(fs, fft_size, n_frames, d_coded, d_ap):
    _check(_L().wc_decode_aperiodicity_device(int(fs), int(fft_size), int(n_frames), _ptr(d_coded), _ptr(d_ap)))


def decode_features_device(fs, fft_size, n_frames, number_of_dimensions, d_coded_sp, d_coded_ap, d_sp, d_ap):
    """both coded rows of n_frames frames -> spectrogram and aperiodicity rows (fft_size/2+1 each), one pass on the device"""
    _check(_L().wc_decode_features_device(int(fs), int(fft_size), int(n_frames), int(number_of_dimensions), _ptr(d_coded_sp),
                                          _ptr(d_coded_ap), _ptr(d_sp), _ptr(d_ap)))


def decode_features_modified_device(fs, fft_size, n_frames, number_of_dimensions, d_coded_sp, d_coded_ap, d_spectral_ratio, d_sp, d_ap):
    """decode_features_device with the spectral rows stretched frame by frame (io.modify_parameters_frames_device's rules for
    d_spectral_ratio, one double per frame); None: decode_features_device"""
    _check(_L().wc_decode_features_modified_device(int(fs), int(fft_size), int(n_frames), int(number_of_dimensions), _ptr(d_coded_sp),
                                                   _ptr(d_coded_ap), _opt(d_spectral_ratio), _ptr(d_sp), _ptr(d_ap)))


def code_features_device(fs, fft_size, n_frames, number_of_dimensions, d_sp, d_ap, d_coded_sp, d_coded_ap):
    """spectrogram and aperiodicity rows of n_frames frames -> both coded rows, one pass on the device, enqueue-only;
    d_ap and d_coded_ap both None: the spectral envelope alone"""
    _check(_L().wc_code_features_device(int(fs), int(fft_size), int(n_frames), int(number_of_dimensions), _ptr(d_sp),
                                        _opt(d_ap), _ptr(d_coded_sp), _opt(d_coded_ap)))
