// Row rules that kernels of several translation units share, each stated once:
//   the spectral stretch of the reference demo (test/test.cpp:222-240): stretch_kernel (wc_io.hip), retime_kernel<true>
//     (wc_retime.hip), decode_features_wave_kernel<true> (wc_synth_coded.hip) and, in the log domain, morph_kernel<true> (wc_morph.hip)
//   the decoded band-aperiodicity row (reference src/codec.cpp:19-40): decode_ap_kernel (wc_codec.hip) and
//     decode_features_wave_kernel
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace wc {

constexpr int kMaxBins = 4096 / 2 + 1;  // the rows of the largest fft_size

// what a frame's spectral ratio must be to stretch its row (0 = leave it is tested before): finite and cut = int(fft_size / 2 * ratio) >= 1
__host__ __device__ inline bool frame_ratio_valid(double ratio, int fft_size) {
	return ratio >= 2.0 / fft_size && ratio <= 1.7976931348623157e308;
}

// Bin i of a row stretched by `ratio`, in the log domain: reference interp1 (src/world_matlabfunctions.cpp:157-182) of the row's
// log envelope lg(k) from the stretched axis onto the plain one, with histc's clamp(#{j : axis1(j) <= xi}, 1, bins - 1) and linear
// extrapolation.  The fill of the bins from cut = int(fft_size / 2 * ratio) upward (:236-240), ratio 0 and invalid ratios are
// the caller's.  FftSize: int, or std::integral_constant where the kernel knows the size (the settling loops then compile as they do
// written out in that kernel).
template <class FftSize, class LogAt>
__device__ __forceinline__ double stretched_log_bin(int i, double ratio, int fs, FftSize size, LogAt lg) {
	const int fft_size = size;
	const int bins = fft_size / 2 + 1;
	auto axis1 = [&](int j) { return ratio * j / fft_size * fs; };  // reference test/test.cpp:222
	const double xi = static_cast<double>(i) / fft_size * fs;
	// c = #{j : axis1(j) <= xi}: start from the real-number estimate and settle with the reference's expressions
	int c = static_cast<int>(i / ratio) + 1;
	c = c < 0 ? 0 : (c > bins ? bins : c);
	while (c < bins && axis1(c) <= xi) ++c;
	while (c > 0 && !(axis1(c - 1) <= xi)) --c;
	const int k = c < 1 ? 1 : (c > bins - 1 ? bins - 1 : c);
	const double x0 = axis1(k - 1), x1 = axis1(k);
	const double s = (xi - x0) / (x1 - x0);
	const double a = lg(k - 1), b = lg(k);
	return a + s * (b - a);
}

// the bin itself: the one exp of its log-domain value (morph_kernel, wc_morph.hip, blends two such values before its exp)
template <class FftSize, class LogAt>
__device__ __forceinline__ double stretched_bin(int i, double ratio, int fs, FftSize size, LogAt lg) {
	return exp(stretched_log_bin(i, ratio, fs, size, lg));
}

constexpr double kFrequencyInterval = 3000.0, kSafeGuard = 0.000000000001;  // world_constantnumbers.hpp

// CheckVUV on the mean of a frame's n_ap coded bands c: an unvoiced frame's row stays at its initial value 1 - kSafeGuard.  No band
// (fs below 12 kHz): 0 / 0 = NaN, not unvoiced, and the row is the line from -60 dB at 0 Hz to fs/2
__device__ __forceinline__ bool coded_ap_unvoiced(const double *c, int n_ap) {
	double tmp = 0.0;
	for (int i = 0; i < n_ap; ++i) tmp += c[i];
	tmp /= n_ap;
	return tmp > -0.5;
}

// the dB value of bin j of a voiced frame's row: interp1 of (-60, the bands, -kSafeGuard) at (0, the 3 kHz multiples, fs/2); the
// caller takes 10^(v/20) of it
__device__ __forceinline__ double coded_ap_db(const double *c, int n_ap, int fs, int fft_size, int j) {
	const int na = n_ap + 2;
	auto axis = [&](int q) { return q == na - 1 ? fs / 2.0 : q * kFrequencyInterval; };
	auto val = [&](int q) { return q == 0 ? -60.0 : (q == na - 1 ? -kSafeGuard : c[q - 1]); };
	const double f = static_cast<double>(fs) / fft_size * j;
	int k = 1;  // histc: clamp(#{q : axis(q) <= f}, 1, na - 1)
	while (k < na && f >= axis(k)) ++k;
	k = k < na - 1 ? k : na - 1;
	const double x0 = axis(k - 1), x1 = axis(k);
	const double s = (f - x0) / (x1 - x0);
	return val(k - 1) + s * (val(k) - val(k - 1));
}

}  // namespace wc
