// The frame of the time-scale modification, stated once for the kernels that form it: retime_kernel and retime_stream_kernel
// (wc_retime.hip) and morph_kernel (wc_morph.hip).  One workgroup of RT_T threads per output frame; a row of fft_size/2+1 doubles
// starts on a 16-byte boundary on every other frame only, so the 16-byte accesses are issued with 8-byte alignment and the row's
// odd last bin is peeled.
#pragma once
#include <hip/hip_runtime.h>

#include "wc_stretch.hpp"

namespace wc {

constexpr int RT_T = 256;

typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));  // two bins of a row: 16 bytes at the row's 8-byte alignment

// where a position falls among n source frames: p = clamp(pos, 0, n - 1), i = floor(p), a = p - i, j = i + 1 where a > 0 (which
// implies p < n - 1: j stays inside the utterance); a position that is not finite: finite = false, frame 0
struct RtPlace {
	int i, j;
	double a, w0;
	bool finite;
};
__device__ __forceinline__ RtPlace rt_place(double pos, int n) {
	RtPlace q;
	q.finite = pos >= -1.7976931348623157e308 && pos <= 1.7976931348623157e308;
	double p = pos < 0.0 ? 0.0 : pos;
	p = p > n - 1 ? n - 1 : p;
	q.i = q.finite ? static_cast<int>(floor(p)) : 0;
	q.a = q.finite ? p - q.i : 0.0;
	q.j = q.a > 0.0 ? q.i + 1 : q.i;
	q.w0 = 1.0 - q.a;
	return q;
}

// the two source bins b, b + 1 of the frame: row ri, or (1 - a) * ri + a * rj (two products and one sum, each rounded)
__device__ __forceinline__ d2u rt_pair(const double *__restrict__ ri, const double *__restrict__ rj, double w0, double a, int b) {
	d2u x = *reinterpret_cast<const d2u *>(ri + b);
	if (a > 0.0) {
		const d2u y = *reinterpret_cast<const d2u *>(rj + b);
		x = w0 * x + a * y;
	}
	return x;
}
__device__ __forceinline__ double rt_one(const double *__restrict__ ri, const double *__restrict__ rj, double w0, double a, int b) {
	return a > 0.0 ? w0 * ri[b] + a * rj[b] : ri[b];
}

__device__ __forceinline__ void rt_row(const double *__restrict__ ri, const double *__restrict__ rj, double w0, double a,
									   double *__restrict__ out, int bins, int tid) {
	for (int t = tid; t < bins / 2; t += RT_T) *reinterpret_cast<d2u *>(out + 2 * t) = rt_pair(ri, rj, w0, a, 2 * t);
	if (tid == 0) out[bins - 1] = rt_one(ri, rj, w0, a, bins - 1);
}
__device__ __forceinline__ void rt_nan_row(double *__restrict__ out, int bins, int tid) {
	for (int b = tid; b < bins; b += RT_T) out[b] = __builtin_nan("");
}

// the frame's F0: voiced exactly where Synthesis' own interpolated voicing is (the rule of tests/retime_rule.py)
__device__ __forceinline__ double rt_f0(double fi, double fj, double w0, double a) {
	const bool vi = fi != 0.0, vj = fj != 0.0;
	if (!(a > 0.0)) return fi;
	if (vi && vj) return w0 * fi + a * fj;
	if (vi) return a < 0.5 ? fi : 0.0;
	if (vj) return a > 0.5 ? fj : 0.0;
	return 0.0;
}

// the interpolated row's logarithm to lg (LDS, kMaxBins doubles; the caller's, one row per workgroup)
__device__ __forceinline__ void rt_log_row(const double *__restrict__ ri, const double *__restrict__ rj, double w0, double a,
										   double *__restrict__ lg, int bins, int tid) {
	for (int t = tid; t < bins / 2; t += RT_T) {
		const d2u x = rt_pair(ri, rj, w0, a, 2 * t);
		lg[2 * t] = log(x.x);
		lg[2 * t + 1] = log(x.y);
	}
	if (tid == 0) lg[bins - 1] = log(rt_one(ri, rj, w0, a, bins - 1));
}

// the interpolated row of sp to LDS as its logarithm, stretched by a valid ratio (wc::stretched_bin) before its one write; lg
// (kMaxBins doubles) and fill (one) are the workgroup's LDS
__device__ __forceinline__ void rt_stretched_row(const double *__restrict__ ri, const double *__restrict__ rj, double w0, double a,
												 double *__restrict__ out, double ratio, int fs, int fft_size, int tid,
												 double *__restrict__ lg, double *__restrict__ fill) {
	const int bins = fft_size / 2 + 1;
	rt_log_row(ri, rj, w0, a, lg, bins, tid);
	__syncthreads();
	const int cut = static_cast<int>(fft_size / 2.0 * ratio);  // >= 1 for a valid ratio
	const int top = ratio < 1.0 ? cut : bins;                 // bins from `cut` upward repeat bin cut - 1
	for (int b = tid; b < top; b += RT_T) {
		const double v = stretched_bin(b, ratio, fs, fft_size, [&](int k) { return lg[k]; });
		out[b] = v;
		if (b == top - 1) *fill = v;
	}
	if (top < bins) {
		__syncthreads();
		const double f = *fill;
		for (int b = top + tid; b < bins; b += RT_T) out[b] = f;
	}
}

}  // namespace wc
