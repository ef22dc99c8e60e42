// The blend of voice morphing, stated once for the kernels that form it: morph_kernel (wc_morph.hip), morph_stream_kernel
// (wc_morph_stream.hip), track_morph_kernel (wc_track_morph.hip) and track_morph_coded_kernel (wc_track_morph_coded.hip).  Each
// voice's retimed frame comes from wc_retime_rows.hpp; what is here is what crosses the two voices: the F0 rule, a source's log
// envelope stretched by that source's ratio, and the two row blends (mp_ap_row, mp_sp_row).  A kernel brings its own placement, its
// own row pointers and its own refusals (the frame that is NaN throughout); nothing here asks who calls it.
#pragma once
#include <hip/hip_runtime.h>

#include "wc_retime_rows.hpp"
#include "wc_stretch.hpp"

namespace wc {

__device__ __forceinline__ bool mp_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

// the frame's F0 from the two retimed values: the nearer-source rule of rt_f0 across the two voices
__device__ __forceinline__ double mp_f0(double fa, double fb, double wf) {
	if (!mp_finite(wf)) return __builtin_nan("");
	if (wf == 0.0) return fa;
	if (wf == 1.0) return fb;
	const bool va = fa != 0.0, vb = fb != 0.0;
	if (va && vb) return exp((1.0 - wf) * log(fa) + wf * log(fb));
	if (va) return wf < 0.5 ? fa : 0.0;
	if (vb) return wf > 0.5 ? fb : 0.0;
	return 0.0;
}

// la(b) of a source whose interpolated row's logarithm sits in lg: the row stretched by `ratio` in the log domain (0: as it is).
// fill: the value of bin cut - 1, used from bin `top` upward (ratio < 1)
struct MpLog {
	const double *lg;
	double ratio, fill;
	int top, fs, fft_size;
	__device__ __forceinline__ double at(int b) const {
		if (ratio == 0.0) return lg[b];
		if (b >= top) return fill;
		return stretched_log_bin(b, ratio, fs, fft_size, [&](int k) { return lg[k]; });
	}
};
__device__ __forceinline__ MpLog mp_log(const double *lg, double ratio, int fs, int fft_size) {
	MpLog m;
	m.lg = lg; m.ratio = ratio; m.fs = fs; m.fft_size = fft_size;
	const int bins = fft_size / 2 + 1;
	m.top = bins;
	m.fill = 0.0;
	if (ratio != 0.0 && ratio < 1.0) {
		m.top = static_cast<int>(fft_size / 2.0 * ratio);  // >= 1 for a valid ratio
		m.fill = stretched_log_bin(m.top - 1, ratio, fs, fft_size, [&](int k) { return lg[k]; });
	}
	return m;
}

// one voice's retimed row of a frame, as the rt_* functions take it: row i, or w0 * i + a * j where a > 0
struct MpRow {
	const double *i, *j;
	double w0, a;
};

// the aperiodicity row: (1 - w) * A + w * B on the two retimed rows; w == 0 and w == 1 write the one voice's retimed row bit for bit
__device__ __forceinline__ void mp_ap_row(const MpRow &A, const MpRow &B, double w, double *__restrict__ out, int bins, int tid) {
	const double w0 = 1.0 - w;
	if (w == 0.0) rt_row(A.i, A.j, A.w0, A.a, out, bins, tid);
	else if (w == 1.0) rt_row(B.i, B.j, B.w0, B.a, out, bins, tid);
	else {
		for (int t = tid; t < bins / 2; t += RT_T) {
			const d2u x = rt_pair(A.i, A.j, A.w0, A.a, 2 * t), y = rt_pair(B.i, B.j, B.w0, B.a, 2 * t);
			*reinterpret_cast<d2u *>(out + 2 * t) = w0 * x + w * y;
		}
		if (tid == 0) out[bins - 1] = w0 * rt_one(A.i, A.j, A.w0, A.a, bins - 1) + w * rt_one(B.i, B.j, B.w0, B.a, bins - 1);
	}
}

// the envelope row: exp((1 - w) * la + w * lb) on the two log envelopes; the last statement of its kernel (w, ra and rb are the
// workgroup's: every lane takes the same path to the one barrier or past it).
// STRETCH = false: no LDS, the blend straight from registers (ra, rb unused).
// STRETCH: each voice's retimed row goes to LDS as its logarithm (two rows of kMaxBins doubles, 32 KB at fft 4096: four workgroups per
// CU of 160 KB); la(b) / lb(b) are mp_log of the row by that voice's ratio, 0 or valid.  w == 0 and w == 1 write the one voice's row
// as retime_kernel<true> writes it.
template <bool STRETCH>
__device__ __forceinline__ void mp_sp_row(const MpRow &A, const MpRow &B, double w, double ra, double rb, double *__restrict__ out, int fs,
										  int fft_size, int tid) {
	const int bins = fft_size / 2 + 1;
	const double w0 = 1.0 - w;
	if constexpr (STRETCH) {
		__shared__ double lga[kMaxBins], lgb[kMaxBins];
		__shared__ double fill;
		if (w == 0.0 || w == 1.0) {
			const bool first = w == 0.0;
			const double r = first ? ra : rb, a = first ? A.a : B.a, a0 = first ? A.w0 : B.w0;
			const double *__restrict__ ri = first ? A.i : B.i, *__restrict__ rj = first ? A.j : B.j;
			if (r == 0.0) rt_row(ri, rj, a0, a, out, bins, tid);
			else rt_stretched_row(ri, rj, a0, a, out, r, fs, fft_size, tid, lga, &fill);
			return;
		}
		rt_log_row(A.i, A.j, A.w0, A.a, lga, bins, tid);
		rt_log_row(B.i, B.j, B.w0, B.a, lgb, bins, tid);
		__syncthreads();
		const MpLog la = mp_log(lga, ra, fs, fft_size), lb = mp_log(lgb, rb, fs, fft_size);
		for (int b = tid; b < bins; b += RT_T) out[b] = exp(w0 * la.at(b) + w * lb.at(b));
	} else {
		if (w == 0.0) rt_row(A.i, A.j, A.w0, A.a, out, bins, tid);
		else if (w == 1.0) rt_row(B.i, B.j, B.w0, B.a, out, bins, tid);
		else {
			for (int t = tid; t < bins / 2; t += RT_T) {
				const d2u x = rt_pair(A.i, A.j, A.w0, A.a, 2 * t), y = rt_pair(B.i, B.j, B.w0, B.a, 2 * t);
				d2u v;
				v.x = exp(w0 * log(x.x) + w * log(y.x));
				v.y = exp(w0 * log(x.y) + w * log(y.y));
				*reinterpret_cast<d2u *>(out + 2 * t) = v;
			}
			if (tid == 0)
				out[bins - 1] = exp(w0 * log(rt_one(A.i, A.j, A.w0, A.a, bins - 1)) + w * log(rt_one(B.i, B.j, B.w0, B.a, bins - 1)));
		}
	}
}

}  // namespace wc
