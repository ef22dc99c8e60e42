// The blend of voice morphing, stated once for the kernels that form it: morph_kernel (wc_morph.hip) and morph_stream_kernel
// (wc_morph_stream.hip).  The two retimed frames come from wc_retime_rows.hpp; what is here is what crosses the two voices: the
// F0 rule and a source's log envelope stretched by that source's ratio.
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

}  // namespace wc
