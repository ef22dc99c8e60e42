// Feature coding on the device (include/world_class_codec.h: wc_code_features_device; world_class_c.h:
// wc_pipeline_run_coded_device; world_class_stream.h: wc_stream_push_coded_device): the mirror image of wc_synth_coded.hip.
//
//   code_features_wave_kernel   one 64-lane wavefront per frame at fft_size 2048 and 4096, both rows of the frame in one pass:
//     spectral envelope (reference src/codec.cpp:72-90, :119-135, :267-296): log per bin into LDS -> interp1 onto the mel axis,
//       each lane straight into the slots of the packed signal z[m] = w[2 m] + i w[2 m + 1] of DCTForCodec's even/odd reordered
//       waveform w (the plan is stored in that order, so its loads are contiguous) -> complex transform of fft_size/4 points in
//       registers (wc_wavefft.hpp: wf8_fft512_dit<+1> + wf8_r2c_unpack at 2048, wf_fft1024_dit<+1> + wf_r2c_unpack at 4096) ->
//       weights -> the first nd coefficients
//     aperiodicity (:216-235): lane b codes band b with the arithmetic of code_ap_kernel (bit for bit its values)
//   A frame's coded rows depend on that frame alone.  The logarithm is wf_log_fast (~3e-16 absolute, against the 1e-11 the
//   coefficients are held to; a coefficient is a sum of fft_size/2 logs times 2 / sqrt(fft_size * fft_size/2)); a bin that is zero, negative or
//   not finite becomes NaN and with it the whole coded row of its frame, as code_sp_kernel's -inf / NaN does.
//   fft_size 512 and 1024 take the codec's workgroup-per-frame kernels (wc_codec.hip) on the cached plan.
//   The plan is wc::codec_plan's (wc_codec.hip), built and uploaded once per (device, fs, fft_size) and kept: a call then only enqueues.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/world_class_c.h"
#include "../../include/world_class_codec.h"
#include "wc_stages.hpp"
#include "wc_wavefft.hpp"

using namespace wc;

namespace {

// MD = fft_size / 2 real points: 1024 (wf8_fft512_dit, eight complex points per lane) or 2048 (wf_fft1024_dit, sixteen).
// SMALL: nd <= MD / 8, the wanted bins sit in the first slot of every group of the paired layout, so the last butterflies and
// the unpacking of the other slots' outputs are dead code and leave the kernel
template <int MD, bool SMALL>
__global__ __launch_bounds__(64) void code_features_wave_kernel(const double *__restrict__ sp, const double *__restrict__ ap,
																 double *__restrict__ csp, double *__restrict__ cap, int nd, int n_ap,
																 int fs, CodecPlanArgs p, const double2 *__restrict__ tw) {
	constexpr int BINS = MD + 1, FFT = 2 * MD, NS = MD / 128, NG = MD / 512;  // slots per lane, groups of four slots
	__shared__ double L[BINS + 7];  // the row of logarithms, then the transform's exchange buffer
	static_assert(BINS + 7 >= (MD == 1024 ? kWf8Lds : kWfLds), "exchange buffer");
	const int lane = threadIdx.x;
	const long long f = blockIdx.x;

	// ---- aperiodicity: 20 log10 at the two bins either side of each 3 kHz multiple, interp1Q (code_ap_kernel) ----
	if (ap != nullptr && lane < n_ap) {
		const double *__restrict__ row = ap + f * BINS;
		const double delta_x = static_cast<double>(fs) / FFT;
		const double xi = kFrequencyInterval * (lane + 1.0);
		const int base = static_cast<int>((xi - 0) / delta_x);
		const double frac = (xi - 0) / delta_x - base;
		const double y0 = 20 * log10(row[base]);
		const double dy = (base == BINS - 1) ? 0.0 : 20 * log10(row[base + 1]) - y0;
		cap[f * n_ap + lane] = y0 + dy * frac;
	}

	// ---- spectral envelope ----
	{
		const double *__restrict__ row = sp + f * BINS;
#pragma unroll
		for (int h = 0; h < MD / 1024; ++h) {
			double v[16];
#pragma unroll
			for (int q = 0; q < 16; ++q) v[q] = row[lane + 64 * (q + 16 * h)];
#pragma unroll
			for (int q = 0; q < 16; ++q) L[lane + 64 * (q + 16 * h)] = wf_log_ok(v[q]) ? wf_log_fast(v[q], tw) : __builtin_nan("");
		}
		const double last = lane == 0 ? row[MD] : 1.0;
		if (lane == 0) L[MD] = wf_log_ok(last) ? wf_log_fast(last, tw) : __builtin_nan("");
	}
	wf_fence();
	double re[NS], im[NS];
#pragma unroll
	for (int q = 0; q < NS; ++q) {
		// (the plan in the wavefront's order: entry (2 q + h) * 64 + lane belongs to waveform[2 (lane + 64 q) + h])
		const int ke = p.k[(2 * q) * 64 + lane], ko = p.k[(2 * q + 1) * 64 + lane];
		const double se = p.s[(2 * q) * 64 + lane], so = p.s[(2 * q + 1) * 64 + lane];
		re[q] = L[ke - 1] + se * (L[ke] - L[ke - 1]);
		im[q] = L[ko - 1] + so * (L[ko] - L[ko - 1]);
	}
	wf_fence();  // the transform's exchanges overwrite the row
	double nyq;
	if constexpr (MD == 1024) {
		wf8_fft512_dit<+1>(re, im, L, tw, lane);
		wf8_r2c_unpack(re, im, nyq, tw, lane);  // slot 4 g + c: 2 X[wf8_bin(lane, g, c)]
	} else {
		wf_fft1024_dit<+1>(re, im, L, tw, lane);
		wf_r2c_unpack(re, im, nyq, tw, lane);  // slot 4 g + c: 2 X[wf_bin(lane, g, c)]
	}
	const double normalization = sqrt((double)MD);
	double *__restrict__ out = csp + f * nd;
#pragma unroll
	for (int g = 0; g < NG; ++g)
#pragma unroll
		for (int c = 0; c < (SMALL ? 1 : 4); ++c) {
			const int i = MD == 1024 ? wf8_bin(lane, g, c) : wf_bin(lane, g, c);
			if (i < nd) {
				const double2 w = p.w[i];
				out[i] = ((0.5 * re[4 * g + c]) * w.x - (0.5 * im[4 * g + c]) * w.y) / normalization;
			}
		}
	if (!SMALL && lane == 0 && nd > MD / 2) out[MD / 2] = ((0.5 * nyq) * p.w[MD / 2].x - 0.0 * p.w[MD / 2].y) / normalization;
}

}  // namespace

const char *wc::code_features_check(int fs, int fft_size, int nd, bool with_ap) {
	if (!fft_size_supported(fft_size)) return "code_features: fft_size must be 512, 1024, 2048 or 4096";
	if (nd < 1 || nd > fft_size / 4 + 1) return "code_features: number_of_dimensions must be 1 .. fft_size/4+1";
	if (fs <= 0) return "code_features: fs must be positive";
	if (with_ap && GetNumberOfAperiodicities(fs) < 1) return "code_features: aperiodicity needs fs of at least 12 kHz (no band below)";
	return nullptr;
}

int wc::code_features_prepare(Device *dev, int fs, int fft_size) {
	const CodecPlan *pl;
	return codec_plan(dev, fs, fft_size, true, &pl);
}

int wc::code_features_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, long long n_frames, int nd, const double *d_sp,
							  const double *d_ap, double *d_coded_sp, double *d_coded_ap) {
	if (n_frames == 0) return WC_OK;
	const CodecPlan *pl;
	int rc;
	if ((rc = codec_plan(dev, fs, fft_size, true, &pl))) return rc;
	if (fft_size >= 2048) {
		const CodecPlanArgs p = pl->wave_args();
		const int n_ap = d_ap ? GetNumberOfAperiodicities(fs) : 0;
		const dim3 grid((unsigned)n_frames), block(64);
		const double2 *tw = (const double2 *)dev->twiddle;
		if (fft_size == 2048 && nd <= 128)
			hipLaunchKernelGGL((code_features_wave_kernel<1024, true>), grid, block, 0, s, d_sp, d_ap, d_coded_sp, d_coded_ap, nd, n_ap, fs, p, tw);
		else if (fft_size == 2048)
			hipLaunchKernelGGL((code_features_wave_kernel<1024, false>), grid, block, 0, s, d_sp, d_ap, d_coded_sp, d_coded_ap, nd, n_ap, fs, p, tw);
		else if (nd <= 256)
			hipLaunchKernelGGL((code_features_wave_kernel<2048, true>), grid, block, 0, s, d_sp, d_ap, d_coded_sp, d_coded_ap, nd, n_ap, fs, p, tw);
		else
			hipLaunchKernelGGL((code_features_wave_kernel<2048, false>), grid, block, 0, s, d_sp, d_ap, d_coded_sp, d_coded_ap, nd, n_ap, fs, p, tw);
		WC_HIP(hipGetLastError());
		return WC_OK;
	}
	if ((rc = codec_code_sp_launch(dev, s, fft_size, n_frames, nd, d_sp, d_coded_sp, *pl))) return rc;
	return d_ap ? codec_code_ap_launch(s, fs, fft_size, n_frames, d_ap, d_coded_ap) : WC_OK;
}

extern "C" {

int wc_code_features_device(int fs, int fft_size, long long n_frames, int number_of_dimensions, const double *d_sp, const double *d_ap,
							double *d_coded_sp, double *d_coded_ap) {
	if ((d_ap == nullptr) != (d_coded_ap == nullptr)) return fail(WC_ERR_INVALID, "code_features: d_ap and d_coded_ap go together (both NULL: spectral envelope only)");
	if (const char *why = code_features_check(fs, fft_size, number_of_dimensions, d_ap != nullptr)) return fail(WC_ERR_INVALID, why);
	if (n_frames < 0 || n_frames > 0xffffffffll) return fail(WC_ERR_INVALID, "code_features: n_frames out of range");
	if (n_frames > 0 && (!d_sp || !d_coded_sp)) return fail(WC_ERR_INVALID, "code_features: null argument");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	return code_features_enqueue(dev, dev->active(), fs, fft_size, n_frames, number_of_dimensions, d_sp, d_ap, d_coded_sp, d_coded_ap);
}

}  // extern "C"
