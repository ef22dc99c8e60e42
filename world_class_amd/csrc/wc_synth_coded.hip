// Feature decoding for Synthesis from coded features (include/world_class_codec.h: wc_decode_features_device,
// wc_decode_features_modified_device; world_class_c.h: wc_synthesis_compute_coded_device, wc_synthesis_compute_coded_modified_device;
// world_class_stream.h: wc_synth_stream_push_coded_device).
//
//   decode_features_wave_kernel<MOD>   one 64-lane wavefront per frame at fft_size 2048, both rows of the frame in one pass:
//     spectral envelope (reference src/codec.cpp:63-85, :298-325): weights -> IDCTForCodec as a BACKWARD c2c transform of
//       1024 points held in registers (wf_fft1024_dit, wc_wavefft.hpp; pruned first stage when nd <= 256) -> the even/odd
//       interleave onto the mel axis in LDS -> interp1 onto the linear axis -> exp
//     aperiodicity (:19-40, :238-267): voiced/unvoiced test on the band mean -> interp1 at 3 kHz multiples -> 10^(v/20)
//   The arithmetic of the codec's decode_sp_kernel / decode_ap_kernel (wc_codec.hip) on the same plan (wc::codec_plan) and the same
//   band-aperiodicity row (wc_stretch.hpp), except for the FFT's order of operations and 10^(v/20) as one exp: the rows differ from
//   theirs in the last bits only.  The kernel is bound by its FP64 transcendentals (an exp per bin of either row), so the second
//   stage's twiddles sit in LDS: 162 VGPRs, 3 waves per SIMD.  Other fft sizes take those workgroup-per-frame kernels, enqueued
//   on the same stream through the codec's launch helpers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <string>

#include "../../include/world_class_c.h"
#include "../../include/world_class_codec.h"
#include "wc_stages.hpp"
#include "wc_wavefft.hpp"

using namespace wc;

namespace {

constexpr double kLn10By20 = 0.11512925464970228420;  // ln(10) / 20

// MOD: the frame's row of sp stretched by rat[frame] (wc_decode_features_modified_device), the rule of stretch_kernel
// (wc::stretched_bin, wc_stretch.hpp) on the log envelope the mel row holds before the exp: the interpolation from the mel axis and
// the one along the stretched axis are both piecewise linear, so a bin takes the mel row's value at the two ends of its segment,
// interpolates and takes the one exp.  ratio 0: the unmodified expression; a ratio stretch_kernel<true> would refuse: NaN.
template <bool MOD>
__global__ __launch_bounds__(64) void decode_features_wave_kernel(const double *__restrict__ csp, const double *__restrict__ cap,
																  double *__restrict__ sp, double *__restrict__ ap, int nd, int n_ap,
																  int fs, CodecPlanArgs p, const double2 *__restrict__ tw,
																  const double *__restrict__ rat) {
	constexpr int MD = 1024, BINS = MD + 1, FFT = 2 * MD;
	__shared__ double L[kWfLds];  // the transform's exchange buffer, then the mel-axis row mel[0 .. MD + 1]
	__shared__ double T2[kWfT2Lds];  // the second stage's twiddles: out of the registers, which then leave room for 3 waves per SIMD
	const int lane = threadIdx.x;
	const long long f = blockIdx.x;
	wf_t2_to_lds(T2, tw, lane);

	// ---- spectral envelope ----
	{
		const double *__restrict__ c = csp + f * nd;
		const double normalization = sqrt((double)MD);
		double re[16], im[16];
#pragma unroll
		for (int q = 0; q < 16; ++q) {  // strided: slot q holds coefficient lane + 64 q
			const int i = lane + 64 * q;
			re[q] = 0.0;
			im[q] = 0.0;
			if (i < nd) {
				const double2 w = p.w[i];
				re[q] = c[i] * w.x * normalization;
				im[q] = -c[i] * w.y * normalization;
			}
		}
		if (nd <= 256) wdft16<-1, 1>(re, im);  // coefficients 256 .. 1023 are zero
		else wdft16<-1>(re, im);
		wf_fft1024_dit_rest<-1>(re, im, L, tw, lane, T2);
		// paired: slot 4 g + q holds X[j_g + 256 q].  mel[1 + 2 k] = Re X[k] (k < 512), mel[2048 - 2 k] = Re X[k] (k >= 512);
		// the two ends repeat their neighbours: mel[0] = X[0] (lane 0, A_0), mel[MD + 1] = X[512] (lane 0, A_2)
		const int jg[4] = {lane, lane ? 256 - lane : 128, 64 + lane, 192 - lane};
#pragma unroll
		for (int g = 0; g < 4; ++g)
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const int k = jg[g] + 256 * q;
				L[k < 512 ? 1 + 2 * k : 2048 - 2 * k] = re[4 * g + q];
			}
		if (lane == 0) {
			L[0] = re[0];
			L[MD + 1] = re[2];
		}
		wf_fence();
		double *__restrict__ row = sp + f * BINS;
		const double ratio = MOD ? rat[f] : 0.0;
		if (!MOD || ratio == 0.0) {
			for (int j = lane; j < BINS; j += 64) {
				const int k = p.k[j];
				const double v = L[k - 1] + p.s[j] * (L[k] - L[k - 1]);
				row[j] = exp(v / MD);
			}
		} else if (!frame_ratio_valid(ratio, FFT)) {
			for (int j = lane; j < BINS; j += 64) row[j] = __builtin_nan("");
		} else {
			auto mel = [&](int b) {  // the unstretched log envelope at bin b
				const int k = p.k[b];
				return (L[k - 1] + p.s[b] * (L[k] - L[k - 1])) / MD;
			};
			const int cut = static_cast<int>(FFT / 2.0 * ratio);  // >= 1 for a valid ratio
			for (int j = lane; j < BINS; j += 64) {
				const int i = (ratio < 1.0 && j >= cut) ? cut - 1 : j;  // bins from `cut` upward repeat bin cut - 1 (reference :236-240)
				row[j] = stretched_bin(i, ratio, fs, std::integral_constant<int, FFT>(), mel);
			}
		}
	}

	// ---- aperiodicity ----
	const double *__restrict__ c = cap + f * n_ap;
	double *__restrict__ row = ap + f * BINS;
	if (coded_ap_unvoiced(c, n_ap)) {
		for (int j = lane; j < BINS; j += 64) row[j] = 1.0 - kSafeGuard;
		return;
	}
	// 10^(v/20): one exp instead of pow's log + exp (within 1e-15 of it: ap <= 1, |v| <= 60)
	for (int j = lane; j < BINS; j += 64) row[j] = exp(coded_ap_db(c, n_ap, fs, FFT, j) * kLn10By20);
}

}  // namespace

const char *wc::decode_features_check(int fs, int fft_size, int nd) {
	if (!fft_size_supported(fft_size)) return "decode_features: fft_size must be 512, 1024, 2048 or 4096";
	if (nd < 1 || nd > fft_size / 2) return "decode_features: number_of_dimensions must be 1 .. fft_size/2";
	if (fs <= 0 || GetNumberOfAperiodicities(fs) < 1) return "decode_features: fs must be at least 12 kHz (no aperiodicity band below)";
	return nullptr;
}

int wc::decode_features_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, long long n_frames, int nd, const double *d_coded_sp,
								const double *d_coded_ap, const double *d_spectral_ratio, double *d_sp, double *d_ap) {
	if (n_frames == 0) return WC_OK;
	const CodecPlan *pl;
	int rc;
	if ((rc = codec_plan(dev, fs, fft_size, false, &pl))) return rc;
	// WC_DECODE_MOD=route: the stretch as a pass of its own behind the one-wavefront decoder (the measurement of DESIGN.md section 10)
	static const bool route_mod = [] { const char *e = getenv("WC_DECODE_MOD"); return e && std::string(e) == "route"; }();
	if (fft_size == 2048) {
		const dim3 grid((unsigned)n_frames), block(64);
		const int n_ap = GetNumberOfAperiodicities(fs);
		const double2 *tw = (const double2 *)dev->twiddle;
		if (d_spectral_ratio && !route_mod) {
			hipLaunchKernelGGL(decode_features_wave_kernel<true>, grid, block, 0, s, d_coded_sp, d_coded_ap, d_sp, d_ap, nd, n_ap, fs, pl->args(), tw,
							   d_spectral_ratio);
			WC_HIP(hipGetLastError());
			return WC_OK;
		}
		hipLaunchKernelGGL(decode_features_wave_kernel<false>, grid, block, 0, s, d_coded_sp, d_coded_ap, d_sp, d_ap, nd, n_ap, fs, pl->args(), tw,
						   (const double *)nullptr);
		WC_HIP(hipGetLastError());
	} else {
		if ((rc = codec_decode_sp_launch(dev, s, fft_size, n_frames, nd, d_coded_sp, d_sp, *pl))) return rc;
		if ((rc = codec_decode_ap_launch(s, fs, fft_size, n_frames, d_coded_ap, d_ap))) return rc;
	}
	return d_spectral_ratio ? modify_frames_enqueue(s, fs, fft_size, n_frames, nullptr, d_sp, nullptr, d_spectral_ratio) : WC_OK;
}

extern "C" {

int wc_decode_features_modified_device(int fs, int fft_size, long long n_frames, int number_of_dimensions, const double *d_coded_sp,
									   const double *d_coded_ap, const double *d_spectral_ratio, double *d_sp, double *d_ap) {
	if (const char *why = decode_features_check(fs, fft_size, number_of_dimensions)) return fail(WC_ERR_INVALID, why);
	if (n_frames < 0 || n_frames > 0xffffffffll) return fail(WC_ERR_INVALID, "decode_features: n_frames out of range");
	if (n_frames > 0 && (!d_coded_sp || !d_coded_ap || !d_sp || !d_ap)) return fail(WC_ERR_INVALID, "decode_features: null argument");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	return decode_features_enqueue(dev, dev->active(), fs, fft_size, n_frames, number_of_dimensions, d_coded_sp, d_coded_ap, d_spectral_ratio,
								   d_sp, d_ap);
}

int wc_decode_features_device(int fs, int fft_size, long long n_frames, int number_of_dimensions, const double *d_coded_sp,
							  const double *d_coded_ap, double *d_sp, double *d_ap) {
	return wc_decode_features_modified_device(fs, fft_size, n_frames, number_of_dimensions, d_coded_sp, d_coded_ap, nullptr, d_sp, d_ap);
}

}  // extern "C"
