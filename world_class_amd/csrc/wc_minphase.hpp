// The three forms of the minimum-phase analysis, stated once for the translation units that turn a log spectrum into a causal
// response: Synthesis (wc_synthesis.hip) and the frame filter (wc_filter.hip).  minimum_phase_lds is the workgroup form at every
// size; minimum_phase_wave (N = 2048) and minimum_phase_wave8 (N = 1024) live in the registers of one wavefront on the transforms
// of wc_wavefft.hpp.  tests/test_gpu_minimum_phase.py holds each of them to tests/minimum_phase_rule.py through
// wc_debug_minimum_phase (wc_synthesis.hip).
#pragma once
#include "wc_device.hpp"
#include "wc_wavefft.hpp"

namespace wc {

// MinimumPhaseAnalysis::compute (reference src/world_common.cpp:196-233) for the block.
// ls[BPT]: log spectrum of this thread's bins k = tid + e T (k <= M).  On return A[0..M] holds the
// minimum-phase spectrum (full complex, M+1 entries).  Ends with a __syncthreads().
#ifndef WC_SYN_MINPHASE_REAL
#define WC_SYN_MINPHASE_REAL 1
#endif
template <int N, int T>
__device__ __forceinline__ void minimum_phase_lds(double2 *A, const double (&ls)[(N / 2 + T) / T],
												  const double2 *__restrict__ tw, int tid) {
	constexpr int M = N / 2;
	constexpr int BPT = (M + T) / T;
	double *Ar = reinterpret_cast<double *>(A);
	WC_FRESH(tid);
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		int k = tid + e * T;
		if (k <= M) {
			Ar[k] = ls[e];
			if (k > 0 && k < M) Ar[N - k] = ls[e];  // mirroring (reference :199-200)
		}
	}
	__syncthreads();
	fft_lds<M, T, +1>(A, tw, tid);
	r2c_post<M, T>(A, tw, tid);
	WC_FRESH(tid);
#if WC_SYN_MINPHASE_REAL
	// cepstrum folding (reference :207-217): bins 1..M-1 doubled (and conjugated), upper half zeroed.  The cepstrum of a
	// real even log spectrum is real -- the imaginary parts the reference carries along are its FFT's rounding noise,
	// 1e-16 of the real parts -- so the second transform is taken as a real one too (an M-point complex FFT and the
	// unpacking pass instead of an N-point complex FFT; SYN_MINPHASE_REAL=0 keeps the complex transform for comparison).
	double cr[2 * BPT];  // this thread's real samples n = tid + e T, n < N
#pragma unroll
	for (int e = 0; e < 2 * BPT; ++e) {
		int n = tid + e * T;
		cr[e] = 0.0;
		if (n == 0) cr[e] = A[0].x;
		else if (n == M) cr[e] = A[0].y;
		else if (n < M) cr[e] = A[n].x * 2.0;
	}
	__syncthreads();
#pragma unroll
	for (int e = 0; e < 2 * BPT; ++e) {
		int n = tid + e * T;
		if (n < N) Ar[n] = cr[e];
	}
	__syncthreads();
	fft_lds<M, T, +1>(A, tw, tid);
	r2c_post<M, T>(A, tw, tid);
	WC_FRESH(tid);
	double2 c[BPT];
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		int k = tid + e * T;
		if (k <= M) {
			double2 m = (k == 0) ? make_double2(A[0].x, 0.0) : (k == M) ? make_double2(A[0].y, 0.0) : A[k];
			double t = exp(m.x / N), sn, cs;
			sincos(m.y / N, &sn, &cs);
			c[e] = make_double2(t * cs, t * sn);
		}
	}
#else
	// cepstrum folding (reference :207-217): bins 1..M-1 doubled and conjugated, upper half zeroed
	double2 c[BPT];
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		int k = tid + e * T;
		c[e] = make_double2(0.0, 0.0);
		if (k == 0) c[e] = make_double2(A[0].x, 0.0);
		else if (k == M) c[e] = make_double2(A[0].y, 0.0);
		else if (k < M) c[e] = make_double2(A[k].x * 2.0, A[k].y * -2.0);
	}
	__syncthreads();
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		int k = tid + e * T;
		if (k <= M) A[k] = c[e];
		if (k >= 1 && k < M) A[M + k] = make_double2(0.0, 0.0);
	}
	__syncthreads();
	fft_lds<N, T, +1>(A, tw, tid);
	WC_FRESH(tid);
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		int k = tid + e * T;
		if (k <= M) {
			double2 m = A[k];
			double t = exp(m.x / N), sn, cs;
			sincos(m.y / N, &sn, &cs);
			c[e] = make_double2(t * cs, t * sn);
		}
	}
#endif
	__syncthreads();
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		int k = tid + e * T;
		if (k <= M) A[k] = c[e];
	}
	__syncthreads();
}

// ==== N = 2048: one wavefront, 16 complex points per lane, bins in the "paired" layout ==========================================
// MinimumPhaseAnalysis::compute (reference src/world_common.cpp:196-233): in: the log spectrum ls[4 g + q] of bin
// j_g + 256 q and lsM of bin 1024 (lane 0); out: the minimum-phase spectrum (mr, mi) in the same layout, (mMr, 0) for bin 1024.
// (the caller has put the log spectrum into L itself, value by value as it formed them: L[bin], bins 0 .. 1024)
__device__ __forceinline__ void minimum_phase_wave(double (&mr)[16], double (&mi)[16], double &mMr,
												   double *L, const double *T, const double2 *__restrict__ tw, int lane) {
	constexpr int N = 2048, M = 1024;
	WC_FRESH(lane);
	int jg[4];
#pragma unroll
	for (int g = 0; g < 4; ++g) jg[g] = wf_bin(lane, g, 0);
	// the mirrored log spectrum (reference :199-200) as the packed input of the first transform
	wf_fence();
#pragma unroll
	for (int q = 0; q < 8; ++q) {
		const double2 v = *reinterpret_cast<const double2 *>(&L[2 * lane + 128 * q]);
		mr[q] = v.x;
		mi[q] = v.y;
	}
#pragma unroll
	for (int q = 8; q < 16; ++q) {
		mr[q] = L[2048 - 2 * lane - 128 * q];
		mi[q] = L[2047 - 2 * lane - 128 * q];
	}
	wf_fence();
	wf_fft1024_dit<+1>(mr, mi, L, tw, lane);
	double nyq;
	wf_r2c_unpack_re(mr, mi, nyq, tw, lane);  // twice the (real) cepstrum
	// folding (reference :207-217): bins 1 .. M-1 doubled, 0 and M kept, the upper half zero; the cepstrum of a real even log
	// spectrum is real, so the second transform is a real one too (see minimum_phase_lds)
#pragma unroll
	for (int g = 0; g < 4; ++g)
#pragma unroll
		for (int q = 0; q < 4; ++q) L[jg[g] + 256 * q] = (g == 0 && q == 0 && lane == 0) ? 0.5 * mr[0] : mr[4 * g + q];
	if (lane == 0) L[M] = 0.5 * nyq;
	wf_fence();
#pragma unroll
	for (int q = 0; q < 8; ++q) {
		const double2 v = *reinterpret_cast<const double2 *>(&L[2 * lane + 128 * q]);
		mr[q] = v.x;
		mi[q] = v.y;
	}
	mr[8] = lane == 0 ? L[M] : 0.0;
	mi[8] = 0.0;
#pragma unroll
	for (int q = 9; q < 16; ++q) mr[q] = mi[q] = 0.0;
	wf_fence();
	wf_fft1024_dit<+1>(mr, mi, L, tw, lane);
	wf_r2c_unpack(mr, mi, nyq, tw, lane);  // twice the spectrum of the folded cepstrum
#pragma unroll
	for (int s = 0; s < 16; ++s) {
		const double t = wf_exp_l(mr[s] * (0.5 / N), T);
		double sn, cs;
		wf_sincos(mi[s] * (0.5 / N), sn, cs);
		mr[s] = t * cs;
		mi[s] = t * sn;
	}
	mMr = wf_exp_l(nyq * (0.5 / N), T);
}

// ==== N = 1024: the same on the 512-point transforms wf8_*, eight points per lane; in: ls[4 g + q] of bin wf8_bin(lane, g, q) in L[bin],
// bin 512 in L[512] ============================================================================================================
__device__ __forceinline__ void minimum_phase_wave8(double (&mr)[8], double (&mi)[8], double &mMr,
													double *L, const double *T, const double2 *__restrict__ tw, int lane) {
	constexpr int N = 1024, M = 512;
	WC_FRESH(lane);
	int jg[2];
#pragma unroll
	for (int g = 0; g < 2; ++g) jg[g] = wf8_bin(lane, g, 0);
	// the mirrored log spectrum (reference :199-200) as the packed input of the first transform
	wf_fence();
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const double2 v = *reinterpret_cast<const double2 *>(&L[2 * lane + 128 * q]);
		mr[q] = v.x;
		mi[q] = v.y;
	}
#pragma unroll
	for (int q = 4; q < 8; ++q) {
		mr[q] = L[1024 - 2 * lane - 128 * q];
		mi[q] = L[1023 - 2 * lane - 128 * q];
	}
	wf_fence();
	wf8_fft512_dit<+1>(mr, mi, L, tw, lane);
	double nyq;
	wf8_r2c_unpack_re(mr, mi, nyq, tw, lane);  // twice the (real) cepstrum
	// folding (reference :207-217): bins 1 .. M-1 doubled, 0 and M kept, the upper half zero (see minimum_phase_wave)
#pragma unroll
	for (int g = 0; g < 2; ++g)
#pragma unroll
		for (int q = 0; q < 4; ++q) L[jg[g] + 128 * q] = (g == 0 && q == 0 && lane == 0) ? 0.5 * mr[0] : mr[4 * g + q];
	if (lane == 0) L[M] = 0.5 * nyq;
	wf_fence();
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const double2 v = *reinterpret_cast<const double2 *>(&L[2 * lane + 128 * q]);
		mr[q] = v.x;
		mi[q] = v.y;
	}
	mr[4] = lane == 0 ? L[M] : 0.0;
	mi[4] = 0.0;
#pragma unroll
	for (int q = 5; q < 8; ++q) mr[q] = mi[q] = 0.0;
	wf_fence();
	wf8_fft512_dit<+1>(mr, mi, L, tw, lane);
	wf8_r2c_unpack(mr, mi, nyq, tw, lane);  // twice the spectrum of the folded cepstrum
#pragma unroll
	for (int s = 0; s < 8; ++s) {
		const double t = wf_exp_l(mr[s] * (0.5 / N), T);
		double sn, cs;
		wf_sincos(mi[s] * (0.5 / N), sn, cs);
		mr[s] = t * cs;
		mi[s] = t * sn;
	}
	mMr = wf_exp_l(nyq * (0.5 / N), T);
}

}  // namespace wc
