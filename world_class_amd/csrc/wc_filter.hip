// Frame filtering (include/world_class_filter.h): a waveform shaped by one gain row per frame, without the vocoder.
//
//   filter_segment_wave_kernel<N>  N = 2048 / 1024: one 64-lane wavefront takes one segment, nothing crosses a workgroup barrier.  The
//                    structure is that of the unvoiced class (CLS == 2) of syn_pulse_wave_kernel with the weighted piece of the input
//                    where the noise is: the segment is loaded and weighted straight into the packed real input of the forward
//                    transform (wf_fft1024_dit + wf_r2c_unpack, the wf8 forms at 1024), its spectrum waits outside the registers
//                    (real parts in LDS, imaginary parts in the first half of the segment's own row) while the row's log gains go
//                    to their places in L and minimum_phase_wave / minimum_phase_wave8 (wc_minphase.hpp) turns them into the
//                    minimum-phase spectrum in the same paired bin layout; the complex product, wf_c2r_pack, the backward transform,
//                    and the row written to rows + seg * N.  The log of a POWER row is the lean wf_log_l; the non-finite test is one
//                    wave-wide ballot.  Two wavefronts per SIMD at 2048, as the unvoiced pulses (DESIGN 11 records what three cost
//                    there); four at 1024.
//   filter_segment_kernel<N, T>    the same rule by one workgroup per segment on minimum_phase_lds / fft_lds / r2c_post / c2r_pre, the
//                    way syn_pulse_kernel<N, T> forms its aperiodic response: fft_size 512 and 4096, and 1024 / 2048 under
//                    WC_FILTER_KERNEL=block so that the two forms can be held against each other.
//   filter_overlap_add_kernel<N>   one workgroup per tile of outputs, as syn_overlap_add_kernel.  The segments that reach a tile
//                    follow from the c_t formula (no bisection); every thread adds the rows' samples to its outputs in segment order
//                    from 0.0 and writes every sample of y.  No atomics.
//   filter_difference_kernel       the coded call's d = to - from (d[0] = 0.0 with skip_energy), in front of the codec's decoder.
// Every load and store is bounded by the utterance's own n, f_length and S; the centres c_t are computed by one expression on the
// host and on the device (ff_centre in wc_filter_stream_plan.hpp; the build contracts no product into an fma).
// The segment kernels and the difference kernel also serve the filter streams (wc_filter_stream.hip), through filter_segments_launch
// and filter_difference_launch (wc_internal.hpp): a record's t0 is the number of its first segment, 0 for the batch, and its offsets
// count from the sample a_t0 and the row t0.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <string>

#include "../../include/world_class_filter.h"
#include "wc_device.hpp"
#include "wc_features_rows.hpp"
#include "wc_filter_stream_plan.hpp"  // ff_centre, ff_segments
#include "wc_internal.hpp"
#include "wc_minphase.hpp"
#include "wc_options.hpp"
#include "wc_stages.hpp"
#include "wc_wavefft.hpp"

namespace wc {

// where a segment stands: its utterance, its number within the record, its centres and its span, counted from the record's a_t0
struct FfPlace {
	int u, t, Lt;
	long long cm, c0, cp, a;
};
__device__ __forceinline__ FfPlace ff_place(const FfArgs &a, long long seg) {
	int lo = 0, hi = a.n_utt - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (a.utts[mid].seg_off <= seg) lo = mid; else hi = mid - 1;
	}
	FfPlace p;
	p.u = lo;
	p.t = (int)(seg - a.utts[lo].seg_off);
	const int t0 = a.utts[lo].t0;
	const long long ta = (long long)t0 + p.t;  // the segment's number in the signal
	const long long base = t0 ? ff_centre((long long)t0 - 1, a.fp_ms, a.fs) + 1 : 0;
	p.cm = ta ? ff_centre(ta - 1, a.fp_ms, a.fs) - base : 0;
	p.c0 = ff_centre(ta, a.fp_ms, a.fs) - base;
	p.cp = ff_centre(ta + 1, a.fp_ms, a.fs) - base;
	p.a = ta ? p.cm + 1 : 0;
	const long long b = min((long long)a.utts[lo].n - 1, p.cp - 1);
	p.Lt = (int)(b - p.a + 1);
	return p;
}
// s_t[j] of THE rule (xs: the utterance's samples)
__device__ __forceinline__ double ff_value(const FfPlace &p, const double *__restrict__ xs, int j) {
	if (j >= p.Lt) return 0.0;
	const long long k = p.a + j;
	double w = 1.0;
	if (k < p.c0) w = (double)(k - p.cm) / (double)(p.c0 - p.cm);
	else if (k > p.c0) w = 1.0 - (double)(k - p.c0) / (double)(p.cp - p.c0);
	return xs[k] * w;
}
__device__ __forceinline__ bool ff_bad(double v) { return !(fabs(v) <= DBL_MAX); }

// ---- one workgroup per segment --------------------------------------------------------------------------------------------------
template <int N, int T>
__global__ __launch_bounds__(T) void filter_segment_kernel(FfArgs a, long long seg0) {
	constexpr int M = N / 2;
	constexpr int BPT = (M + T) / T;  // bins per thread (k <= M)
	constexpr int EPT = N / T;        // time samples per thread
	__shared__ double2 A[WC_SYN_MINPHASE_REAL ? fft_lds_size(N / 2) + 1 : fft_lds_size(N)];
	double *Ar = reinterpret_cast<double *>(A);
	int tid = threadIdx.x;
	const long long seg = seg0 + blockIdx.x;
	if (seg >= a.total_seg) return;
	const FfPlace p = ff_place(a, seg);
	const FfUtt ud = a.utts[p.u];
	const double *__restrict__ xs = a.x + ud.x_off;
	const double *__restrict__ gr = a.gain + (ud.row_off + min(p.t, ud.f_len - 1)) * (long long)(M + 1);
	double *__restrict__ row = a.rows + seg * N;
	// the weighted segment, zero behind, and its spectrum
#pragma unroll
	for (int e = 0; e < EPT; ++e) {
		const int j = tid + e * T;
		Ar[j] = ff_value(p, xs, j);
	}
	__syncthreads();
	fft_lds<M, T, +1>(A, a.tw, tid);
	r2c_post<M, T>(A, a.tw, tid);
	WC_FRESH(tid);
	double2 ns[BPT];
	double ls[BPT];
	int bad = 0;
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		const int k = tid + e * T;
		ns[e] = make_double2(0.0, 0.0);
		ls[e] = 0.0;
		if (k == 0) ns[e] = make_double2(A[0].x, 0.0);
		else if (k == M) ns[e] = make_double2(A[0].y, 0.0);
		else if (k < M) ns[e] = A[k];
		if (k <= M) {
			const double g = gr[k];
			ls[e] = a.kind == WC_FILTER_POWER ? log(g) / 2.0 : g;
			bad |= ff_bad(ls[e]);
		}
	}
	if (__syncthreads_or(bad)) {  // (the barrier in front of the analysis' first store as well)
#pragma unroll
		for (int e = 0; e < EPT; ++e) row[tid + e * T] = __builtin_nan("");
		return;
	}
	minimum_phase_lds<N, T>(A, ls, a.tw, tid);
	WC_FRESH(tid);
	double2 pr[BPT];
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		const int k = tid + e * T;
		pr[e] = make_double2(0.0, 0.0);
		if (k <= M) {
			const double2 m = A[k];
			pr[e] = make_double2(fma(m.x, ns[e].x, -(m.y * ns[e].y)), fma(m.x, ns[e].y, m.y * ns[e].x));
		}
	}
	__syncthreads();
#pragma unroll
	for (int e = 0; e < BPT; ++e) {
		const int k = tid + e * T;
		if (k > 0 && k < M) A[k] = pr[e];
		else if (k == 0) Ar[0] = pr[e].x;  // A[0] = (Y[0].re, Y[M].re)
		else if (k == M) Ar[1] = pr[e].x;
	}
	__syncthreads();
	c2r_pre<M, T>(A, a.tw, tid);
	fft_lds<M, T, -1>(A, a.tw, tid);
	WC_FRESH(tid);
#pragma unroll
	for (int e = 0; e < EPT; ++e) {
		const int j = tid + e * T;
		row[j] = Ar[j] / N;
	}
}

// ---- one wavefront per segment: N = 2048 on the 1024-point transforms, N = 1024 on the 512-point ones ------------------------------
template <int S>
__device__ __forceinline__ void ffw_dit(double (&re)[16], double (&im)[16], double *L, const double2 *__restrict__ tw, int lane) { wf_fft1024_dit<S>(re, im, L, tw, lane); }
template <int S>
__device__ __forceinline__ void ffw_dit(double (&re)[8], double (&im)[8], double *L, const double2 *__restrict__ tw, int lane) { wf8_fft512_dit<S>(re, im, L, tw, lane); }
template <int S>
__device__ __forceinline__ void ffw_dif(double (&re)[16], double (&im)[16], double *L, const double2 *__restrict__ tw, int lane) { wf_fft1024_dif<S>(re, im, L, tw, lane); }
template <int S>
__device__ __forceinline__ void ffw_dif(double (&re)[8], double (&im)[8], double *L, const double2 *__restrict__ tw, int lane) { wf8_fft512_dif<S>(re, im, L, tw, lane); }
__device__ __forceinline__ void ffw_unpack(double (&re)[16], double (&im)[16], double &nyq, const double2 *__restrict__ tw, int lane) { wf_r2c_unpack(re, im, nyq, tw, lane); }
__device__ __forceinline__ void ffw_unpack(double (&re)[8], double (&im)[8], double &nyq, const double2 *__restrict__ tw, int lane) { wf8_r2c_unpack(re, im, nyq, tw, lane); }
__device__ __forceinline__ void ffw_pack(double (&re)[16], double (&im)[16], double nyq, const double2 *__restrict__ tw, int lane) { wf_c2r_pack(re, im, nyq, tw, lane); }
__device__ __forceinline__ void ffw_pack(double (&re)[8], double (&im)[8], double nyq, const double2 *__restrict__ tw, int lane) { wf8_c2r_pack(re, im, nyq, tw, lane); }
__device__ __forceinline__ void ffw_minimum_phase(double (&mr)[16], double (&mi)[16], double &mM, double *L, const double *T, const double2 *__restrict__ tw, int lane) { minimum_phase_wave(mr, mi, mM, L, T, tw, lane); }
__device__ __forceinline__ void ffw_minimum_phase(double (&mr)[8], double (&mi)[8], double &mM, double *L, const double *T, const double2 *__restrict__ tw, int lane) { minimum_phase_wave8(mr, mi, mM, L, T, tw, lane); }
// bin held by slot s = 4 g + q of the paired layout with Q slots per lane
template <int Q>
__device__ __forceinline__ int ffw_bin(int lane, int s) { return Q == 16 ? wf_bin(lane, s >> 2, s & 3) : wf8_bin(lane, s >> 2, s & 3); }

#ifndef WC_FILTER_WAVE_OCC
#define WC_FILTER_WAVE_OCC 2  // wavefronts per SIMD at N = 2048, the unvoiced pulses' choice (WC_SYN_UNV_OCC)
#endif
#ifndef WC_FILTER_WAVE8_OCC
#define WC_FILTER_WAVE8_OCC 4
#endif
template <int N>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(N == 2048 ? WC_FILTER_WAVE_OCC : WC_FILTER_WAVE8_OCC, N == 2048 ? WC_FILTER_WAVE_OCC : WC_FILTER_WAVE8_OCC)))
void filter_segment_wave_kernel(FfArgs a, long long seg0) {
	constexpr int M = N / 2, Q = N / 128;  // Q complex points per lane
	__shared__ __attribute__((aligned(16))) double L[N == 2048 ? kWfLds : kWf8Lds];
	__shared__ __attribute__((aligned(16))) double T[kWfTabLds];
	__shared__ __attribute__((aligned(16))) double P[M];
	const int lane = threadIdx.x;
	const long long seg = seg0 + blockIdx.x;
	if (seg >= a.total_seg) return;
	wf_tables_to_lds(T, a.tw, lane);  // (requested first: in flight while the segment's own data are looked up)
	const FfPlace p = ff_place(a, seg);
	const FfUtt ud = a.utts[p.u];
	const double *__restrict__ xs = a.x + ud.x_off;
	const double *__restrict__ gr = a.gain + (ud.row_off + min(p.t, ud.f_len - 1)) * (long long)(M + 1);
	double *__restrict__ row = a.rows + seg * N;
	int ln = lane;
	WC_FRESH(ln);
	double wr[Q], wi[Q];
	double nr[Q], ni[Q], nsM = 0.0;
	// the weighted segment as the packed real input: samples 2 lane + 128 q and the next one (L_t <= M: the upper half is zero)
#pragma unroll
	for (int q = 0; q < Q; ++q) {
		nr[q] = ni[q] = 0.0;
		if (q < Q / 2 && q * 128 < p.Lt) {
			nr[q] = ff_value(p, xs, 2 * ln + 128 * q);
			ni[q] = ff_value(p, xs, 2 * ln + 128 * q + 1);
		}
	}
	ffw_dit<+1>(nr, ni, L, a.tw, ln);
	ffw_unpack(nr, ni, nsM, a.tw, ln);  // twice the segment's spectrum
	// the spectrum waits outside the registers while the minimum phase is worked out (see syn_pulse_wave_kernel): its real parts in
	// LDS, its imaginary parts in the first half of the segment's own row (free until the end)
#pragma unroll
	for (int sI = 0; sI < Q; ++sI) {
		P[64 * sI + ln] = nr[sI];
		row[64 * sI + ln] = ni[sI];
	}
	wf_fence();
	// the row's log amplitude gains, straight to their places in the transform's input
	bool bad = false;
#pragma unroll
	for (int s0 = 0; s0 < Q; s0 += 8) {
		double v[8];
#pragma unroll
		for (int q = 0; q < 8; ++q) v[q] = gr[ffw_bin<Q>(ln, s0 + q)];
		WF_SCHED_FENCE();
#pragma unroll
		for (int q = 0; q < 8; ++q) {
			const double l = a.kind == WC_FILTER_POWER ? wf_log_l(v[q], T) / 2.0 : v[q];
			bad |= ff_bad(l);
			L[ffw_bin<Q>(ln, s0 + q)] = l;
		}
	}
	{
		const double vM = gr[M];
		const double lsM = a.kind == WC_FILTER_POWER ? wf_log_l(vM, T) / 2.0 : vM;
		bad |= ff_bad(lsM);
		if (ln == 0) L[M] = lsM;
	}
	if (__builtin_amdgcn_ballot_w64(bad) != 0) {  // (wave-uniform)
#pragma unroll
		for (int q = 0; q < 2 * Q; ++q) row[64 * q + ln] = __builtin_nan("");
		return;
	}
	double mM;
	ffw_minimum_phase(wr, wi, mM, L, T, a.tw, ln);
	{
		const double *rp = row;
		asm volatile("" : "+s"(rp));  // (an opaque pointer: real loads, not the stored values kept in registers)
#pragma unroll
		for (int sI = 0; sI < Q; ++sI) {
			ni[sI] = rp[64 * sI + ln];
			nr[sI] = P[64 * sI + ln];
		}
		WF_SCHED_FENCE();
	}
#pragma unroll
	for (int sI = 0; sI < Q; ++sI) {
		const double x = wr[sI], y = wi[sI], nx = 0.5 * nr[sI], ny = 0.5 * ni[sI];
		wr[sI] = fma(x, nx, -(y * ny));
		wi[sI] = fma(x, ny, y * nx);
	}
	const double yM = mM * (0.5 * nsM);
	ffw_pack(wr, wi, yM, a.tw, ln);
	ffw_dif<-1>(wr, wi, L, a.tw, ln);
#pragma unroll
	for (int q = 0; q < Q; ++q) *reinterpret_cast<double2 *>(row + 2 * ln + 128 * q) = make_double2(wr[q] / N, wi[q] / N);
}

// ---- overlap-add ---------------------------------------------------------------------------------------------------------------------
constexpr int FO_T = 256, FO_K = 4, FO_TILE = FO_T * FO_K;
template <int N>
__global__ __launch_bounds__(FO_T) void filter_overlap_add_kernel(FfArgs a, int u0) {
	const int u = u0 + blockIdx.y;
	const FfUtt ud = a.utts[u];
	const long long t0 = (long long)blockIdx.x * FO_TILE;
	if (t0 >= ud.n) return;
	const long long last = t0 + FO_TILE - 1;
	const double h = a.fp_ms * (double)a.fs / 1000.0;
	// segment t covers outputs a_t .. a_t + N - 1 with a_t = c_{t-1} + 1 near (t - 1) h: the estimate lies at or in front of the first
	// segment that reaches the tile, the walk ends on it
	const double est = floor((double)(t0 - N) / h) - 1.0;
	int t = est > 0.0 ? (int)est : 0;
	auto start = [&](int tt) { return tt ? ff_centre(tt - 1, a.fp_ms, a.fs) + 1 : 0ll; };
	while (t < ud.S && start(t) + N <= t0) ++t;
	double acc[FO_K];
#pragma unroll
	for (int m = 0; m < FO_K; ++m) acc[m] = 0.0;
	const long long o0 = t0 + threadIdx.x;
	const double *__restrict__ rows = a.rows + ud.seg_off * N;
	constexpr int PB = 4;  // segments per trip: their loads are requested together, the additions stay in segment order
	for (; t < ud.S; t += PB) {
		if (start(t) > last) break;
		double v[PB][FO_K];
#pragma unroll
		for (int b = 0; b < PB; ++b) {
			const int tt = min(t + b, ud.S - 1);
			const long long st = start(tt);
			const bool on = t + b < ud.S && st <= last;
#pragma unroll
			for (int m = 0; m < FO_K; ++m) {
				const long long j = o0 + m * FO_T - st;
				v[b][m] = (on && j >= 0 && j < N) ? rows[(long long)tt * N + j] : 0.0;
			}
		}
#pragma unroll
		for (int b = 0; b < PB; ++b)
#pragma unroll
			for (int m = 0; m < FO_K; ++m) acc[m] += v[b][m];
	}
	double *__restrict__ out = a.y + ud.x_off;
#pragma unroll
	for (int m = 0; m < FO_K; ++m) {
		const long long o = o0 + m * FO_T;
		if (o < ud.n) out[o] = acc[m];
	}
}

__global__ __launch_bounds__(256) void filter_difference_kernel(const double *__restrict__ to, const double *__restrict__ from,
																double *__restrict__ d, long long total, int nd, int skip_energy) {
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= total) return;
	double v = from ? to[i] - from[i] : to[i];
	if (skip_energy && i % nd == 0) v = 0.0;
	d[i] = v;
}

}  // namespace wc

using namespace wc;

struct wc_frame_filter {
	int fs = 0, fft_size = 0;
	double fp_ms = 0.0;
	Device *dev = nullptr;
	bool block = false;  // WC_FILTER_KERNEL=block: the workgroup-per-segment kernel at 1024 / 2048 too
	RecPair rec;         // the utterances' records
	DevBuf rows, diff, dec;
	hipEvent_t done = nullptr;  // behind the last call's kernels: a call on another stream waits for it on the device
	hipStream_t last = nullptr;
};

namespace {

int refuse(const char *why) { return fail(WC_ERR_INVALID, std::string("frame filter: ") + why); }

int segments_of(const wc_frame_filter *f, int n) { return (int)ff_segments(n, f->fp_ms, f->fs); }

struct Totals {
	long long x = 0, frames = 0, seg = 0;
};

// everything a run call refuses, in front of the first allocation
int check(const wc_frame_filter *f, int n_utt, const double *d_x, const int *x_length, const int *f_length, const double *d_y, Totals *tot) {
	if (!f) return refuse("null handle");
	if (n_utt < 0) return refuse("n_utt < 0");
	if (n_utt == 0) return WC_OK;
	if (!x_length || !f_length) return refuse("null length array");
	for (int u = 0; u < n_utt; ++u) {
		if (x_length[u] < 0 || f_length[u] < 0) return refuse("a negative length");
		if (x_length[u] > 0 && f_length[u] < 1) return refuse("samples without a row (x_length > 0 with f_length < 1)");
		tot->x += x_length[u];
		tot->frames += f_length[u];
		tot->seg += segments_of(f, x_length[u]);
	}
	if (tot->x > 0 && (!d_x || !d_y)) return refuse("null d_x or d_y");
	if (d_y != d_x && overlap(d_y, 8ull * tot->x, d_x, 8ull * tot->x)) return refuse("d_y overlaps d_x without being d_x");
	return WC_OK;
}

constexpr int block_threads(int n) { return (n >= 2048) ? 256 : (n / 8 < 64 ? 64 : n / 8); }  // (as syn_pulse_kernel's)

template <int N>
void launch_block(const FfArgs &a, long long seg0, unsigned n, hipStream_t s) {
	hipLaunchKernelGGL((filter_segment_kernel<N, block_threads(N)>), dim3(n), dim3(block_threads(N)), 0, s, a, seg0);
}
template <int N>
void launch_ola(const FfArgs &a, int u0, unsigned tiles, unsigned nu, hipStream_t s) {
	hipLaunchKernelGGL(filter_overlap_add_kernel<N>, dim3(tiles, nu), dim3(FO_T), 0, s, a, u0);
}

}  // namespace

namespace wc {
int filter_segments_launch(Device *dev, hipStream_t s, int fft_size, bool block, const FfArgs &a) {
	const int N = fft_size;
	int rc;
	const bool wave = !block && (N == 1024 || N == 2048);
	const char *name = wave ? "filter_segment_wave_kernel" : "filter_segment_kernel";
	if ((rc = dev->time_begin(name, s))) return rc;
	constexpr long long kGrid = 1ll << 30;
	for (long long seg0 = 0; seg0 < a.total_seg; seg0 += kGrid) {
		const unsigned n = (unsigned)(a.total_seg - seg0 < kGrid ? a.total_seg - seg0 : kGrid);
		if (wave && N == 2048) hipLaunchKernelGGL(filter_segment_wave_kernel<2048>, dim3(n), dim3(64), 0, s, a, seg0);
		else if (wave) hipLaunchKernelGGL(filter_segment_wave_kernel<1024>, dim3(n), dim3(64), 0, s, a, seg0);
		else if (N == 512) launch_block<512>(a, seg0, n, s);
		else if (N == 1024) launch_block<1024>(a, seg0, n, s);
		else if (N == 2048) launch_block<2048>(a, seg0, n, s);
		else launch_block<4096>(a, seg0, n, s);
		WC_HIP(hipGetLastError());
	}
	return dev->time_end(name, s);
}
int filter_difference_launch(hipStream_t s, const double *d_to, const double *d_from, double *d_diff, long long total, int nd, int skip_energy) {
	if (total <= 0) return WC_OK;
	hipLaunchKernelGGL(filter_difference_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_to, d_from, d_diff, total, nd, skip_energy);
	WC_HIP(hipGetLastError());
	return WC_OK;
}
}  // namespace wc

namespace {

// the POWER / LOG call behind its checks
int enqueue(wc_frame_filter *f, hipStream_t s, int n_utt, const double *d_x, const int *x_length, int kind, const double *d_rows,
			const int *f_length, double *d_y, const Totals &tot) {
	Device *dev = f->dev;
	const int N = f->fft_size;
	FfUtt *h = f->rec.begin<FfUtt>(sizeof(FfUtt) * ((size_t)n_utt + 1));
	if (!h) return WC_ERR_DEVICE;
	int rc;
	if ((rc = f->rows.reserve(sizeof(double) * (size_t)tot.seg * N))) return rc;
	long long xo = 0, ro = 0, so = 0;
	int max_n = 0;
	for (int u = 0; u < n_utt; ++u) {
		const int S = segments_of(f, x_length[u]);
		h[u] = FfUtt{xo, ro, so, x_length[u], f_length[u], S, 0};
		xo += x_length[u];
		ro += f_length[u];
		so += S;
		if (x_length[u] > max_n) max_n = x_length[u];
	}
	h[n_utt] = FfUtt{xo, ro, so, 0, 0, 0, 0};
	const FfUtt *d_utts = nullptr;
	if ((rc = f->rec.upload(s, sizeof(FfUtt) * ((size_t)n_utt + 1), &d_utts))) return rc;
	FfArgs a;
	a.x = d_x; a.gain = d_rows; a.rows = f->rows.as<double>(); a.y = d_y; a.utts = d_utts; a.tw = dev->twiddle;
	a.total_seg = tot.seg; a.fp_ms = f->fp_ms; a.n_utt = n_utt; a.fs = f->fs; a.kind = kind;
	if ((rc = filter_segments_launch(dev, s, N, f->block, a))) return rc;
	if ((rc = dev->time_begin("filter_overlap_add_kernel", s))) return rc;
	const unsigned tiles = (unsigned)((max_n + FO_TILE - 1) / FO_TILE);
	for (int u0 = 0; u0 < n_utt; u0 += 65535) {
		const unsigned nu = (unsigned)(n_utt - u0 < 65535 ? n_utt - u0 : 65535);
		if (N == 512) launch_ola<512>(a, u0, tiles, nu, s);
		else if (N == 1024) launch_ola<1024>(a, u0, tiles, nu, s);
		else if (N == 2048) launch_ola<2048>(a, u0, tiles, nu, s);
		else launch_ola<4096>(a, u0, tiles, nu, s);
		WC_HIP(hipGetLastError());
	}
	return dev->time_end("filter_overlap_add_kernel", s);
}

// the handle's scratch passes from stream to stream behind an event
int take(wc_frame_filter *f, hipStream_t s) {
	if (f->done && f->last != s) WC_HIP(hipStreamWaitEvent(s, f->done, 0));
	return WC_OK;
}
int hand(wc_frame_filter *f, hipStream_t s) {
	if (!f->done) WC_HIP(hipEventCreateWithFlags(&f->done, hipEventDisableTiming));
	WC_HIP(hipEventRecord(f->done, s));
	f->last = s;
	return WC_OK;
}

}  // namespace

extern "C" {

wc_frame_filter *wc_frame_filter_create(int fs, int fft_size, double frame_period_ms) {
	const auto no = [](const char *why) { set_error(std::string("frame filter create: ") + why); return (wc_frame_filter *)nullptr; };
	if (!fft_size_supported(fft_size)) return no("fft_size must be 512, 1024, 2048 or 4096");
	if (fs <= 0) return no("fs must be positive");
	const double h = frame_period_ms * (double)fs / 1000.0;
	if (!(h >= 1.0) || !(h <= DBL_MAX)) return no("the hop frame_period_ms * fs / 1000 must be finite and at least 1");
	if (2.0 * ceil(h) - 1.0 > (double)(fft_size / 2)) return no("the longest segment, 2 * ceil(hop) - 1 samples, must fit half the transform");
	Device *dev = current_device();
	if (!dev) return nullptr;
	wc_frame_filter *f = new wc_frame_filter();
	f->fs = fs;
	f->fft_size = fft_size;
	f->fp_ms = frame_period_ms;
	f->dev = dev;
	f->block = opt_is("WC_FILTER_KERNEL", "block");
	return f;
}

void wc_frame_filter_destroy(wc_frame_filter *f) {
	if (!f) return;
	f->dev->quiesce();
	if (f->done) (void)hipEventDestroy(f->done);
	f->rec.release(); f->rows.release(); f->diff.release(); f->dec.release();
	delete f;
}

int wc_frame_filter_segments(const wc_frame_filter *f, int x_length) {
	if (!f) return refuse("null handle");
	if (x_length < 0) return refuse("a negative length");
	return segments_of(f, x_length);
}

int wc_frame_filter_run_device(wc_frame_filter *f, int n_utt, const double *d_x, const int *x_length, int kind, const double *d_rows,
							   const int *f_length, double *d_y) {
	Totals tot;
	if (int rc = check(f, n_utt, d_x, x_length, f_length, d_y, &tot)) return rc;
	if (kind != WC_FILTER_POWER && kind != WC_FILTER_LOG) return refuse("kind is 0 (power gains) or 1 (log amplitude gains)");
	if (tot.x == 0) return WC_OK;
	if (!d_rows) return refuse("null d_rows");
	if (overlap(d_y, 8ull * tot.x, d_rows, 8ull * tot.frames * (f->fft_size / 2 + 1))) return refuse("d_y overlaps d_rows");
	Device *dev = f->dev;
	DeviceLock lock(dev);
	OnDeviceOf here(dev);
	hipStream_t s = dev->active();
	int rc;
	if ((rc = take(f, s))) return rc;
	if ((rc = enqueue(f, s, n_utt, d_x, x_length, kind, d_rows, f_length, d_y, tot))) return rc;
	return hand(f, s);
}

int wc_frame_filter_run_coded_device(wc_frame_filter *f, int n_utt, const double *d_x, const int *x_length, const double *d_coded_to,
									 const double *d_coded_from, int number_of_dimensions, int skip_energy, const int *f_length,
									 double *d_y) {
	Totals tot;
	if (int rc = check(f, n_utt, d_x, x_length, f_length, d_y, &tot)) return rc;
	const int nd = number_of_dimensions;
	if (nd < 1 || nd > f->fft_size / 2) return refuse("number_of_dimensions outside 1 .. fft_size/2");
	if (tot.x == 0) return WC_OK;
	if (!d_coded_to) return refuse("null d_coded_to");
	const unsigned long long cb = 8ull * tot.frames * nd;
	if (overlap(d_y, 8ull * tot.x, d_coded_to, cb) || overlap(d_y, 8ull * tot.x, d_coded_from, cb)) return refuse("d_y overlaps the coded rows");
	Device *dev = f->dev;
	DeviceLock lock(dev);
	OnDeviceOf here(dev);
	hipStream_t s = dev->active();
	const int N = f->fft_size;
	const CodecPlan *pl;
	int rc;
	if ((rc = codec_plan(dev, f->fs, N, false, &pl))) return rc;
	if ((rc = f->diff.reserve(sizeof(double) * (size_t)tot.frames * nd))) return rc;
	if ((rc = f->dec.reserve(sizeof(double) * (size_t)tot.frames * (N / 2 + 1)))) return rc;
	if ((rc = take(f, s))) return rc;
	const long long total = tot.frames * nd;
	if ((rc = filter_difference_launch(s, d_coded_to, d_coded_from, f->diff.as<double>(), total, nd, skip_energy))) return rc;
	if ((rc = codec_decode_sp_launch(dev, s, N, tot.frames, nd, f->diff.as<double>(), f->dec.as<double>(), *pl))) return rc;
	if ((rc = enqueue(f, s, n_utt, d_x, x_length, WC_FILTER_POWER, f->dec.as<double>(), f_length, d_y, tot))) return rc;
	return hand(f, s);
}

}  // extern "C"
