// Sample-rate conversion on the device (include/world_class_resample.h): a polyphase Kaiser-windowed-sinc resampler for rational
// ratios in FP64, as a whole-batch call and as a streaming handle.  The header states the rule; this file is its only implementation:
// the batch call and the streams run the same two kernels, and both kernels form an output in rs_output, so what a stream commits is
// bit for bit the whole call's by construction.  The filter's prototype and the host half of the handles are the variable-ratio
// converter's too: wc_resample_plan.hpp.
//
// Two mappings of outputs to lanes.
//   Phase mapping (resample_phase_kernel).  Outputs n and n + L share the table row p and their inputs lie M samples apart.  A block
//   takes a tile of R x 64 x L consecutive outputs of one signal -- it starts at a multiple of L outputs behind the signal's first, so
//   its inputs are the R x 64 x M samples from q_base plus the halo of 2K -- and puts them into local memory once.  Each wavefront then
//   takes 64 outputs of ONE phase at a time (lane i: output first + i L, inputs from q + i M): the coefficient G[p][j] is uniform over
//   the wavefront, and per tap and lane there is one 8-byte read from local memory, one multiplication and one addition.
//   Local memory is banked by 8-byte word modulo 32 for such a read, 32 lanes at a time, so a lane stride of M words is free of
//   conflicts exactly when M is odd; at 48 -> 44.1 kHz (M = 160) all 32 lanes would meet on one bank.  The tile is therefore stored
//   in rows of M words with one word of padding behind each row when M is even and at least 32: word idx sits at
//   idx + (idx div M) pad, which turns the lane stride into M + pad (odd).  A lane's taps are then contiguous up to the end of a row,
//   the same tap for every lane, so rs_output walks them in runs whose reads differ by constant offsets.  Short even rows (M = 2 at
//   48 -> 24 kHz) would make runs shorter than the unrolled loop body; their tile is split instead: even samples in one half, odd
//   ones in the other, so the lane stride is M / 2 words (odd for M = 2, 6, 10, ...; M = 4, 12 keep a two-way conflict) and a lane's
//   taps alternate between the halves, again at constant offsets.
//   Plain mapping (resample_plain_kernel).  Adjacent lanes take adjacent outputs and read inputs and coefficients from global memory.
//   It serves signals and pushes of fewer than 32 L outputs, where a wavefront of one phase would be mostly idle, and plans whose tile
//   would not fit the local memory (M above about 300).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/world_class_resample.h"
#include "wc_resample_plan.hpp"

using namespace wc;

namespace {

constexpr int kWave = 64;
constexpr int kPhaseThreads = 512;        // of the phase mapping's block, and
constexpr int kPhaseThreadsWide = 1024;   // where the tile leaves room for one block per compute unit only
#ifndef WC_RS_UNROLL
#define WC_RS_UNROLL 16
#endif
constexpr long long kLdsPreferred = 8192;   // doubles of a tile that is made longer than one wavefront row per phase (64 KB)
constexpr long long kLdsMax = 20480;        // doubles a tile may take at all: the 160 KB of a gfx950 compute unit
constexpr int kPhaseMinRows = 32;           // the phase mapping from 32 L outputs on: its wavefronts are at least half full
constexpr int kPadMinRow = 32;              // even rows of at least so many words are padded, shorter ones split (see above)
constexpr int kTasksWanted = 32;            // (wavefront, phase) tasks a tile should hold where the local memory allows

typedef __int128 wide;

// ---- the plan ---------------------------------------------------------------------------------------------------------------
constexpr char kName[] = "resample";

struct Plan {
	int L, M, K, taps;
	RsFilter f;
};

// L and M alone
const char *ratio_of(int fs_in, int fs_out, Plan *out) {
	if (fs_in < 1 || fs_out < 1) return "resample: the rates must be positive";
	if (fs_in == fs_out) return "resample: the rates are equal";
	const int g = std::gcd(fs_in, fs_out);
	out->L = fs_out / g;
	out->M = fs_in / g;
	return nullptr;
}

// the refusal's text, or empty
std::string plan_of(int fs_in, int fs_out, int zeros, double rolloff, double beta, Plan *out) {
	Plan p = {};
	if (const char *why = ratio_of(fs_in, fs_out, &p)) return why;
	const std::string why = rs_filter_check(kName, zeros, rolloff, beta);
	if (!why.empty()) return why;
	p.f = rs_filter_of(zeros, rolloff, beta, (double)p.L / p.M);
	if (!(p.K = rs_half_width(p.f, p.L))) return rs_table_refusal(kName);
	p.taps = 2 * p.K + 1;
	*out = p;
	return std::string();
}

// G[p][j] = g((k L - p) / L), k = j - K
void build_table(const Plan &p, double *G) {
	const double i0b = bessel_i0(p.f.beta);
	for (int ph = 0; ph < p.L; ++ph)
		for (int j = 0; j < p.taps; ++j) {
			const long long k = j - p.K;
			G[(size_t)ph * p.taps + j] = rs_prototype(p.f, i0b, (double)(k * p.L - ph) / (double)p.L);
		}
}

// ceil(a L / M) for a >= 0, or -1 where it leaves 63 bits
long long ceil_mul_div(long long a, int L, int M) {
	const wide v = ((wide)a * L + (M - 1)) / M;
	return v > (wide)LLONG_MAX ? -1 : (long long)v;
}

long long committed_of(const Plan &p, long long T, bool flushed) {
	if (flushed) return ceil_mul_div(T, p.L, p.M);
	if (T <= p.K) return 0;
	return std::min(ceil_mul_div(T - p.K, p.L, p.M), ceil_mul_div(T, p.L, p.M));
}

// ---- the tiling -------------------------------------------------------------------------------------------------------------
struct Tiling : RsTiles {  // tile_out: R x 64 x L; tiled_min: the phase mapping's phase_min
	int R;          // wavefront rows of 64 outputs per phase in a tile; 0: no phase mapping
	int pad;        // words of padding behind every M words of the tile
	int split;      // 1: even and odd samples apart, S = lds_words / 2 words each (short even rows)
	int lds_words;  // doubles of local memory
};

long long tile_words(const Plan &p, long long R, int pad) {
	const long long span = R * kWave * p.M + p.taps;
	return (span + span / p.M * pad + 2) / 2 * 2;  // (even: a split tile is two halves)
}

Tiling tiling_of(const Plan &p) {
	Tiling t = {};
	t.pad = p.M % 2 == 0 && p.M >= kPadMinRow ? 1 : 0;
	t.split = p.M % 2 == 0 && !t.pad ? 1 : 0;
	t.tiled_min = (long long)kPhaseMinRows * p.L;
	if (tile_words(p, 1, t.pad) > kLdsMax) return t;
	const int want = std::max(1, (kTasksWanted + p.L - 1) / p.L);
	t.R = 1;
	while (t.R < want && tile_words(p, t.R + 1, t.pad) <= kLdsPreferred) ++t.R;
	t.tile_out = t.R * kWave * p.L;
	t.lds_words = (int)tile_words(p, t.R, t.pad);
	t.lds_bytes = t.lds_words * (int)sizeof(double);
	t.threads = 2 * t.lds_words > kLdsMax ? kPhaseThreadsWide : kPhaseThreads;
	return t;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------
// one signal's share of a launch
struct RsRec {
	long long x_off;  // element of x that holds the signal's sample 0
	long long y_off;  // element of y that takes the record's first output
	long long q0;     // q of the record's first output, as a sample of the signal
	int p0;           // and its p
	int lo, hi;       // the signal's samples [lo, hi) exist; every other one reads as +0.0
	int n_out;
	int block0;       // the record's first block in its launch
	int pad_;
};
struct RsArgs {
	const RsRec *rec;
	int n_rec;
	const void *x;
	void *y;
	int L, M, K, taps;
	int R, pad, split, half, out_format;  // half: words of one half of a split tile
};

// THE output of the rule: the taps of one table row by ascending j from 0.0, every product rounded, then every sum.  `in` hands out
// x[q - K], x[q - K + 1], ... wherever the mapping keeps them, in runs: in.at(r) is the r-th sample from where `in` stands, for
// r < in.run(); in.skip(n) moves it on.  (Inside a run the addresses differ by constants, which the unrolled loop folds into the
// reads' offsets: per tap a read, a multiplication and an addition are left.)
template <class In> __device__ __forceinline__ double rs_output(In in, const double *__restrict__ g, int taps) {
#pragma clang fp contract(off)
	double acc = 0.0;
	int j = 0;
	while (j < taps) {
		const int run = min(taps - j, in.run());
#pragma unroll WC_RS_UNROLL
		for (int r = 0; r < run; ++r) {
			const double prod = in.at(r) * g[j + r];
			acc = acc + prod;
		}
		in.skip(run);
		j += run;
	}
	return acc;
}

// inputs out of the tile in local memory: `a` is the word of the lane's next sample, `m` that sample's place in its row of M (pad > 0)
struct RsTileIn {
	const double *tile;
	int a, m, M, pad;
	__device__ __forceinline__ int run() const { return pad ? M - m : INT_MAX; }
	__device__ __forceinline__ double at(int r) const { return tile[a + r]; }
	__device__ __forceinline__ void skip(int n) {
		a += n;
		m += n;
		if (pad && m == M) { m = 0; a += pad; }
	}
};
// inputs out of a split tile: sample idx sits at (idx & 1) half + (idx >> 1), so a lane stride of M samples is one of M / 2 words
// (odd for M = 2, 6, 10, ...), and a lane's taps alternate between the two halves at offsets that are constants of the unrolled loop
struct RsSplitIn {
	const double *tile;
	int even, odd, half;  // the words of the lane's samples at r = 0 and r = 1
	__device__ __forceinline__ void at_sample(int idx) {
		even = (idx & 1) * half + (idx >> 1);
		odd = ((idx + 1) & 1) * half + ((idx + 1) >> 1);
	}
	__device__ __forceinline__ int run() const { return INT_MAX; }
	__device__ __forceinline__ double at(int r) const { return tile[(r & 1 ? odd : even) + (r >> 1)]; }
	__device__ __forceinline__ void skip(int n) {
		const int e = n & 1 ? odd : even, o = n & 1 ? even + 1 : odd;
		even = e + (n >> 1);
		odd = o + (n >> 1);
	}
};
// inputs out of global memory
template <int FMT> struct RsGlobalIn {
	const void *x;
	long long x_off, i;
	int lo, hi;
	__device__ __forceinline__ int run() const { return INT_MAX; }
	__device__ __forceinline__ double at(int r) const { return i + r >= lo && i + r < hi ? rs_load<FMT>(x, x_off + i + r) : 0.0; }
	__device__ __forceinline__ void skip(int n) { i += n; }
};

// (G apart from the other arguments and __restrict__: the coefficients of a wavefront's phase then come by scalar loads)
template <int FMT> __global__ __launch_bounds__(kPhaseThreadsWide) void resample_phase_kernel(RsArgs a, const double *__restrict__ G) {
	extern __shared__ double rs_tile[];
	const RsRec r = a.rec[rs_find(a.rec, a.n_rec, (int)blockIdx.x)];
	const long long t = (long long)blockIdx.x - r.block0;
	const long long i_base = t * a.R * kWave * a.L;   // the tile's first output, counted from the record's first
	const long long q_base = r.q0 + t * a.R * kWave * a.M;  // q of an output at i_base with p = 0
	const int span = a.R * kWave * a.M + a.taps;
	for (int idx = threadIdx.x; idx < span; idx += blockDim.x) {
		const long long g = q_base - a.K + idx;
		rs_tile[a.split ? (idx & 1) * a.half + (idx >> 1) : idx + idx / a.M * a.pad] = g >= r.lo && g < r.hi ? rs_load<FMT>(a.x, r.x_off + g) : 0.0;
	}
	__syncthreads();
	const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave), lane = threadIdx.x % kWave;
	const int n_tasks = a.R * a.L;
	for (int task = wave; task < n_tasks; task += blockDim.x / kWave) {
		const int row = task / a.L, n0 = task - row * a.L;
		const long long first = i_base + (long long)row * kWave * a.L + n0;  // lane 0's output
		if (first >= r.n_out) continue;
		const long long tot = r.p0 + (long long)n0 * a.M;
		const int dq = (int)(tot / a.L), p = (int)(tot - (long long)dq * a.L);  // dq <= M
		const int off = row * kWave * a.M + dq;  // lane 0's x[q - K] as a sample of the tile
		double v;
		if (a.split) {
			RsSplitIn in;
			in.tile = rs_tile;
			in.half = a.half;
			in.at_sample(off + lane * a.M);
			v = rs_output(in, G + (size_t)p * a.taps, a.taps);
		} else {
			RsTileIn in;
			in.tile = rs_tile;
			in.M = a.M; in.pad = a.pad;
			in.m = off % a.M;
			in.a = off + off / a.M * a.pad + lane * (a.M + a.pad);
			v = rs_output(in, G + (size_t)p * a.taps, a.taps);
		}
		const long long i = first + (long long)lane * a.L;
		if (i < r.n_out) rs_store(a.y, a.out_format, r.y_off + i, v);
	}
}

template <int FMT> __global__ __launch_bounds__(kPlainBlock) void resample_plain_kernel(RsArgs a, const double *__restrict__ G) {
	const RsRec r = a.rec[rs_find(a.rec, a.n_rec, (int)blockIdx.x)];
	const long long i = ((long long)blockIdx.x - r.block0) * kPlainBlock + threadIdx.x;
	if (i >= r.n_out) return;
	const long long tot = r.p0 + i * a.M;
	const long long dq = tot / a.L;
	const int p = (int)(tot - dq * a.L);
	RsGlobalIn<FMT> in;
	in.x = a.x; in.x_off = r.x_off;
	in.i = r.q0 + dq - a.K;
	in.lo = r.lo; in.hi = r.hi;
	rs_store(a.y, a.out_format, r.y_off + i, rs_output(in, G + (size_t)p * a.taps, a.taps));
}

// ---- the handles (wc_resample_plan.hpp) around them ------------------------------------------------------------------------------
typedef RsCore<Plan, Tiling> Core;

// the table built and uploaded for a checked plan; nullptr + error on failure
Core *core_create(const Plan &p) {
	const Tiling t = tiling_of(p);
	const void *const phase_kernels[3] = {(const void *)resample_phase_kernel<0>, (const void *)resample_phase_kernel<1>, (const void *)resample_phase_kernel<2>};
	return rs_core_create<Core>(kName, "the input tile", p, t, t.R > 0, (size_t)p.L * p.taps, [&](double *G) { build_table(p, G); }, phase_kernels);
}

// the records of a launch are on the device: those of the phase mapping, then those of the plain mapping
int rs_enqueue(const Core &c, hipStream_t hs, const RsRec *d_rec, const RsSorted &s, const void *x, int in_format, void *y, int out_format) {
	RsArgs a = {};
	a.x = x; a.y = y;
	a.L = c.p.L; a.M = c.p.M; a.K = c.p.K; a.taps = c.p.taps;
	a.R = c.t.R; a.pad = c.t.pad; a.split = c.t.split; a.half = c.t.lds_words / 2; a.out_format = out_format;
	return rs_timed(c, "resample_kernels", hs, [&] {
		rs_with_format(in_format, [&](auto format) {
			constexpr int FMT = decltype(format)::value;
			rs_launch_pair(c, hs, a, d_rec, s, resample_phase_kernel<FMT>, resample_plain_kernel<FMT>);
		});
	});
}

}  // namespace

struct wc_resampler : RsBatch<Core> {};
struct wc_resample_stream : RsStreams<Core, RsStreamState> {};

extern "C" {

int wc_resample_plan(int fs_in, int fs_out, int zeros, double rolloff, double beta, int *up, int *down, int *half_width) {
	Plan p;
	const std::string why = plan_of(fs_in, fs_out, zeros, rolloff, beta, &p);
	if (!why.empty()) return fail(WC_ERR_INVALID, why);
	if (up) *up = p.L;
	if (down) *down = p.M;
	if (half_width) *half_width = p.K;
	return WC_OK;
}

int wc_resample_filter(int fs_in, int fs_out, int zeros, double rolloff, double beta, double *taps, long long capacity) {
	Plan p;
	const std::string why = plan_of(fs_in, fs_out, zeros, rolloff, beta, &p);
	if (!why.empty()) return fail(WC_ERR_INVALID, why);
	if (!taps || capacity < (long long)p.L * p.taps) return fail(WC_ERR_INVALID, "resample filter: the array holds fewer than L x (2K+1) doubles");
	build_table(p, taps);
	return WC_OK;
}

long long wc_resample_out_length(int fs_in, int fs_out, long long n_in) {
	Plan p = {};
	if (const char *why = ratio_of(fs_in, fs_out, &p)) return fail(WC_ERR_INVALID, why);
	if (n_in < 0) return fail(WC_ERR_INVALID, "resample: a negative length");
	const long long n = ceil_mul_div(n_in, p.L, p.M);
	return n < 0 ? fail(WC_ERR_INVALID, "resample: the output length leaves 63 bits") : n;
}

long long wc_resample_committed(int fs_in, int fs_out, int zeros, double rolloff, long long samples_in, int flushed) {
	Plan p;
	const std::string why = plan_of(fs_in, fs_out, zeros, rolloff, 0.0, &p);
	if (!why.empty()) return fail(WC_ERR_INVALID, why);
	if (samples_in < 0) return fail(WC_ERR_INVALID, "resample: a negative sample count");
	const long long n = committed_of(p, samples_in, flushed != 0);
	return n < 0 ? fail(WC_ERR_INVALID, "resample: the output count leaves 63 bits") : n;
}

int wc_resample_tiling(int fs_in, int fs_out, int zeros, double rolloff, int *tile_outputs, int *phase_min, int *plain_block) {
	Plan p;
	const std::string why = plan_of(fs_in, fs_out, zeros, rolloff, 0.0, &p);
	if (!why.empty()) return fail(WC_ERR_INVALID, why);
	const Tiling t = tiling_of(p);
	if (tile_outputs) *tile_outputs = t.tile_out;
	if (phase_min) *phase_min = (int)t.tiled_min;
	if (plain_block) *plain_block = kPlainBlock;
	return WC_OK;
}

// ---- batch --------------------------------------------------------------------------------------------------------------------
wc_resampler *wc_resampler_create(int fs_in, int fs_out, int zeros, double rolloff, double beta) {
	Plan p;
	const std::string why = plan_of(fs_in, fs_out, zeros, rolloff, beta, &p);
	if (!why.empty()) { set_error(why); return nullptr; }
	return rs_batch_create<wc_resampler>(core_create(p));
}

void wc_resampler_destroy(wc_resampler *r) { rs_batch_destroy(r); }

int wc_resample_device(wc_resampler *r, int n_utt, const void *d_x, int in_format, const int *x_length, void *d_y, int out_format) {
	return rs_batch_run<RsRec>(
		kName, r, x_length && d_x && d_y, n_utt, in_format, out_format, x_length,
		[&](int u, RsRec &, long long *n_out) -> const char * {
			*n_out = ceil_mul_div(x_length[u], r->c->p.L, r->c->p.M);
			return nullptr;
		},
		[&](hipStream_t hs, const RsRec *d_rec, const RsSorted &s) { return rs_enqueue(*r->c, hs, d_rec, s, d_x, in_format, d_y, out_format); });
}

// ---- streams ------------------------------------------------------------------------------------------------------------------
wc_resample_stream *wc_resample_stream_create(int fs_in, int fs_out, int zeros, double rolloff, double beta, int n_streams,
											  int max_samples_per_push) {
	if (!rs_stream_counts_ok(kName, n_streams, max_samples_per_push)) return nullptr;
	Plan p;
	const std::string why = plan_of(fs_in, fs_out, zeros, rolloff, beta, &p);
	if (!why.empty()) { set_error(why); return nullptr; }
	// a flush of a full push: committed(after, flushed) - committed(before) <= ceil((max + K) L / M)
	const long long max_out = ceil_mul_div((long long)max_samples_per_push + p.K, p.L, p.M);
	if (max_out < 0 || (wide)max_out * p.M > (wide)INT_MAX) { set_error("resample stream: max_out_per_push x M leaves 31 bits"); return nullptr; }
	return rs_stream_create<wc_resample_stream, RsRec>(core_create(p), n_streams, max_samples_per_push, (int)max_out);
}

void wc_resample_stream_destroy(wc_resample_stream *h) { rs_stream_destroy(h); }

int wc_resample_stream_max_out_per_push(const wc_resample_stream *h) { return rs_stream_max_out(h); }

int wc_resample_stream_reset(wc_resample_stream *h, int stream) { return rs_stream_reset(kName, h, stream); }

int wc_resample_stream_push_device(wc_resample_stream *h, const void *d_chunk, int in_format, const int *n_new, const int *flush,
								   void *d_y, int out_format, int *samples_out) {
	return rs_stream_push<RsRec>(
		kName, " stream push: the output count leaves 63 bits", h, d_chunk, in_format, n_new, flush, d_y, out_format, samples_out,
		// the count: what the stream has committed after the push less what it has committed
		[&](const RsStreamState &s, long long T, bool flushed) {
			const long long after = committed_of(h->c->p, T, flushed);
			return after < 0 ? -1 : after - s.committed;
		},
		// the first output: n = committed, at q = n M div L and p = n M mod L
		[&](const RsStreamState &s, RsRec &q) {
			const Plan &p = h->c->p;
			const wide nm = (wide)s.committed * p.M;
			q.q0 = (long long)(nm / p.L - ((wide)s.received - 2 * p.K));
			q.p0 = (int)(nm % p.L);
		},
		// the position is the count of committed outputs itself
		[](RsStreamState &, long long) {},
		[&](hipStream_t hs, const RsRec *d_rec, const RsSorted &s, const void *x) { return rs_enqueue(*h->c, hs, d_rec, s, x, 0, d_y, out_format); });
}

long long wc_resample_stream_samples_received(const wc_resample_stream *h, int stream) { return rs_stream_received(h, stream); }

long long wc_resample_stream_samples_committed(const wc_resample_stream *h, int stream) { return rs_stream_committed(h, stream); }

}  // extern "C"
