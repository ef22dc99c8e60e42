// Sample-rate conversion on the device (include/world_class_resample.h): a polyphase Kaiser-windowed-sinc resampler for rational
// ratios in FP64, as a whole-batch call and as a streaming handle.  The header states the rule; this file is its only implementation:
// the batch call and the streams run the same two kernels, and both kernels form an output in rs_output, so what a stream commits is
// bit for bit the whole call's by construction.
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
#include "wc_internal.hpp"
#include "wc_resample_dev.hpp"

using namespace wc;

namespace {

constexpr int kWave = 64;
constexpr int kPhaseThreads = 512;        // of the phase mapping's block, and
constexpr int kPhaseThreadsWide = 1024;   // where the tile leaves room for one block per compute unit only
#ifndef WC_RS_UNROLL
#define WC_RS_UNROLL 16
#endif
constexpr long long kMaxTable = 1ll << 21;  // doubles
constexpr long long kLdsPreferred = 8192;   // doubles of a tile that is made longer than one wavefront row per phase (64 KB)
constexpr long long kLdsMax = 20480;        // doubles a tile may take at all: the 160 KB of a gfx950 compute unit
constexpr int kPhaseMinRows = 32;           // the phase mapping from 32 L outputs on: its wavefronts are at least half full
constexpr int kPadMinRow = 32;              // even rows of at least so many words are padded, shorter ones split (see above)
constexpr int kTasksWanted = 32;            // (wavefront, phase) tasks a tile should hold where the local memory allows

typedef __int128 wide;

// ---- the plan ---------------------------------------------------------------------------------------------------------------
struct Plan {
	int L, M, K, taps, zeros;
	double s, beta;
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

const char *plan_of(int fs_in, int fs_out, int zeros, double rolloff, double beta, Plan *out) {
	Plan p = {};
	if (const char *why = ratio_of(fs_in, fs_out, &p)) return why;
	if (zeros < 0) return "resample: zeros must be at least 1 (0: the default, 64)";
	if (!(rolloff >= 0.0 && rolloff <= 1.0)) return "resample: rolloff must lie in (0, 1] (0.0: the default)";
	if (!std::isfinite(beta) || beta < 0.0) return "resample: beta must be finite and not negative (0.0: the default)";
	if (beta > 700.0) return "resample: beta above 700 (I0 overflows)";
	p.zeros = zeros == 0 ? 64 : zeros;
	const double ro = rolloff == 0.0 ? 0.9475937167399596 : rolloff;
	p.beta = beta == 0.0 ? 14.769656459379492 : beta;
	p.s = ro * std::min(1.0, (double)p.L / p.M);
	const double kd = std::ceil(p.zeros / p.s);
	if (!(kd <= (double)kMaxTable) || (long long)p.L * (2 * (long long)kd + 1) > kMaxTable) return "resample: a table of more than 2^21 doubles";
	p.K = (int)kd;
	p.taps = 2 * p.K + 1;
	*out = p;
	return nullptr;
}

// the modified Bessel function of the first kind and order 0 by its power series: every term is positive, so the sum is good to a
// few ulp wherever it does not overflow
double bessel_i0(double x) {
	const double h = 0.25 * x * x;
	double term = 1.0, sum = 1.0;
	for (int k = 1; k < 4000; ++k) {
		term = term * h / ((double)k * k);
		sum += term;
		if (term < 1e-18 * sum) break;
	}
	return sum;
}

void build_table(const Plan &p, double *G) {
	const double pi = 3.14159265358979323846;
	const double i0b = bessel_i0(p.beta);
	for (int ph = 0; ph < p.L; ++ph)
		for (int j = 0; j < p.taps; ++j) {
			const long long k = j - p.K;
			const double d = (double)(k * p.L - ph) / (double)p.L;
			const double u = d * p.s / p.zeros;
			const double w = std::fabs(u) < 1.0 ? bessel_i0(p.beta * std::sqrt(1.0 - u * u)) / i0b : 0.0;
			const double v = p.s * d;
			G[(size_t)ph * p.taps + j] = p.s * (v == 0.0 ? 1.0 : std::sin(pi * v) / (pi * v)) * w;
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
struct Tiling {
	int R;          // wavefront rows of 64 outputs per phase in a tile; 0: no phase mapping
	int pad;        // words of padding behind every M words of the tile
	int split;      // 1: even and odd samples apart, S = lds_words / 2 words each (short even rows)
	int tile_out;   // R x 64 x L
	int lds_words;  // doubles of local memory
	int threads;    // of a block of the phase mapping
	long long phase_min;
};

long long tile_words(const Plan &p, long long R, int pad) {
	const long long span = R * kWave * p.M + p.taps;
	return (span + span / p.M * pad + 2) / 2 * 2;  // (even: a split tile is two halves)
}

Tiling tiling_of(const Plan &p) {
	Tiling t = {};
	t.pad = p.M % 2 == 0 && p.M >= kPadMinRow ? 1 : 0;
	t.split = p.M % 2 == 0 && !t.pad ? 1 : 0;
	t.phase_min = (long long)kPhaseMinRows * p.L;
	if (tile_words(p, 1, t.pad) > kLdsMax) return t;
	const int want = std::max(1, (kTasksWanted + p.L - 1) / p.L);
	t.R = 1;
	while (t.R < want && tile_words(p, t.R + 1, t.pad) <= kLdsPreferred) ++t.R;
	t.tile_out = t.R * kWave * p.L;
	t.lds_words = (int)tile_words(p, t.R, t.pad);
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

// ---- what the batch handle and the stream handle share --------------------------------------------------------------------------
struct Core {
	Plan p;
	Tiling t;
	bool phase = false;  // the phase mapping is available on this device
	Device *dev = nullptr;
	DevBuf G;
};

const void *phase_kernel(int fmt) {
	return fmt == 0 ? (const void *)resample_phase_kernel<0> : fmt == 1 ? (const void *)resample_phase_kernel<1> : (const void *)resample_phase_kernel<2>;
}

void core_destroy(Core *c) {
	if (!c) return;
	c->G.release();
	delete c;
}

// the plan checked, the table built and uploaded; nullptr + error on failure
Core *core_create(int fs_in, int fs_out, int zeros, double rolloff, double beta) {
	Plan p;
	if (const char *why = plan_of(fs_in, fs_out, zeros, rolloff, beta, &p)) { set_error(why); return nullptr; }
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	Core *c = new Core();
	c->p = p;
	c->t = tiling_of(p);
	c->dev = dev;
	std::vector<double> G((size_t)p.L * p.taps);
	build_table(p, G.data());
	if (c->G.reserve(G.size() * sizeof(double)) || hipMemcpy(c->G.p, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
		set_error("resample: the table could not be uploaded");
		c->G.release();
		delete c;
		return nullptr;
	}
	// a tile above the 64 KB every kernel may take has to be asked for.  The library is built for gfx950 alone, whose compute units
	// have the 160 KB that kLdsMax counts on: a device that grants less is an error, not a reason to change the mapping quietly
	c->phase = c->t.R > 0;
	const size_t bytes = (size_t)c->t.lds_words * sizeof(double);
	if (c->phase && bytes > 65536) {
		int limit = 0;
		bool ok = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev->id) == hipSuccess && (size_t)limit >= bytes;
		for (int fmt = 0; fmt < 3 && ok; ++fmt)
			ok = hipFuncSetAttribute(phase_kernel(fmt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
		if (!ok) {
			(void)hipGetLastError();
			set_error("resample: the device grants " + std::to_string(limit) + " bytes of local memory per workgroup, the input tile needs " + std::to_string(bytes));
			core_destroy(c);
			return nullptr;
		}
	}
	return c;
}

bool rec_is_phase(const Core &c, long long n_out) { return c.phase && n_out >= c.t.phase_min; }
int rec_blocks(const Core &c, long long n_out) {
	return rec_is_phase(c, n_out) ? (int)((n_out + c.t.tile_out - 1) / c.t.tile_out) : (int)((n_out + kPlainBlock - 1) / kPlainBlock);
}

template <int FMT> void launch_pair(const Core &c, hipStream_t hs, RsArgs a, const RsRec *d_phase, int n_phase, int blocks_phase, const RsRec *d_plain,
									int n_plain, int blocks_plain) {
	if (n_phase > 0) {
		a.rec = d_phase; a.n_rec = n_phase;
		hipLaunchKernelGGL(resample_phase_kernel<FMT>, dim3((unsigned)blocks_phase), dim3(c.t.threads), (size_t)c.t.lds_words * sizeof(double), hs, a, c.G.as<double>());
	}
	if (n_plain > 0) {
		a.rec = d_plain; a.n_rec = n_plain;
		hipLaunchKernelGGL(resample_plain_kernel<FMT>, dim3((unsigned)blocks_plain), dim3(kPlainBlock), 0, hs, a, c.G.as<double>());
	}
}

// the records of a launch are on the device: those of the phase mapping, then those of the plain mapping
int rs_enqueue(const Core &c, hipStream_t hs, const RsRec *d_rec, int n_phase, int blocks_phase, int n_plain, int blocks_plain, const void *x,
			   int in_format, void *y, int out_format) {
	RsArgs a = {};
	a.x = x; a.y = y;
	a.L = c.p.L; a.M = c.p.M; a.K = c.p.K; a.taps = c.p.taps;
	a.R = c.t.R; a.pad = c.t.pad; a.split = c.t.split; a.half = c.t.lds_words / 2; a.out_format = out_format;
	int rc;
	if ((rc = c.dev->time_begin("resample_kernels", hs))) return rc;
	if (in_format == 0) launch_pair<0>(c, hs, a, d_rec, n_phase, blocks_phase, d_rec + n_phase, n_plain, blocks_plain);
	else if (in_format == 1) launch_pair<1>(c, hs, a, d_rec, n_phase, blocks_phase, d_rec + n_phase, n_plain, blocks_plain);
	else launch_pair<2>(c, hs, a, d_rec, n_phase, blocks_phase, d_rec + n_phase, n_plain, blocks_plain);
	WC_HIP(hipGetLastError());
	return c.dev->time_end("resample_kernels", hs);
}

// the host's records sorted into the staging (phase records first, block0 assigned per launch)
struct Sorted {
	int n_phase = 0, n_plain = 0, blocks_phase = 0, blocks_plain = 0;
};
Sorted sort_records(const Core &c, const std::vector<RsRec> &recs, RsRec *to) {
	Sorted s;
	for (const RsRec &r : recs) s.n_phase += rec_is_phase(c, r.n_out) ? 1 : 0;
	int kp = 0, kq = s.n_phase;
	for (const RsRec &r : recs) {
		const bool ph = rec_is_phase(c, r.n_out);
		RsRec &d = to[ph ? kp++ : kq++];
		d = r;
		d.block0 = ph ? s.blocks_phase : s.blocks_plain;
		(ph ? s.blocks_phase : s.blocks_plain) += rec_blocks(c, r.n_out);
	}
	s.n_plain = (int)recs.size() - s.n_phase;
	return s;
}

bool format_ok(int in_format, int out_format) { return in_format >= 0 && in_format <= 2 && (out_format == 0 || out_format == 1); }

}  // namespace

struct wc_resampler {
	Core *c = nullptr;
	DevBuf drec;
	HostBuf h_rec[2];  // a pair: a call waits for the copy of the call before the last only
	int parity = 0;
};

struct wc_resample_stream {
	Core *c = nullptr;
	int n_streams = 0, max_new = 0, max_out = 0;
	long long cap = 0;  // doubles per buffer: 2K + max_new
	struct Stream {
		long long received = 0, committed = 0;
		int parity = 0;  // the buffer whose head holds the history
		bool flushed = false;
	};
	std::vector<Stream> st;
	DevBuf buf;   // n_streams x 2 x cap
	DevBuf drec;  // RsPush per stream with samples, then RsRec per stream with outputs
	HostBuf h_rec[2];
	int parity = 0;
};

extern "C" {

int wc_resample_plan(int fs_in, int fs_out, int zeros, double rolloff, double beta, int *up, int *down, int *half_width) {
	Plan p;
	if (const char *why = plan_of(fs_in, fs_out, zeros, rolloff, beta, &p)) return fail(WC_ERR_INVALID, why);
	if (up) *up = p.L;
	if (down) *down = p.M;
	if (half_width) *half_width = p.K;
	return WC_OK;
}

int wc_resample_filter(int fs_in, int fs_out, int zeros, double rolloff, double beta, double *taps, long long capacity) {
	Plan p;
	if (const char *why = plan_of(fs_in, fs_out, zeros, rolloff, beta, &p)) return fail(WC_ERR_INVALID, why);
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
	if (const char *why = plan_of(fs_in, fs_out, zeros, rolloff, 0.0, &p)) return fail(WC_ERR_INVALID, why);
	if (samples_in < 0) return fail(WC_ERR_INVALID, "resample: a negative sample count");
	const long long n = committed_of(p, samples_in, flushed != 0);
	return n < 0 ? fail(WC_ERR_INVALID, "resample: the output count leaves 63 bits") : n;
}

int wc_resample_tiling(int fs_in, int fs_out, int zeros, double rolloff, int *tile_outputs, int *phase_min, int *plain_block) {
	Plan p;
	if (const char *why = plan_of(fs_in, fs_out, zeros, rolloff, 0.0, &p)) return fail(WC_ERR_INVALID, why);
	const Tiling t = tiling_of(p);
	if (tile_outputs) *tile_outputs = t.tile_out;
	if (phase_min) *phase_min = (int)t.phase_min;
	if (plain_block) *plain_block = kPlainBlock;
	return WC_OK;
}

// ---- batch --------------------------------------------------------------------------------------------------------------------
wc_resampler *wc_resampler_create(int fs_in, int fs_out, int zeros, double rolloff, double beta) {
	Core *c = core_create(fs_in, fs_out, zeros, rolloff, beta);
	if (!c) return nullptr;
	wc_resampler *r = new wc_resampler();
	r->c = c;
	return r;
}

void wc_resampler_destroy(wc_resampler *r) {
	if (!r) return;
	r->c->dev->quiesce();
	r->drec.release(); r->h_rec[0].release(); r->h_rec[1].release();
	core_destroy(r->c);
	delete r;
}

int wc_resample_device(wc_resampler *r, int n_utt, const void *d_x, int in_format, const int *x_length, void *d_y, int out_format) {
	if (!r || !x_length || !d_x || !d_y) return fail(WC_ERR_INVALID, "resample: null argument");
	if (n_utt < 1) return fail(WC_ERR_INVALID, "resample: n_utt must be at least 1");
	if (!format_ok(in_format, out_format)) return fail(WC_ERR_INVALID, "resample: in_format is 0, 1 or 2 and out_format 0 or 1");
	const Core &c = *r->c;
	DeviceLock lock(c.dev);
	std::vector<RsRec> recs((size_t)n_utt);
	long long x_off = 0, y_off = 0;
	for (int u = 0; u < n_utt; ++u) {
		if (x_length[u] < 1) return fail(WC_ERR_INVALID, "resample: every length must be at least 1");
		const long long n_out = ceil_mul_div(x_length[u], c.p.L, c.p.M);
		if (n_out < 0 || y_off + n_out > INT_MAX) return fail(WC_ERR_INVALID, "resample: the packed output exceeds 2^31 - 1 samples");
		RsRec &q = recs[u];
		q = RsRec();
		q.x_off = x_off; q.y_off = y_off;
		q.lo = 0; q.hi = x_length[u];
		q.n_out = (int)n_out;
		x_off += x_length[u];
		y_off += n_out;
	}
	// ---- no refusal is left ----
	const size_t bytes = sizeof(RsRec) * (size_t)n_utt;
	WC_HIP(hipSetDevice(c.dev->id));
	hipStream_t hs = c.dev->active();
	HostBuf &hb = r->h_rec[r->parity];
	if (hb.reserve(bytes) || r->drec.reserve(bytes)) return WC_ERR_DEVICE;
	const Sorted s = sort_records(c, recs, hb.as<RsRec>());
	WC_HIP(hipMemcpyAsync(r->drec.p, hb.p, bytes, hipMemcpyHostToDevice, hs));
	int rc;
	if ((rc = hb.mark(hs))) return rc;
	r->parity = 1 - r->parity;
	return rs_enqueue(c, hs, r->drec.as<RsRec>(), s.n_phase, s.blocks_phase, s.n_plain, s.blocks_plain, d_x, in_format, d_y, out_format);
}

// ---- streams ------------------------------------------------------------------------------------------------------------------
wc_resample_stream *wc_resample_stream_create(int fs_in, int fs_out, int zeros, double rolloff, double beta, int n_streams,
											  int max_samples_per_push) {
	if (n_streams < 1 || max_samples_per_push < 1) { set_error("resample stream: n_streams and max_samples_per_push must be at least 1"); return nullptr; }
	Plan p;
	if (const char *why = plan_of(fs_in, fs_out, zeros, rolloff, beta, &p)) { set_error(why); return nullptr; }
	// a flush of a full push: committed(after, flushed) - committed(before) <= ceil((max + K) L / M)
	const long long max_out = ceil_mul_div((long long)max_samples_per_push + p.K, p.L, p.M);
	if (max_out < 0 || (wide)max_out * p.M > (wide)INT_MAX) { set_error("resample stream: max_out_per_push x M leaves 31 bits"); return nullptr; }
	Core *c = core_create(fs_in, fs_out, zeros, rolloff, beta);
	if (!c) return nullptr;
	DeviceLock lock(c->dev);
	wc_resample_stream *h = new wc_resample_stream();
	h->c = c;
	h->n_streams = n_streams; h->max_new = max_samples_per_push; h->max_out = (int)max_out;
	h->cap = 2ll * p.K + max_samples_per_push;
	h->st.assign((size_t)n_streams, wc_resample_stream::Stream());
	const size_t rec = (sizeof(RsPush) + sizeof(RsRec)) * (size_t)n_streams;
	if (h->buf.reserve(sizeof(double) * (size_t)n_streams * 2 * (size_t)h->cap) || h->drec.reserve(rec) || h->h_rec[0].reserve(rec) || h->h_rec[1].reserve(rec)) {
		wc_resample_stream_destroy(h);
		return nullptr;
	}
	return h;
}

void wc_resample_stream_destroy(wc_resample_stream *h) {
	if (!h) return;
	h->c->dev->quiesce();
	h->buf.release(); h->drec.release(); h->h_rec[0].release(); h->h_rec[1].release();
	core_destroy(h->c);
	delete h;
}

int wc_resample_stream_max_out_per_push(const wc_resample_stream *h) { return h ? h->max_out : WC_ERR_INVALID; }

int wc_resample_stream_reset(wc_resample_stream *h, int stream) {
	if (!h || stream < 0 || stream >= h->n_streams) return fail(WC_ERR_INVALID, "resample stream: bad stream index");
	DeviceLock lock(h->c->dev);
	// (the history is not cleared: the records say how much of it exists)
	wc_resample_stream::Stream &s = h->st[stream];
	s.received = 0; s.committed = 0; s.flushed = false;
	return WC_OK;
}

int wc_resample_stream_push_device(wc_resample_stream *h, const void *d_chunk, int in_format, const int *n_new, const int *flush,
								   void *d_y, int out_format, int *samples_out) {
	if (!h || !n_new || !samples_out) return fail(WC_ERR_INVALID, "resample stream push: null argument");
	if (!format_ok(in_format, out_format)) return fail(WC_ERR_INVALID, "resample stream push: in_format is 0, 1 or 2 and out_format 0 or 1");
	const Core &c = *h->c;
	const Plan &p = c.p;
	DeviceLock lock(c.dev);
	const int n = h->n_streams, hist = 2 * p.K;
	std::vector<long long> after((size_t)n);
	long long total_in = 0, total_out = 0;
	int n_push = 0;
	for (int u = 0; u < n; ++u) {
		const wc_resample_stream::Stream &s = h->st[u];
		if (n_new[u] < 0 || n_new[u] > h->max_new) return fail(WC_ERR_INVALID, "resample stream push: a count outside 0 .. max_samples_per_push");
		if (s.flushed && n_new[u] > 0) return fail(WC_ERR_INVALID, "resample stream push: samples for a flushed stream (reset it first)");
		const bool fl = s.flushed || (flush && flush[u]);
		after[u] = committed_of(p, s.received + n_new[u], fl);
		if (after[u] < 0) return fail(WC_ERR_INVALID, "resample stream push: the output count leaves 63 bits");
		total_in += n_new[u];
		total_out += after[u] - s.committed;
		n_push += n_new[u] > 0 ? 1 : 0;
	}
	if ((total_in > 0 && !d_chunk) || (total_out > 0 && !d_y)) return fail(WC_ERR_INVALID, "resample stream push: null array");
	// ---- no refusal is left: the records ----
	HostBuf &hb = h->h_rec[h->parity];
	if (hb.reserve(0)) return WC_ERR_DEVICE;  // (the copy of the push before the last has read this staging)
	RsPush *push = hb.as<RsPush>();
	std::vector<RsRec> recs;
	long long c_off = 0, y_off = 0;
	int kp = 0, widen_blocks = 0;
	for (int u = 0; u < n; ++u) {
		const wc_resample_stream::Stream &s = h->st[u];
		const long long cur = ((long long)u * 2 + s.parity) * h->cap, other = ((long long)u * 2 + (1 - s.parity)) * h->cap;
		if (n_new[u] > 0) {
			RsPush &w = push[kp++];
			w.c_off = c_off; w.cur_off = cur; w.other_off = other;
			w.n_new = n_new[u]; w.block0 = widen_blocks;
			widen_blocks += (n_new[u] + hist + kPlainBlock - 1) / kPlainBlock;
		}
		const long long n_out = after[u] - s.committed;
		samples_out[u] = (int)n_out;  // (<= max_out)
		if (n_out > 0) {
			// the buffer's double b is the stream's sample received - 2K + b
			const wide nm = (wide)s.committed * p.M;
			RsRec q = RsRec();
			q.x_off = cur; q.y_off = y_off;
			q.q0 = (long long)(nm / p.L - ((wide)s.received - hist));
			q.p0 = (int)(nm % p.L);
			q.lo = s.received >= hist ? 0 : (int)(hist - s.received);
			q.hi = hist + n_new[u];
			q.n_out = (int)n_out;
			recs.push_back(q);
		}
		c_off += n_new[u];
		y_off += n_out;
	}
	WC_HIP(hipSetDevice(c.dev->id));
	hipStream_t hs = c.dev->active();
	if (n_push > 0 || !recs.empty()) {
		RsRec *rec = reinterpret_cast<RsRec *>(push + n_push);
		const Sorted so = sort_records(c, recs, rec);
		const size_t bytes = sizeof(RsPush) * (size_t)n_push + sizeof(RsRec) * recs.size();
		WC_HIP(hipMemcpyAsync(h->drec.p, hb.p, bytes, hipMemcpyHostToDevice, hs));
		int rc;
		if ((rc = hb.mark(hs))) return rc;
		h->parity = 1 - h->parity;
		if (n_push > 0) {
			const RsPush *d_push = h->drec.as<RsPush>();
			double *buf = h->buf.as<double>();
			if (in_format == 0) hipLaunchKernelGGL(resample_widen_kernel<0>, dim3((unsigned)widen_blocks), dim3(kPlainBlock), 0, hs, d_push, n_push, d_chunk, buf, hist);
			else if (in_format == 1) hipLaunchKernelGGL(resample_widen_kernel<1>, dim3((unsigned)widen_blocks), dim3(kPlainBlock), 0, hs, d_push, n_push, d_chunk, buf, hist);
			else hipLaunchKernelGGL(resample_widen_kernel<2>, dim3((unsigned)widen_blocks), dim3(kPlainBlock), 0, hs, d_push, n_push, d_chunk, buf, hist);
			WC_HIP(hipGetLastError());
		}
		if (!recs.empty()) {
			const RsRec *d_rec = reinterpret_cast<const RsRec *>(h->drec.as<RsPush>() + n_push);
			if ((rc = rs_enqueue(c, hs, d_rec, so.n_phase, so.blocks_phase, so.n_plain, so.blocks_plain, h->buf.p, 0, d_y, out_format))) return rc;
		}
	}
	for (int u = 0; u < n; ++u) {
		wc_resample_stream::Stream &s = h->st[u];
		s.received += n_new[u];
		s.committed = after[u];
		if (flush && flush[u]) s.flushed = true;
		if (n_new[u] > 0) s.parity = 1 - s.parity;
	}
	return WC_OK;
}

long long wc_resample_stream_samples_received(const wc_resample_stream *h, int stream) {
	return h && stream >= 0 && stream < h->n_streams ? h->st[stream].received : -1;
}

long long wc_resample_stream_samples_committed(const wc_resample_stream *h, int stream) {
	return h && stream >= 0 && stream < h->n_streams ? h->st[stream].committed : -1;
}

}  // extern "C"
