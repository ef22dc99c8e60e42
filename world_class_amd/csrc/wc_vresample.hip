// Variable-ratio sample-rate conversion on the device (include/world_class_vresample.h): the Kaiser-windowed sinc of wc_resample.hip
// read at a continuous phase out of a table of piecewise polynomials, as a whole-batch call with a step per utterance and as a streaming
// handle whose steps move between pushes.  The header states the rule; this file is its only implementation: the batch call and the
// streams run the same two kernels, and both kernels form an output in vr_output, so what a stream commits is bit for bit the whole
// call's by construction.  The filter's prototype and the host half of the handles are the rational converter's too:
// wc_resample_plan.hpp.
//
// Two mappings of outputs to lanes.
//   Segment mapping (vresample_segment_kernel).  Outputs whose fractions f fall into the same segment share the D+1 coefficients of
//   every tap.  A block takes a tile of consecutive outputs of one signal, puts their inputs -- floor(tile x step / 2^32) + 2K + 2
//   samples at most, sized for step_max -- into local memory once, and buckets the tile's outputs by segment with a counting sort in
//   local memory.  Each wavefront then takes 64 outputs of ONE segment at a time: the coefficients C[seg][j][0 .. D] are uniform over
//   the wavefront, and per tap and lane there is one 8-byte read from local memory and D+1 multiplications and additions in
//   independent chains.  Where an output lands in its bucket decides nothing about its value, so the sort may fill the buckets in any
//   order; a bucket may hold the whole tile (step = 2^32 keeps every output of a tile in one segment).
//   Plain mapping (vresample_plain_kernel).  Adjacent lanes take adjacent outputs and read inputs and their own segment's rows from
//   global memory.  It serves signals and pushes of fewer than segment_min outputs and plans whose tile would not fit the local memory.
// Warping (include/world_class_warp.h) is the same rule at positions read from device memory, one per output: warp_segment_kernel and
// warp_plain_kernel are the two mappings again, on the same tiling, sort (vr_sort_starts, vr_sort_place), task loop (vr_tasks) and vr_output, so at
// the positions n x step they give wc_vresample_device's bits; warp_map_kernel turns frame-level time maps into such positions.
// Where the positions come from is a template argument of the two kernels: an array (wc_warp_device), or the map rule evaluated
// where the array would have been read (include/world_class_warp_stream.h: wc_warp_along_map_device and the warp streams, whose
// pushes are that call's records with a first output and a first entry of their own).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/world_class_warp_stream.h"  // (with world_class_warp.h and world_class_vresample.h)
#include "wc_resample_plan.hpp"

using namespace wc;

namespace {

constexpr int kWave = 64;
constexpr int kSegThreads = 512;        // of the segment mapping's block, and
constexpr int kSegThreadsWide = 1024;   // where the tile leaves room for one block per compute unit only
#ifndef WC_VR_UNROLL
#define WC_VR_UNROLL 4
#endif
#ifndef WC_VR_FORCE_PLAIN
#define WC_VR_FORCE_PLAIN 0   // 1: a variant build for measurements that never takes the segment mapping
#endif
constexpr int kMaxSegments = 256;
constexpr int kMaxDegree = 7;
#ifndef WC_VR_TILE_MAX
#define WC_VR_TILE_MAX 8192
#endif
constexpr int kTileMax = WC_VR_TILE_MAX, kTileMin = 256;  // outputs of a tile: a power of two in between (an output's place in its tile is 16 bits)
constexpr long long kLdsPreferred = 65536;   // bytes a tile takes where a longer one is to be had: two blocks and more per compute unit
constexpr long long kLdsMax = 163840;        // bytes a tile may take at all: the 160 KB of a gfx950 compute unit
constexpr int kSegMinRows = 32;              // the segment mapping from 32 P outputs on: its wavefronts are about half full and more
constexpr unsigned long long kStepLo = 1ull << 28, kStepHi = 1ull << 36;

typedef unsigned __int128 uwide;
typedef unsigned long long u64;

// ---- the plan ---------------------------------------------------------------------------------------------------------------
constexpr char kName[] = "vresample";

struct Plan {
	u64 step_min, step_max;
	int B, P, D, K, taps;
	RsFilter f;
};

bool step_ok(u64 step) { return step >= kStepLo && step <= kStepHi; }

// the refusal's text, or empty
std::string plan_of(u64 step_min, u64 step_max, int zeros, double rolloff, double beta, int phase_bits, int degree, Plan *out) {
	Plan p = {};
	if (!step_ok(step_min) || !step_ok(step_max)) return "vresample: a step outside [2^28, 2^36]";
	if (step_min > step_max) return "vresample: step_min above step_max";
	const std::string why = rs_filter_check(kName, zeros, rolloff, beta);
	if (!why.empty()) return why;
	if (phase_bits < 0 || phase_bits > 8) return "vresample: phase_bits must lie in 0 .. 8";
	if (degree != 0 && degree != 3 && degree != 5 && degree != 7) return "vresample: degree must be 3, 5 or 7 (0: the default pair, 3 bits and degree 5)";
	if (degree == 0 && phase_bits != 0) return "vresample: degree 0 selects the default pair and takes phase_bits 0 only";
	p.step_min = step_min; p.step_max = step_max;
	p.B = degree == 0 ? 3 : phase_bits;
	p.D = degree == 0 ? 5 : degree;
	p.P = 1 << p.B;
	p.f = rs_filter_of(zeros, rolloff, beta, 4294967296.0 / (double)step_max);
	if (!(p.K = rs_half_width(p.f, (long long)p.P * (p.D + 1)))) return rs_table_refusal(kName);
	p.taps = 2 * p.K + 1;
	*out = p;
	return std::string();
}

// The node system is the same for every segment and tap: its inverse once (Gauss-Jordan with row pivoting in long double), then every
// polynomial is a product with the prototype's values at the nodes.
void build_table(const Plan &p, double *C) {
	const double pi = 3.14159265358979323846;
	const int n = p.D + 1;
	double nu[kMaxDegree + 1];
	long double A[kMaxDegree + 1][2 * (kMaxDegree + 1)];
	for (int i = 0; i < n; ++i) {
		nu[i] = -std::cos(pi * (i + 0.5) / n);
		long double pw = 1.0L;
		for (int m = 0; m < n; ++m) {
			A[i][m] = pw;
			A[i][n + m] = i == m ? 1.0L : 0.0L;
			pw *= (long double)nu[i];
		}
	}
	for (int col = 0; col < n; ++col) {
		int piv = col;
		for (int r = col + 1; r < n; ++r)
			if (fabsl(A[r][col]) > fabsl(A[piv][col])) piv = r;
		for (int c = 0; c < 2 * n; ++c) std::swap(A[col][c], A[piv][c]);
		const long double inv = 1.0L / A[col][col];
		for (int c = 0; c < 2 * n; ++c) A[col][c] *= inv;
		for (int r = 0; r < n; ++r) {
			if (r == col) continue;
			const long double f = A[r][col];
			for (int c = 0; c < 2 * n; ++c) A[r][c] -= f * A[col][c];
		}
	}
	const double i0b = bessel_i0(p.f.beta);
	double g[kMaxDegree + 1];
	for (int seg = 0; seg < p.P; ++seg)
		for (int j = 0; j < p.taps; ++j) {
			const double k = (double)(j - p.K);
			for (int i = 0; i < n; ++i) {
				const double phi = ((double)seg + (nu[i] + 1.0) / 2.0) / (double)p.P;
				g[i] = rs_prototype(p.f, i0b, k - phi);
			}
			double *c = C + ((size_t)seg * p.taps + j) * n;
			for (int m = 0; m < n; ++m) {
				long double acc = 0.0L;
				for (int i = 0; i < n; ++i) acc += A[m][n + i] * (long double)g[i];
				c[m] = (double)acc;
			}
		}
}

// ceil(n 2^32 / step) for n >= 0, or -1 where it leaves 63 bits
long long out_length_of(u64 step, long long n) {
	const uwide v = (((uwide)n << 32) + (step - 1)) / step;
	return v > (uwide)LLONG_MAX ? -1 : (long long)v;
}

// the outputs at (q, f), (q, f) + step, ... that lie below lim x 2^32, lim = flushed ? T : max(T - K, 0); -1 where the count leaves 63 bits
long long count_of(long long q, unsigned f, u64 step, int K, long long T, bool flushed) {
	const long long lim = flushed ? T : (T > K ? T - K : 0);
	const uwide pos = ((uwide)q << 32) | f, end = (uwide)lim << 32;
	if (end <= pos) return 0;
	const uwide v = (end - pos + (step - 1)) / step;
	return v > (uwide)LLONG_MAX ? -1 : (long long)v;
}

// ---- the tiling -------------------------------------------------------------------------------------------------------------
struct Tiling : RsTiles {  // tile_out 0: no segment mapping; tiled_min: the segment mapping's segment_min
	int span_max;  // doubles of the input tile (even)
};

long long tile_span(const Plan &p, long long tile) {
	const long long span = (long long)(((uwide)tile * p.step_max) >> 32) + p.taps + 1;
	return (span + 1) / 2 * 2;
}
// the input tile, the buckets' counts, starts and first tasks, and every output's place in the sorted tile
long long tile_bytes(const Plan &p, long long tile) {
	return tile_span(p, tile) * (long long)sizeof(double) + (3 * kMaxSegments + 2) * (long long)sizeof(int) + tile * (long long)sizeof(unsigned short);
}

Tiling tiling_of(const Plan &p) {
	Tiling t = {};
	t.tiled_min = std::max((long long)kSegMinRows * p.P, (long long)kPlainBlock);
	int tile = 0;
	for (int cand = kTileMax; cand >= kTileMin && !tile; cand /= 2)
		if (tile_bytes(p, cand) <= kLdsPreferred) tile = cand;
	for (int cand = kTileMax; cand >= kTileMin && !tile; cand /= 2)
		if (tile_bytes(p, cand) <= kLdsMax) tile = cand;
	if (!tile) return t;
	t.tile_out = tile;
	t.span_max = (int)tile_span(p, tile);
	t.lds_bytes = (int)tile_bytes(p, tile);
	t.threads = 2 * (long long)t.lds_bytes > kLdsMax ? kSegThreadsWide : kSegThreads;
	return t;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------
// one signal's share of a launch: output i of the record sits at (q0, f0) + i x step
struct VrRec {
	long long x_off;  // element of x that holds the signal's sample 0
	long long y_off;  // element of y that takes the record's first output
	long long q0;     // q of the record's first output, as a sample of the signal
	u64 step;
	unsigned f0;      // and its f
	int lo, hi;       // the signal's samples [lo, hi) exist; every other one reads as +0.0
	int n_out;
	int block0;       // the record's first block in its launch
	int pad_;
};
template <class Rec> struct VrArgsOf {
	const Rec *rec;
	int n_rec;
	const void *x;
	void *y;
	int K, taps, B;
	int tile_out, span_max, out_format;
};
typedef VrArgsOf<VrRec> VrArgs;

// (i < 2^31 and the step's low word < 2^32: the product stays inside 64 bits)
__device__ __forceinline__ void vr_pos(const VrRec &r, long long i, long long *q, unsigned *f) {
	const u64 t = (u64)r.f0 + (u64)i * (r.step & 0xffffffffull);
	*f = (unsigned)t;
	*q = r.q0 + i * (long long)(r.step >> 32) + (long long)(t >> 32);
}
__device__ __forceinline__ int vr_seg(unsigned f, int B) { return B ? (int)(f >> (32 - B)) : 0; }
// nu = 2 mu - 1, mu = (f mod 2^(32-B)) 2^(B-32): the shift drops the segment's bits
__device__ __forceinline__ double vr_nu(unsigned f, int B) {
	const double mu = (double)(unsigned)(f << B) * (1.0 / 4294967296.0);
	return 2.0 * mu - 1.0;
}

// THE output of the rule: D+1 sums over the taps of one segment by ascending j from 0.0, every product rounded, then every sum, and
// Horner's scheme in nu over the sums, every step of it rounded twice.  in.at(j) is x[q - K + j] wherever the mapping keeps it.
template <int D, class In> __device__ __forceinline__ double vr_output(In in, const double *__restrict__ c, int taps, double nu) {
#pragma clang fp contract(off)
	double acc[D + 1];
#pragma unroll
	for (int m = 0; m <= D; ++m) acc[m] = 0.0;
#pragma unroll WC_VR_UNROLL
	for (int j = 0; j < taps; ++j) {
		const double x = in.at(j);
#pragma unroll
		for (int m = 0; m <= D; ++m) {
			const double prod = x * c[j * (D + 1) + m];
			acc[m] = acc[m] + prod;
		}
	}
	double y = acc[D];
#pragma unroll
	for (int m = D - 1; m >= 0; --m) {
		const double prod = y * nu;
		y = prod + acc[m];
	}
	return y;
}

struct VrTileIn {
	const double *at0;
	__device__ __forceinline__ double at(int j) const { return at0[j]; }
};
template <int FMT> struct VrGlobalIn {
	const void *x;
	long long x_off, i;
	int lo, hi;
	__device__ __forceinline__ double at(int j) const { return i + j >= lo && i + j < hi ? rs_load<FMT>(x, x_off + i + j) : 0.0; }
};

// the local memory of a tile's block (tile_bytes)
struct VrLds {
	double *tile;           // span_max inputs
	int *cnt;               // outputs per segment, then the buckets' fill
	int *start;             // P + 1: a bucket's first place in the sorted tile
	int *tstart;            // P + 1: and its first task
	unsigned short *order;  // the sorted tile: every place's output
};
__device__ __forceinline__ VrLds vr_lds_of(double *base, int span_max) {
	VrLds l;
	l.tile = base;
	l.cnt = reinterpret_cast<int *>(base + span_max);
	l.start = l.cnt + kMaxSegments;
	l.tstart = l.start + kMaxSegments + 1;
	l.order = reinterpret_cast<unsigned short *>(l.tstart + kMaxSegments + 1);
	return l;
}

// The counting sort of a tile's outputs by segment, in three steps with a barrier of the caller's behind each.  The count: cnt[s]
// outputs fall into segment s.  The starts (one thread): a bucket's first place and first task out of the counts, which are zero
// again afterwards.
__device__ __forceinline__ void vr_sort_starts(const VrLds &l, int P) {
	if (threadIdx.x == 0) {
		int at = 0, task = 0;
		for (int s = 0; s < P; ++s) {
			const int n = l.cnt[s];
			l.start[s] = at; l.tstart[s] = task;
			at += n;
			task += (n + kWave - 1) / kWave;
			l.cnt[s] = 0;
		}
		l.start[P] = at; l.tstart[P] = task;
	}
}
// The places: every output that was counted takes the next place of its bucket.  seg_of(k) is output k's segment; where not ALL
// outputs were counted, a negative one leaves k out.
template <bool ALL, class SegOf> __device__ __forceinline__ void vr_sort_place(const VrLds &l, int n_here, SegOf seg_of) {
	for (int k = threadIdx.x; k < n_here; k += blockDim.x) {
		const int s = seg_of(k);
		if (ALL || s >= 0) l.order[l.start[s] + atomicAdd(&l.cnt[s], 1)] = (unsigned short)k;
	}
}
// all three for a tile whose n_here outputs all take part, on counts that are zero and visible to the block
template <class SegOf> __device__ __forceinline__ void vr_sort_tile(const VrLds &l, int P, int n_here, SegOf seg_of) {
	for (int k = threadIdx.x; k < n_here; k += blockDim.x) atomicAdd(&l.cnt[seg_of(k)], 1);
	__syncthreads();
	vr_sort_starts(l, P);
	__syncthreads();
	vr_sort_place<true>(l, n_here, seg_of);
	__syncthreads();
}

// The sorted tile's tasks: a wavefront takes 64 places of ONE bucket at a time.  body(seg, k, live): seg is wave-uniform, k the
// output at the lane's place -- at lane 0's place, which lies inside the bucket, where the lane has none (live false).
template <class Body> __device__ __forceinline__ void vr_tasks(const VrLds &l, int P, Body body) {
	const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave), lane = threadIdx.x % kWave;
	const int n_tasks = l.tstart[P];
	int seg = 0;
	for (int task = wave; task < n_tasks; task += blockDim.x / kWave) {
		while (l.tstart[seg + 1] <= task) ++seg;
		seg = __builtin_amdgcn_readfirstlane(seg);
		const int first = __builtin_amdgcn_readfirstlane(l.start[seg] + (task - l.tstart[seg]) * kWave);
		const int end = __builtin_amdgcn_readfirstlane(l.start[seg + 1]);
		const bool live = first + lane < end;
		body(seg, (int)l.order[live ? first + lane : first], live);
	}
}

// (C apart from the other arguments and __restrict__: the coefficients of a wavefront's segment then come by scalar loads)
template <int FMT, int D> __global__ __launch_bounds__(kSegThreadsWide) void vresample_segment_kernel(VrArgs a, const double *__restrict__ C) {
	extern __shared__ double vr_lds[];
	const VrLds l = vr_lds_of(vr_lds, a.span_max);
	const int P = 1 << a.B;
	const VrRec r = a.rec[rs_find(a.rec, a.n_rec, (int)blockIdx.x)];
	const long long i_base = ((long long)blockIdx.x - r.block0) * a.tile_out;  // the tile's first output, counted from the record's first
	const int n_here = (int)min((long long)a.tile_out, (long long)r.n_out - i_base);
	long long q_first, q_last;
	unsigned f;
	vr_pos(r, i_base, &q_first, &f);
	vr_pos(r, i_base + n_here - 1, &q_last, &f);
	const int span = min((int)(q_last - q_first) + a.taps, a.span_max);  // (the host sized span_max for step_max: never less)
	for (int idx = threadIdx.x; idx < span; idx += blockDim.x) {
		const long long g = q_first - a.K + idx;
		l.tile[idx] = g >= r.lo && g < r.hi ? rs_load<FMT>(a.x, r.x_off + g) : 0.0;
	}
	for (int s = threadIdx.x; s < P; s += blockDim.x) l.cnt[s] = 0;
	__syncthreads();
	vr_sort_tile(l, P, n_here, [&](int k) {
		long long q;
		unsigned fk;
		vr_pos(r, i_base + k, &q, &fk);
		return vr_seg(fk, a.B);
	});
	vr_tasks(l, P, [&](int seg, int k, bool live) {
		long long q;
		unsigned fk;
		vr_pos(r, i_base + k, &q, &fk);
		VrTileIn in;
		in.at0 = l.tile + (int)(q - q_first);  // x[q - K]
		const double v = vr_output<D>(in, C + (size_t)seg * a.taps * (D + 1), a.taps, vr_nu(fk, a.B));
		if (live) rs_store(a.y, a.out_format, r.y_off + i_base + k, v);
	});
}

// ---- warping (include/world_class_warp.h): the same outputs at positions read from device memory --------------------------------------
// A tile of the segment mapping does not know its input span in advance: the pass that counts its outputs by segment reduces the
// lowest and highest q of its live outputs as well.  A near tile (the span fits span_max) then goes as vresample_segment_kernel's;
// a far tile keeps the sort and reads x from global memory with bounds.  An output that is not live has every tap outside the
// signal: it is +0.0 by the rule, takes no part in the sort, and no address is formed for it.  The positions are read three times,
// by the counting pass, the placing pass and the tasks: in local memory they would take 8 bytes per output and halve the tile
// (what the re-reads cost: DESIGN.md section 10, "Warping").  With the map as the source each of the three is the map rule
// evaluated again -- three divisions that do not show beside the taps, on entries that stay in the caches (section 10, "Warp
// streams").

// THE map rule (world_class_warp.h), on the host and on the device: every operation in double and rounded apart.  entry(i) is map
// entry i, 0 <= i < L, from one of the sources below; i and n are 64-bit, since a stream counts both from its reset.
constexpr long long kNoPosition = LLONG_MIN;
template <class Entry> __host__ __device__ inline long long wm_position(Entry entry, long long L, double out_per_entry, double in_per_unit, long long n) {
#pragma clang fp contract(off)
	const double t = (double)n / out_per_entry;
	double v;
	if (t >= (double)(L - 1)) {
		v = entry(L - 1);
	} else {
		const double fl = floor(t);
		const long long i = (long long)fl;
		const double w = t - fl;
		if (w == 0.0) {
			v = entry(i);
		} else {
			const double d = entry(i + 1) - entry(i);
			const double wd = w * d;
			v = entry(i) + wd;
		}
	}
	const double p = v * in_per_unit;
	if (!(p >= -1073741824.0 && p < 1073741824.0)) return kNoPosition;  // (a NaN and the infinities fail the comparisons)
	return (long long)floor(p * 4294967296.0);
}
// The sources of an entry.  An array: the whole map.  A stream's push: the entry the stream carries -- the last one an earlier push
// consumed, entry first - 1, which is all a push reads below its own -- in front of the push's new entries, fresh[0] being entry
// `first`.  A stream's flush: the same with the tail's remaining entries as the new ones.  (A whole map is the second with first 0.)
struct WmArray {
	const double *map;
	__host__ __device__ double operator()(long long i) const { return map[i]; }
};
struct WmCarried {
	const double *carried, *fresh;
	long long first;
	__host__ __device__ double operator()(long long i) const { return i < first ? *carried : fresh[i - first]; }
};

struct WpArgs : VrArgs {
	const long long *pos;  // packed like y
	__device__ __forceinline__ long long position(const VrRec &r, long long i) const { return pos[r.y_off + i]; }
	__device__ __forceinline__ bool keeps(int, int) const { return false; }
};

// The map source.  A record is one utterance of wc_warp_along_map_device or one stream's share of a push or flush: output i of the
// record is output n0 + i of a map of L entries.
struct WmRec : VrRec {
	long long map_off;  // element of the entries that holds entry `first`
	long long first;    // the record's first new entry; an entry below it is the carried one
	long long L;
	long long n0;
	double out_per_entry, in_per_unit;
	int carry;          // where the carried entry stands
	int pad2_;
};
// an entry that a push carries on: the last one it consumed, to the stream's other place
struct WsKeep {
	long long from;  // element of the entries
	int to, pad_;
};
struct WsArgs : VrArgsOf<WmRec> {
	const double *map;  // the new entries
	double *carry;      // the streams' carried entries: a pair each, of which a push reads one and writes the other
	const WsKeep *keep;
	int n_keep, keep_block0;  // the plain launch's blocks from keep_block0 on keep the n_keep entries and form no output
	__device__ __forceinline__ long long position(const WmRec &r, long long i) const {
		const WmCarried entry = {carry + r.carry, map + r.map_off, r.first};
		return wm_position(entry, r.L, r.out_per_entry, r.in_per_unit, r.n0 + i);
	}
	__device__ __forceinline__ bool keeps(int block, int thread) const {
		if (block < keep_block0) return false;
		const int k = (block - keep_block0) * kPlainBlock + thread;
		if (k < n_keep) carry[keep[k].to] = map[keep[k].from];
		return true;
	}
};

// output i of a record: (q, f) of its position and whether it is live (one tap at least inside the signal)
template <class Args, class Rec> __device__ __forceinline__ bool wp_pos(const Args &a, const Rec &r, long long i, long long *q, unsigned *f) {
	const long long pos = a.position(r, i);
	*q = pos >> 32;
	*f = (unsigned)pos;
	return *q >= (long long)r.lo - a.K && *q <= (long long)r.hi - 1 + a.K;
}

// x of an output at q, read from global memory with the signal's bounds
template <int FMT, class Args> __device__ __forceinline__ VrGlobalIn<FMT> wp_global_in(const Args &a, const VrRec &r, long long q) {
	VrGlobalIn<FMT> in;
	in.x = a.x; in.x_off = r.x_off;
	in.i = q - a.K;
	in.lo = r.lo; in.hi = r.hi;
	return in;
}

template <int FMT, int D, class Args> __global__ __launch_bounds__(kSegThreadsWide) void warp_segment_kernel(Args a, const double *__restrict__ C) {
	extern __shared__ double vr_lds[];
	const VrLds l = vr_lds_of(vr_lds, a.span_max);
	const int P = 1 << a.B;
	const auto r = a.rec[rs_find(a.rec, a.n_rec, (int)blockIdx.x)];
	const long long i_base = ((long long)blockIdx.x - r.block0) * a.tile_out;
	const int n_here = (int)min((long long)a.tile_out, (long long)r.n_out - i_base);
	const int wave = (int)threadIdx.x / kWave, lane = threadIdx.x % kWave, n_waves = blockDim.x / kWave;
	for (int s = threadIdx.x; s < P; s += blockDim.x) l.cnt[s] = 0;
	__syncthreads();
	// one pass over the positions counts the live outputs by segment, writes the others' +0.0 and finds the live ones' lowest and
	// highest q: per lane, per wavefront, then one exchange where the sorted tile will stand
	long long q_min = LLONG_MAX, q_max = LLONG_MIN;
	for (int k = threadIdx.x; k < n_here; k += blockDim.x) {
		long long q;
		unsigned f;
		if (wp_pos(a, r, i_base + k, &q, &f)) {
			q_min = min(q_min, q);
			q_max = max(q_max, q);
			atomicAdd(&l.cnt[vr_seg(f, a.B)], 1);
		} else {
			rs_store(a.y, a.out_format, r.y_off + i_base + k, 0.0);
		}
	}
	for (int d = kWave / 2; d > 0; d >>= 1) {
		q_min = min(q_min, __shfl_xor(q_min, d));
		q_max = max(q_max, __shfl_xor(q_max, d));
	}
	long long *ends = reinterpret_cast<long long *>(l.order);  // (8-byte aligned: span_max is even; 2 x 16 of them in 256 places and more)
	if (lane == 0) {
		ends[2 * wave] = q_min;
		ends[2 * wave + 1] = q_max;
	}
	__syncthreads();
	for (int w = 0; w < n_waves; ++w) {
		q_min = min(q_min, ends[2 * w]);
		q_max = max(q_max, ends[2 * w + 1]);
	}
	if (q_min > q_max) return;  // no live output (the whole block leaves)
	vr_sort_starts(l, P);
	const bool near = __builtin_amdgcn_readfirstlane((int)(q_max - q_min + a.taps <= (long long)a.span_max)) != 0;
	const int span = near ? (int)(q_max - q_min) + a.taps : 0;
	for (int idx = threadIdx.x; idx < span; idx += blockDim.x) {
		const long long g = q_min - a.K + idx;
		l.tile[idx] = g >= r.lo && g < r.hi ? rs_load<FMT>(a.x, r.x_off + g) : 0.0;
	}
	__syncthreads();  // (every thread has read the ends)
	vr_sort_place<false>(l, n_here, [&](int k) {
		long long q;
		unsigned f;
		return wp_pos(a, r, i_base + k, &q, &f) ? vr_seg(f, a.B) : -1;
	});
	__syncthreads();
	// (only live outputs stand in the sorted tile)  in_at(q): where the tile keeps x[q - K] and the taps behind it
	const auto run = [&](auto in_at) {
		vr_tasks(l, P, [&](int seg, int k, bool live) {
			long long q;
			unsigned f;
			wp_pos(a, r, i_base + k, &q, &f);
			const double v = vr_output<D>(in_at(q), C + (size_t)seg * a.taps * (D + 1), a.taps, vr_nu(f, a.B));
			if (live) rs_store(a.y, a.out_format, r.y_off + i_base + k, v);
		});
	};
	if (near) {
		run([&](long long q) {
			VrTileIn in;
			in.at0 = l.tile + (int)(q - q_min);
			return in;
		});
	} else {
		run([&](long long q) { return wp_global_in<FMT>(a, r, q); });
	}
}

template <int FMT, int D, class Args> __global__ __launch_bounds__(kPlainBlock) void warp_plain_kernel(Args a, const double *__restrict__ C) {
	if (a.keeps((int)blockIdx.x, (int)threadIdx.x)) return;
	const auto r = a.rec[rs_find(a.rec, a.n_rec, (int)blockIdx.x)];
	const long long i = ((long long)blockIdx.x - r.block0) * kPlainBlock + threadIdx.x;
	if (i >= r.n_out) return;
	long long q;
	unsigned f;
	if (!wp_pos(a, r, i, &q, &f)) {
		rs_store(a.y, a.out_format, r.y_off + i, 0.0);
		return;
	}
	rs_store(a.y, a.out_format, r.y_off + i, vr_output<D>(wp_global_in<FMT>(a, r, q), C + (size_t)vr_seg(f, a.B) * a.taps * (D + 1), a.taps, vr_nu(f, a.B)));
}

// a record's x_off, hi and y_off are its map's first entry, its length and its first position; a record of the tiled group counts
// its blocks in tiles of `sub` blocks of the plain size (rs_sort_records), and every thread still takes one output
struct WmArgs {
	const VrRec *rec;
	int n_rec;
	const double *map;
	long long *pos;
	double out_per_entry, in_per_unit;
	int sub;
};
__global__ __launch_bounds__(kPlainBlock) void warp_map_kernel(WmArgs a) {
	const int b = (int)blockIdx.x / a.sub;
	const VrRec r = a.rec[rs_find(a.rec, a.n_rec, b)];
	const long long i = (((long long)b - r.block0) * a.sub + (int)blockIdx.x % a.sub) * kPlainBlock + threadIdx.x;
	if (i >= r.n_out) return;
	const WmArray entry = {a.map + r.x_off};
	a.pos[r.y_off + i] = wm_position(entry, r.hi, a.out_per_entry, a.in_per_unit, i);
}

template <int FMT, int D> __global__ __launch_bounds__(kPlainBlock) void vresample_plain_kernel(VrArgs a, const double *__restrict__ C) {
	const VrRec r = a.rec[rs_find(a.rec, a.n_rec, (int)blockIdx.x)];
	const long long i = ((long long)blockIdx.x - r.block0) * kPlainBlock + threadIdx.x;
	if (i >= r.n_out) return;
	long long q;
	unsigned f;
	vr_pos(r, i, &q, &f);
	VrGlobalIn<FMT> in;
	in.x = a.x; in.x_off = r.x_off;
	in.i = q - a.K;
	in.lo = r.lo; in.hi = r.hi;
	rs_store(a.y, a.out_format, r.y_off + i, vr_output<D>(in, C + (size_t)vr_seg(f, a.B) * a.taps * (D + 1), a.taps, vr_nu(f, a.B)));
}

// f(format, degree) with both as compile-time constants
template <class F> void with_variant(int fmt, int D, F &&f) {
	rs_with_format(fmt, [&](auto format) {
		if (D == 3) f(format, RsConst<3>());
		else if (D == 5) f(format, RsConst<5>());
		else f(format, RsConst<7>());
	});
}

// ---- the handles (wc_resample_plan.hpp) around them ------------------------------------------------------------------------------
typedef RsCore<Plan, Tiling> Core;

// the table built and uploaded for a checked plan; nullptr + error on failure
Core *core_create(const Plan &p) {
	const Tiling t = tiling_of(p);
	const void *segment_kernels[9];  // the converter's and the warp's two
	for (int fmt = 0; fmt < 3; ++fmt)
		with_variant(fmt, p.D, [&](auto format, auto degree) {
			segment_kernels[fmt] = (const void *)vresample_segment_kernel<decltype(format)::value, decltype(degree)::value>;
			segment_kernels[3 + fmt] = (const void *)warp_segment_kernel<decltype(format)::value, decltype(degree)::value, WpArgs>;
			segment_kernels[6 + fmt] = (const void *)warp_segment_kernel<decltype(format)::value, decltype(degree)::value, WsArgs>;
		});
	return rs_core_create<Core>(kName, "the tile", p, t, t.tile_out > 0 && !WC_VR_FORCE_PLAIN, (size_t)p.P * p.taps * (p.D + 1),
								[&](double *C) { build_table(p, C); }, segment_kernels);
}

// the records of a launch are on the device: those of the segment mapping, then those of the plain mapping
int vr_enqueue(const Core &c, hipStream_t hs, const VrRec *d_rec, const RsSorted &s, const void *x, int in_format, void *y, int out_format) {
	VrArgs a = {};
	a.x = x; a.y = y;
	a.K = c.p.K; a.taps = c.p.taps; a.B = c.p.B;
	a.tile_out = c.t.tile_out; a.span_max = c.t.span_max; a.out_format = out_format;
	return rs_timed(c, "vresample_kernels", hs, [&] {
		with_variant(in_format, c.p.D, [&](auto format, auto degree) {
			constexpr int FMT = decltype(format)::value, D = decltype(degree)::value;
			rs_launch_pair(c, hs, a, d_rec, s, vresample_segment_kernel<FMT, D>, vresample_plain_kernel<FMT, D>);
		});
	});
}

// the warp's launch: the same records (their position fields unused) and the positions, packed like y
int wp_enqueue(const Core &c, hipStream_t hs, const VrRec *d_rec, const RsSorted &s, const void *x, int in_format, const long long *pos, void *y,
			   int out_format) {
	WpArgs a = {};
	a.x = x; a.y = y; a.pos = pos;
	a.K = c.p.K; a.taps = c.p.taps; a.B = c.p.B;
	a.tile_out = c.t.tile_out; a.span_max = c.t.span_max; a.out_format = out_format;
	return rs_timed(c, "warp_kernels", hs, [&] {
		with_variant(in_format, c.p.D, [&](auto format, auto degree) {
			constexpr int FMT = decltype(format)::value, D = decltype(degree)::value;
			rs_launch_pair(c, hs, a, d_rec, s, warp_segment_kernel<FMT, D, WpArgs>, warp_plain_kernel<FMT, D, WpArgs>);
		});
	});
}

// the same launch with the map rule as the source of the positions: entries at `map`, carried entries at `carry`; n_keep entries
// are carried on by blocks behind the plain group's own (a launch of those blocks alone where the group is empty)
int ws_enqueue(const Core &c, hipStream_t hs, const WmRec *d_rec, RsSorted s, const void *x, int in_format, const double *map, double *carry,
			   const WsKeep *keep, int n_keep, void *y, int out_format) {
	WsArgs a = {};
	a.x = x; a.y = y; a.map = map; a.carry = carry;
	a.keep = keep; a.n_keep = n_keep; a.keep_block0 = s.blocks_plain;
	a.K = c.p.K; a.taps = c.p.taps; a.B = c.p.B;
	a.tile_out = c.t.tile_out; a.span_max = c.t.span_max; a.out_format = out_format;
	s.blocks_plain += (n_keep + kPlainBlock - 1) / kPlainBlock;
	return rs_timed(c, "warp_map_kernels", hs, [&] {
		with_variant(in_format, c.p.D, [&](auto format, auto degree) {
			constexpr int FMT = decltype(format)::value, D = decltype(degree)::value;
			rs_launch_pair(c, hs, a, d_rec, s, warp_segment_kernel<FMT, D, WsArgs>, warp_plain_kernel<FMT, D, WsArgs>);
		});
	});
}

// the map kernel over both groups of records: one thread per output in blocks of the plain size
int wm_enqueue(const Core &c, hipStream_t hs, const VrRec *d_rec, const RsSorted &s, const double *map, double out_per_entry, double in_per_unit,
			   long long *pos) {
	WmArgs a = {};
	a.map = map; a.pos = pos;
	a.out_per_entry = out_per_entry; a.in_per_unit = in_per_unit;
	return rs_timed(c, "warp_map_kernel", hs, [&] {
		if (s.blocks_tiled > 0) {
			a.rec = d_rec; a.n_rec = s.n_tiled; a.sub = c.t.tile_out / kPlainBlock;
			hipLaunchKernelGGL(warp_map_kernel, dim3((unsigned)s.blocks_tiled * (unsigned)a.sub), dim3(kPlainBlock), 0, hs, a);
		}
		if (s.blocks_plain > 0) {
			a.rec = d_rec + s.n_tiled; a.n_rec = s.n_plain; a.sub = 1;
			hipLaunchKernelGGL(warp_map_kernel, dim3((unsigned)s.blocks_plain), dim3(kPlainBlock), 0, hs, a);
		}
	});
}

bool wm_scale_ok(double v) { return std::isfinite(v) && v > 0.0; }

// a stream's state: the rational streams' and the position (q, f) of its next output with its step
struct State : RsStreamState {
	long long q = 0;
	unsigned f = 0;
	u64 step = 0;
	void rewind() {  // (the step stays)
		RsStreamState::rewind();
		q = 0; f = 0;
	}
};

// ---- warp streams (world_class_warp_stream.h): the host's arithmetic on counts ------------------------------------------------------
// c(E): the n >= 0 with (double)n / out_per_entry <= (double)(E - 1), found from the product and corrected with the predicate;
// -1 where the count leaves 62 bits
long long ws_committed(long long entries, double out_per_entry) {
	if (entries < 1) return 0;
	const double last = (double)(entries - 1);
	const double guess = std::floor(last * out_per_entry);
	if (!(guess < 4611686018427387904.0)) return -1;
	const auto in = [&](long long n) { return (double)n / out_per_entry <= last; };
	long long n = (long long)guess;  // (n = 0 is always in)
	while (in(n + 1)) ++n;
	while (n > 0 && !in(n)) --n;
	return n + 1;
}

// what `entries` more entries can commit at most at out_per_entry: c moves by floor(a + b) - floor(a) <= ceil(b), and by one more
// at either end where a quotient rounds across the predicate; -1 where it leaves 31 bits
long long ws_max_out(int entries, double out_per_entry) {
	if (entries < 1) return 0;
	const double v = std::ceil((double)entries * out_per_entry) + 2.0;
	return v <= (double)INT_MAX ? (long long)v : -1;
}

struct WsState {
	int track = -1;  // -1: not attached
	int delay = 0;
	int parity = 0;  // where of its pair the carried entry stands
	bool ended = false;
	double out_per_entry = 0.0, in_per_unit = 0.0;
	long long rows = 0, entries = 0, committed = 0;
};

constexpr char kWsName[] = "warp stream";
int ws_bytes_of(int format) { return format == 0 ? 8 : format == 1 ? 2 : 4; }

}  // namespace

struct wc_vresampler : RsBatch<Core> {};
struct wc_vresample_stream : RsStreams<Core, State> {};
struct wc_warp_stream {
	Core *c = nullptr;
	int n_streams = 0, n_tracks = 0, max_track = 0, track_format = 0, max_entries = 0, max_delay = 0;
	int max_out_push = 0, max_out_flush = 0;
	double max_out_per_entry = 0.0;
	std::vector<WsState> st;
	std::vector<int> track_len;  // 0: the slot has not been set
	DevBuf tracks;               // n_tracks x max_track samples of track_format
	DevBuf carry;                // n_streams x 2 doubles
	RecPair rec;                 // a record per stream with outputs, then a WsKeep per stream with entries
};

namespace {

// The whole of a push (flush false: counts are n_rows, entries are d_settled's) and of a flush (counts are want, entries are the
// tail's).  Everything is planned from the counts before the first enqueue; the plan becomes the state behind the last one.
int ws_push(wc_warp_stream *h, bool flush, const int *counts, const double *d_entries, void *d_y, int out_format, int *samples_out) {
	const char *what = flush ? " flush" : " push";
	const auto refuse = [&](const char *why) { return rs_refuse(kWsName, (std::string(what) + why).c_str()); };
	if (!h || !counts || !samples_out) return refuse(": null argument");
	if (out_format != 0 && out_format != 1) return refuse(": out_format is 0 or 1");
	const Core &c = *h->c;
	DeviceLock lock(c.dev);
	const int n = h->n_streams, max_out = flush ? h->max_out_flush : h->max_out_push;
	struct Share {
		int slice, consumed;    // doubles of the stream in d_entries; entries consumed, the last ones of the slice
		long long after, outs;  // c(E_after); outputs
	};
	std::vector<Share> share((size_t)n);
	long long total_read = 0, total_out = 0;
	for (int u = 0; u < n; ++u) {
		const WsState &s = h->st[u];
		Share &p = share[u];
		p = Share();
		p.after = s.committed;
		if (flush) {
			if (!counts[u]) continue;
			if (s.track < 0 || s.ended) return refuse(": a wanted stream is not attached or has ended");
			if (s.delay == 0 || s.rows == 0) return refuse(": a wanted stream has delay 0 or no rows (nothing waits)");
			p.slice = (int)std::min<long long>((long long)s.delay + 1, s.rows);
			p.consumed = (int)std::min<long long>(s.delay, s.rows);
		} else {
			if (counts[u] < 0 || counts[u] > h->max_entries) return refuse(": a count outside 0 .. max_entries_per_push");
			if (counts[u] > 0 && (s.track < 0 || s.ended)) return refuse(": rows for a stream that is not attached or has ended (reset it first)");
			p.slice = counts[u];
			p.consumed = (int)(std::max<long long>(s.rows + counts[u] - s.delay, 0) - std::max<long long>(s.rows - s.delay, 0));
		}
		if (p.consumed > 0) {
			p.after = ws_committed(s.entries + p.consumed, s.out_per_entry);
			if (p.after < 0 || p.after - s.committed > max_out) return refuse(": the output count leaves the handle's bound");
		}
		p.outs = p.after - s.committed;
		total_read += p.consumed;
		total_out += p.outs;
	}
	if ((total_read > 0 && !d_entries) || (total_out > 0 && !d_y)) return refuse(": null array");
	// ---- no refusal is left: the records ----
	WmRec *rec = h->rec.begin<WmRec>();
	if (!rec) return WC_ERR_DEVICE;
	std::vector<WmRec> recs;
	std::vector<WsKeep> keeps;
	long long e_off = 0, y_off = 0;
	for (int u = 0; u < n; ++u) {
		const WsState &s = h->st[u];
		const Share &p = share[u];
		samples_out[u] = (int)p.outs;
		if (p.outs > 0) {
			WmRec q = WmRec();
			q.x_off = (long long)s.track * h->max_track; q.y_off = y_off;
			q.lo = 0; q.hi = h->track_len[s.track];
			q.n_out = (int)p.outs;
			q.map_off = e_off + (p.slice - p.consumed);
			q.first = s.entries; q.L = s.entries + p.consumed;
			q.n0 = s.committed;
			q.out_per_entry = s.out_per_entry; q.in_per_unit = s.in_per_unit;
			q.carry = 2 * u + s.parity;
			recs.push_back(q);
		}
		if (p.consumed > 0 && !flush) {
			WsKeep k = {e_off + p.slice - 1, 2 * u + (1 - s.parity), 0};
			keeps.push_back(k);
		}
		e_off += p.slice;
		y_off += p.outs;
	}
	if (!recs.empty() || !keeps.empty()) {
		WC_HIP(hipSetDevice(c.dev->id));
		hipStream_t hs = c.dev->active();
		const RsSorted so = rs_sort_records(c, recs, rec);
		WsKeep *keep = reinterpret_cast<WsKeep *>(rec + recs.size());
		std::copy(keeps.begin(), keeps.end(), keep);
		const size_t bytes = sizeof(WmRec) * recs.size() + sizeof(WsKeep) * keeps.size();
		const WmRec *d_rec;
		int rc;
		if ((rc = h->rec.upload(hs, bytes, &d_rec))) return rc;
		if ((rc = ws_enqueue(c, hs, d_rec, so, h->tracks.p, h->track_format, d_entries, h->carry.as<double>(),
							 reinterpret_cast<const WsKeep *>(d_rec + recs.size()), (int)keeps.size(), d_y, out_format)))
			return rc;
	}
	for (int u = 0; u < n; ++u) {
		WsState &s = h->st[u];
		const Share &p = share[u];
		if (flush) {
			if (!counts[u]) continue;
			s.ended = true;
		} else {
			s.rows += counts[u];
			if (p.consumed > 0) s.parity = 1 - s.parity;
		}
		s.entries += p.consumed;
		s.committed = p.after;
	}
	return WC_OK;
}

bool ws_stream_ok(const wc_warp_stream *h, int stream) { return h && stream >= 0 && stream < h->n_streams; }

}  // namespace

extern "C" {

int wc_vresample_plan(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, double beta, int phase_bits,
					  int degree, int *half_width, int *segments, int *degree_out, double *cutoff) {
	Plan p;
	const std::string why = plan_of(step_min, step_max, zeros, rolloff, beta, phase_bits, degree, &p);
	if (!why.empty()) return fail(WC_ERR_INVALID, why);
	if (half_width) *half_width = p.K;
	if (segments) *segments = p.P;
	if (degree_out) *degree_out = p.D;
	if (cutoff) *cutoff = p.f.s;
	return WC_OK;
}

int wc_vresample_filter(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, double beta, int phase_bits,
						int degree, double *table, long long capacity) {
	Plan p;
	const std::string why = plan_of(step_min, step_max, zeros, rolloff, beta, phase_bits, degree, &p);
	if (!why.empty()) return fail(WC_ERR_INVALID, why);
	if (!table || capacity < (long long)p.P * p.taps * (p.D + 1)) return fail(WC_ERR_INVALID, "vresample filter: the array holds fewer than P x (2K+1) x (D+1) doubles");
	build_table(p, table);
	return WC_OK;
}

long long wc_vresample_out_length(unsigned long long step, long long n_in) {
	if (!step_ok(step)) return fail(WC_ERR_INVALID, "vresample: a step outside [2^28, 2^36]");
	if (n_in < 0) return fail(WC_ERR_INVALID, "vresample: a negative length");
	const long long n = out_length_of(step, n_in);
	return n < 0 ? fail(WC_ERR_INVALID, "vresample: the output length leaves 63 bits") : n;
}

long long wc_vresample_committed(long long q, unsigned int f, unsigned long long step, int half_width, long long samples_in, int flushed) {
	if (!step_ok(step)) return fail(WC_ERR_INVALID, "vresample: a step outside [2^28, 2^36]");
	if (q < 0 || half_width < 0 || samples_in < 0) return fail(WC_ERR_INVALID, "vresample: a negative position, half width or sample count");
	const long long n = count_of(q, f, step, half_width, samples_in, flushed != 0);
	return n < 0 ? fail(WC_ERR_INVALID, "vresample: the output count leaves 63 bits") : n;
}

int wc_vresample_tiling(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, int phase_bits, int degree,
						int *tile_outputs, int *segment_min, int *plain_block) {
	Plan p;
	const std::string why = plan_of(step_min, step_max, zeros, rolloff, 0.0, phase_bits, degree, &p);
	if (!why.empty()) return fail(WC_ERR_INVALID, why);
	const Tiling t = tiling_of(p);
	if (tile_outputs) *tile_outputs = t.tile_out;
	if (segment_min) *segment_min = (int)t.tiled_min;
	if (plain_block) *plain_block = kPlainBlock;
	return WC_OK;
}

// ---- batch --------------------------------------------------------------------------------------------------------------------
wc_vresampler *wc_vresampler_create(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, double beta,
									int phase_bits, int degree) {
	Plan p;
	const std::string why = plan_of(step_min, step_max, zeros, rolloff, beta, phase_bits, degree, &p);
	if (!why.empty()) { set_error(why); return nullptr; }
	return rs_batch_create<wc_vresampler>(core_create(p));
}

void wc_vresampler_destroy(wc_vresampler *r) { rs_batch_destroy(r); }

int wc_vresample_device(wc_vresampler *r, int n_utt, const void *d_x, int in_format, const int *x_length, const unsigned long long *step,
						void *d_y, int out_format) {
	return rs_batch_run<VrRec>(
		kName, r, x_length && step && d_x && d_y, n_utt, in_format, out_format, x_length,
		[&](int u, VrRec &q, long long *n_out) -> const char * {
			if (step[u] < r->c->p.step_min || step[u] > r->c->p.step_max) return ": a step outside the handle's [step_min, step_max]";
			*n_out = out_length_of(step[u], x_length[u]);
			q.step = step[u];
			return nullptr;
		},
		[&](hipStream_t hs, const VrRec *d_rec, const RsSorted &s) { return vr_enqueue(*r->c, hs, d_rec, s, d_x, in_format, d_y, out_format); });
}

// ---- streams ------------------------------------------------------------------------------------------------------------------
wc_vresample_stream *wc_vresample_stream_create(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff,
												double beta, int phase_bits, int degree, int n_streams, int max_samples_per_push) {
	if (!rs_stream_counts_ok(kName, n_streams, max_samples_per_push)) return nullptr;
	Plan p;
	const std::string why = plan_of(step_min, step_max, zeros, rolloff, beta, phase_bits, degree, &p);
	if (!why.empty()) { set_error(why); return nullptr; }
	// a push's outputs lie in [pos, lim x 2^32) with pos >= (T_before - K) 2^32 and lim <= T_after: at most ceil((max + K) 2^32 / step_min)
	const long long max_out = out_length_of(p.step_min, (long long)max_samples_per_push + p.K);
	if (max_out < 0 || max_out > (long long)INT_MAX) { set_error("vresample stream: max_out_per_push leaves 31 bits"); return nullptr; }
	wc_vresample_stream *h = rs_stream_create<wc_vresample_stream, VrRec>(core_create(p), n_streams, max_samples_per_push, (int)max_out);
	if (h)
		for (State &s : h->st) s.step = p.step_max;
	return h;
}

void wc_vresample_stream_destroy(wc_vresample_stream *h) { rs_stream_destroy(h); }

int wc_vresample_stream_max_out_per_push(const wc_vresample_stream *h) { return rs_stream_max_out(h); }

int wc_vresample_stream_reset(wc_vresample_stream *h, int stream) { return rs_stream_reset(kName, h, stream); }

int wc_vresample_stream_set_step(wc_vresample_stream *h, int stream, unsigned long long step) {
	if (!rs_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "vresample stream: bad stream index");
	if (step < h->c->p.step_min || step > h->c->p.step_max) return fail(WC_ERR_INVALID, "vresample stream: a step outside the handle's [step_min, step_max]");
	DeviceLock lock(h->c->dev);
	h->st[stream].step = step;
	return WC_OK;
}

int wc_vresample_stream_push_device(wc_vresample_stream *h, const void *d_chunk, int in_format, const int *n_new, const int *flush,
									void *d_y, int out_format, int *samples_out) {
	return rs_stream_push<VrRec>(
		kName, " stream push: the output count leaves max_out_per_push", h, d_chunk, in_format, n_new, flush, d_y, out_format, samples_out,
		// the count: the outputs from the stream's position on, at its step, that the samples reach
		[&](const State &s, long long T, bool flushed) {
			const long long count = count_of(s.q, s.f, s.step, h->c->p.K, T, flushed);
			return count > h->max_out ? -1 : count;
		},
		// the first output: the stream's position; the first uncommitted output has q >= received - K
		[&](const State &s, VrRec &q) {
			q.q0 = s.q - (s.received - 2 * h->c->p.K);
			q.f0 = s.f;
			q.step = s.step;
		},
		// the position moves on by count x step
		[](State &s, long long count) {
			const uwide pos = (((uwide)s.q << 32) | s.f) + (uwide)count * s.step;
			s.q = (long long)(pos >> 32);
			s.f = (unsigned)pos;
		},
		[&](hipStream_t hs, const VrRec *d_rec, const RsSorted &s, const void *x) { return vr_enqueue(*h->c, hs, d_rec, s, x, 0, d_y, out_format); });
}

long long wc_vresample_stream_samples_received(const wc_vresample_stream *h, int stream) { return rs_stream_received(h, stream); }

long long wc_vresample_stream_samples_committed(const wc_vresample_stream *h, int stream) { return rs_stream_committed(h, stream); }

// ---- warping (world_class_warp.h) -----------------------------------------------------------------------------------------------
int wc_warp_tiling(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, int phase_bits, int degree,
				   int *tile_outputs, int *span_max, int *segment_min, int *plain_block) {
	Plan p;
	const std::string why = plan_of(step_min, step_max, zeros, rolloff, 0.0, phase_bits, degree, &p);
	if (!why.empty()) return fail(WC_ERR_INVALID, why);
	const Tiling t = tiling_of(p);  // the converter's own: at arithmetic positions both kernels cut the same tiles
	if (tile_outputs) *tile_outputs = t.tile_out;
	if (span_max) *span_max = t.tile_out ? t.span_max : (int)tile_span(p, kTileMin);
	if (segment_min) *segment_min = (int)t.tiled_min;
	if (plain_block) *plain_block = kPlainBlock;
	return WC_OK;
}

long long wc_warp_map_out_length(int map_length, double out_per_entry) {
	if (map_length < 1) return fail(WC_ERR_INVALID, "warp map: a map holds one entry at least");
	if (!wm_scale_ok(out_per_entry)) return fail(WC_ERR_INVALID, "warp map: out_per_entry must be finite and positive");
	const double last = std::floor((double)(map_length - 1) * out_per_entry);
	if (!(last < 4611686018427387904.0)) return fail(WC_ERR_INVALID, "warp map: the output length leaves 62 bits");
	return (long long)last + 1;
}

int wc_warp_map_positions(const double *map, int map_length, double out_per_entry, double in_per_unit, long long n_out, long long *pos) {
	if (!map || !pos) return fail(WC_ERR_INVALID, "warp map: null argument");
	if (map_length < 1 || n_out < 0) return fail(WC_ERR_INVALID, "warp map: a map holds one entry at least and n_out is not negative");
	if (!wm_scale_ok(out_per_entry) || !wm_scale_ok(in_per_unit)) return fail(WC_ERR_INVALID, "warp map: out_per_entry and in_per_unit must be finite and positive");
	const WmArray entry = {map};
	for (long long n = 0; n < n_out; ++n) pos[n] = wm_position(entry, map_length, out_per_entry, in_per_unit, n);
	return WC_OK;
}

int wc_warp_device(wc_vresampler *r, int n_utt, const void *d_x, int in_format, const int *x_length, const long long *d_pos,
				   const int *out_length, void *d_y, int out_format) {
	return rs_batch_run<VrRec>(
		"warp", r, x_length && out_length && d_x && d_pos && d_y, n_utt, in_format, out_format, x_length,
		[&](int u, VrRec &, long long *n_out) -> const char * {
			if (out_length[u] < 0) return ": an output length below 0";
			*n_out = out_length[u];
			return nullptr;
		},
		[&](hipStream_t hs, const VrRec *d_rec, const RsSorted &s) { return wp_enqueue(*r->c, hs, d_rec, s, d_x, in_format, d_pos, d_y, out_format); });
}

int wc_warp_map_positions_device(wc_vresampler *r, int n_utt, const double *d_map, const int *map_length, double out_per_entry,
								 double in_per_unit, const int *out_length, long long *d_pos) {
	if (!wm_scale_ok(out_per_entry) || !wm_scale_ok(in_per_unit)) return fail(WC_ERR_INVALID, "warp map: out_per_entry and in_per_unit must be finite and positive");
	// (the records of a batch of signals: a map is the input, its length the record's hi)
	return rs_batch_run<VrRec>(
		"warp map", r, map_length && out_length && d_map && d_pos, n_utt, 0, 0, map_length,
		[&](int u, VrRec &, long long *n_out) -> const char * {
			if (out_length[u] < 0) return ": an output length below 0";
			*n_out = out_length[u];
			return nullptr;
		},
		[&](hipStream_t hs, const VrRec *d_rec, const RsSorted &s) { return wm_enqueue(*r->c, hs, d_rec, s, d_map, out_per_entry, in_per_unit, d_pos); });
}

// ---- warp streams (world_class_warp_stream.h) ---------------------------------------------------------------------------------------
long long wc_warp_stream_committed(long long entries, double out_per_entry) {
	if (entries < 0) return fail(WC_ERR_INVALID, "warp stream: a negative entry count");
	if (!wm_scale_ok(out_per_entry)) return fail(WC_ERR_INVALID, "warp stream: out_per_entry must be finite and positive");
	const long long n = ws_committed(entries, out_per_entry);
	return n < 0 ? fail(WC_ERR_INVALID, "warp stream: the output count leaves 62 bits") : n;
}

int wc_warp_along_map_device(wc_vresampler *r, int n_utt, const void *d_x, int in_format, const int *x_length, const double *d_map,
							 const int *map_length, double out_per_entry, double in_per_unit, const int *out_length, void *d_y,
							 int out_format) {
	if (!wm_scale_ok(out_per_entry) || !wm_scale_ok(in_per_unit)) return fail(WC_ERR_INVALID, "warp along map: out_per_entry and in_per_unit must be finite and positive");
	long long map_off = 0;  // (the utterances are formed in their order)
	return rs_batch_run<WmRec>(
		"warp along map", r, x_length && map_length && out_length && d_x && d_map && d_y, n_utt, in_format, out_format, x_length,
		[&](int u, WmRec &q, long long *n_out) -> const char * {
			if (map_length[u] < 1) return ": a map holds one entry at least";
			if (out_length[u] < 0) return ": an output length below 0";
			*n_out = out_length[u];
			q.map_off = map_off; q.L = map_length[u];
			q.out_per_entry = out_per_entry; q.in_per_unit = in_per_unit;
			map_off += map_length[u];
			return nullptr;
		},
		[&](hipStream_t hs, const WmRec *d_rec, const RsSorted &s) {
			return ws_enqueue(*r->c, hs, d_rec, s, d_x, in_format, d_map, nullptr, nullptr, 0, d_y, out_format);
		});
}

wc_warp_stream *wc_warp_stream_create(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, double beta,
									  int phase_bits, int degree, int n_streams, int n_tracks, int max_track_samples, int track_format,
									  int max_entries_per_push, int max_delay, double max_out_per_entry) {
	if (n_streams < 1 || n_tracks < 1 || max_track_samples < 1 || max_entries_per_push < 1) {
		set_error("warp stream: n_streams, n_tracks, max_track_samples and max_entries_per_push must be at least 1");
		return nullptr;
	}
	if (max_delay < 0) { set_error("warp stream: max_delay must not be negative"); return nullptr; }
	if (track_format < 0 || track_format > 2) { set_error("warp stream: track_format is 0, 1 or 2"); return nullptr; }
	if (!wm_scale_ok(max_out_per_entry)) { set_error("warp stream: max_out_per_entry must be finite and positive"); return nullptr; }
	Plan p;
	const std::string why = plan_of(step_min, step_max, zeros, rolloff, beta, phase_bits, degree, &p);
	if (!why.empty()) { set_error(why); return nullptr; }
	const long long out_push = ws_max_out(max_entries_per_push, max_out_per_entry), out_flush = ws_max_out(max_delay, max_out_per_entry);
	if (out_push < 0 || out_flush < 0 || std::max(out_push, out_flush) * n_streams > (long long)INT_MAX) {
		set_error("warp stream: max_out_per_push or the packed output leaves 31 bits");
		return nullptr;
	}
	Core *c = core_create(p);
	if (!c) return nullptr;
	DeviceLock lock(c->dev);
	wc_warp_stream *h = new wc_warp_stream();
	h->c = c;
	h->n_streams = n_streams; h->n_tracks = n_tracks; h->max_track = max_track_samples; h->track_format = track_format;
	h->max_entries = max_entries_per_push; h->max_delay = max_delay; h->max_out_per_entry = max_out_per_entry;
	h->max_out_push = (int)out_push; h->max_out_flush = (int)out_flush;
	h->st.resize((size_t)n_streams);
	h->track_len.assign((size_t)n_tracks, 0);
	const size_t rec = (sizeof(WmRec) + sizeof(WsKeep)) * (size_t)n_streams;
	if (h->tracks.reserve((size_t)ws_bytes_of(track_format) * (size_t)n_tracks * (size_t)max_track_samples) ||
		h->carry.reserve(sizeof(double) * 2 * (size_t)n_streams) || h->rec.reserve(rec)) {
		wc_warp_stream_destroy(h);
		return nullptr;
	}
	return h;
}

void wc_warp_stream_destroy(wc_warp_stream *h) {
	if (!h) return;
	h->c->dev->quiesce();
	h->tracks.release(); h->carry.release(); h->rec.release();
	rs_core_destroy(h->c);
	delete h;
}

int wc_warp_stream_set_track_device(wc_warp_stream *h, int track, int n_samples, const void *d_x) {
	if (!h || !d_x) return rs_refuse(kWsName, " set_track: null argument");
	if (track < 0 || track >= h->n_tracks) return rs_refuse(kWsName, " set_track: bad track index");
	if (n_samples < 1 || n_samples > h->max_track) return rs_refuse(kWsName, " set_track: n_samples outside 1 .. max_track_samples");
	DeviceLock lock(h->c->dev);
	for (const WsState &s : h->st)
		if (s.track == track && s.rows > 0) return rs_refuse(kWsName, " set_track: a stream that has received rows is attached to the slot");
	const size_t each = (size_t)ws_bytes_of(h->track_format);
	WC_HIP(hipSetDevice(h->c->dev->id));
	WC_HIP(hipMemcpyAsync(static_cast<char *>(h->tracks.p) + each * (size_t)track * (size_t)h->max_track, d_x, each * (size_t)n_samples,
						  hipMemcpyDeviceToDevice, h->c->dev->active()));
	h->track_len[track] = n_samples;
	return WC_OK;
}

int wc_warp_stream_reset(wc_warp_stream *h, int stream, int track, int delay, double out_per_entry, double in_per_unit) {
	if (!ws_stream_ok(h, stream)) return rs_refuse(kWsName, " reset: bad stream index");
	if (track < 0 || track >= h->n_tracks) return rs_refuse(kWsName, " reset: bad track index");
	if (delay < 0 || delay > h->max_delay) return rs_refuse(kWsName, " reset: a delay outside 0 .. max_delay");
	if (!wm_scale_ok(out_per_entry) || out_per_entry > h->max_out_per_entry) return rs_refuse(kWsName, " reset: out_per_entry must be finite, positive and at most max_out_per_entry");
	if (!wm_scale_ok(in_per_unit)) return rs_refuse(kWsName, " reset: in_per_unit must be finite and positive");
	DeviceLock lock(h->c->dev);
	if (h->track_len[track] == 0) return rs_refuse(kWsName, " reset: the slot has not been set");
	WsState &s = h->st[stream];
	const int parity = s.parity;  // (the carried entry is not cleared: no output reads one before an entry has been consumed)
	s = WsState();
	s.parity = parity;
	s.track = track; s.delay = delay;
	s.out_per_entry = out_per_entry; s.in_per_unit = in_per_unit;
	return WC_OK;
}

int wc_warp_stream_max_out_per_push(const wc_warp_stream *h) { return h ? h->max_out_push : WC_ERR_INVALID; }
int wc_warp_stream_max_out_per_flush(const wc_warp_stream *h) { return h ? h->max_out_flush : WC_ERR_INVALID; }

int wc_warp_stream_push_device(wc_warp_stream *h, const int *n_rows, const double *d_map, void *d_y, int out_format, int *samples_out) {
	return ws_push(h, false, n_rows, d_map, d_y, out_format, samples_out);
}

int wc_warp_stream_flush_device(wc_warp_stream *h, const int *want, const double *d_tail, void *d_y, int out_format, int *samples_out) {
	return ws_push(h, true, want, d_tail, d_y, out_format, samples_out);
}

long long wc_warp_stream_rows_received(const wc_warp_stream *h, int stream) { return ws_stream_ok(h, stream) ? h->st[stream].rows : -1; }
long long wc_warp_stream_entries_consumed(const wc_warp_stream *h, int stream) { return ws_stream_ok(h, stream) ? h->st[stream].entries : -1; }
long long wc_warp_stream_samples_committed(const wc_warp_stream *h, int stream) { return ws_stream_ok(h, stream) ? h->st[stream].committed : -1; }
int wc_warp_stream_get_delay(const wc_warp_stream *h, int stream) { return ws_stream_ok(h, stream) ? h->st[stream].delay : -1; }
int wc_warp_stream_track_length(const wc_warp_stream *h, int track) { return h && track >= 0 && track < h->n_tracks ? h->track_len[track] : -1; }

}  // extern "C"

