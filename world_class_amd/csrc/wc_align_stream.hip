// Alignment streams (include/world_class_align_stream.h: wc_align_stream): a live voice is followed row by row through a known
// track.  The streaming form of wc_align_features_ex_device (wc_align.hip) at step pattern 0, band 0 and an open end: row i of D
// needs row i - 1 of D and row i of d only, so a stream carries one row of D from push to push and every pushed row gets the
// open-end scan of its own row of D -- the position in the track and the cost so far.  Two launches per push for the streams
// without a search window and one for those with, all bounded by counts the host wrote into the descriptors:
//
//   align_cost_kernel   (wc_align_cost.hpp, the whole call's kernel and so its rounding)  one AlPair per stream that has rows: the
//     pushed rows against the stream's track, W = m, no band, into the stream's part of the handle's d buffer.
//   align_stream_rows_kernel   one 64-lane wavefront per stream that has rows, no barrier, no LDS.  The rows are taken in passes of
//     up to 64: in a pass lane l owns pushed row i0 + l and does cell j = s - l at step s.  Lane l - 1 finished D(i - 1, j) one step
//     earlier and D(i - 1, j - 1) two steps earlier: the first arrives by one cross-lane move per step, the second is that move's
//     value of the step before; Dl is the lane's own last result.  Lane 0 takes Du / Dd from the stream's state row (D of the last
//     row before the pass; +inf in front of row 0), the lane of the pass's last row writes the new state row.  A stream has TWO
//     state rows and a pass reads one and writes the other, so within a pass no lane reads from memory a D that another lane wrote
//     (the principle of wc_align.hip); where a push takes more than one pass, a fence stands between a pass's last store and the
//     next pass's first load of that row.  Which row is current is host state, so a push that fails leaves the last good row.
//     Eight steps form a round: the eight local costs of the lane's row and (lane 0) eight cells of the state row are loaded
//     together, then the chain of three comparisons and one sum per cell runs on registers.  Each lane keeps its row's running
//     (best, j*) under the strict < of the open-end scan and writes d_position / d_cost when its row has ended.
//
//   align_window_rows_kernel   (include/world_class_align_window.h) the streams with a search window are left out of the two launches
//     above and take this one: one 64-lane wavefront per windowed stream that has rows, no barrier, no LDS.  The window's start is
//     decided on the device from a position that an earlier row of the same push produced, so the host cannot hand
//     align_cost_kernel the columns.  The host's part is the arithmetic of the passes: a pass never crosses an epoch boundary (hop rows
//     on the absolute row index, at most 64), so all its rows share one window [lo, lo + w).  Per pass: (a) lo and w from the window of
//     the row before, its position and the floor q -- read from the stream's record (AwRec) in front of the first pass, carried in
//     uniform registers between the passes, written back behind the last; (b) all 64 lanes compute the R x w local costs with
//     al_cell_costs (wc_align_cost.hpp: the cost kernel's arithmetic per cell) into the stream's part of d; a fence; (c) the
//     lane-skewed chain of the kernel above over the w columns from lo, where lane 0 takes a state cell only inside the window of the
//     row before (+inf outside: never stale memory) and starts its diagonal from D(i - 1, lo - 1) where the window has moved on.
//     Under WC_ALIGN_WINDOW_MONOTONE row i's floor is row i - 1's result: a pass of one row scans under the floor in the chain; a
//     longer pass stores D over d, and behind a fence the wavefront scans the rows one after the other, 64 columns at a time.
//
//   align_stream_settle_kernel, align_stream_tail_kernel   (include/world_class_align_lag.h) a stream with a lag has the two row
//     kernels store every cell's choice in a ring of bytes; behind them the settle kernel walks back from each pushed row's
//     position to the row `lag` frames ago, and the tail kernel does the same walk from the newest row on request.  Their comment
//     stands with them below.
//
//   A push is host arithmetic (every refusal), one asynchronous copy of the descriptors out of page-locked staging and the
//   launches (two for the plain streams, one for the windowed, one more for a settled push; a kind without rows is not launched);
//   set_track is one asynchronous device-to-device copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/world_class_io.h"
#include "../../include/world_class_stream.h"
#include "wc_align_cost.hpp"
#include "wc_stages.hpp"

using namespace wc;

namespace {

constexpr long long kAlignStreamMaxCells = 1ll << 28;  // n_streams x max_rows_per_push x max_track_frames: the whole call's cap

struct AsWork {
	long long out_off;  // first pushed row of the stream in the packed outputs
	long long d_off;    // the stream's local costs: n rows of m
	long long st_off;   // the stream's two state rows
	long long first;    // rows the stream had received before this push
	int n, m;           // rows pushed / rows of the track
	int parity;         // the state row that holds D of the last row before this push
	int flags;
	int u;                // the stream: its entry of lastpos
	unsigned char *ring;  // the stream's ring of choices (world_class_align_lag.h), or null: the stream has no lag
};

struct AsArgs {
	const AsWork *work;
	const double *d;
	double *state;
	long long max_m;  // doubles per state row, bytes per ring row
	double *position, *cost;
	int ring_cap;     // rows of a stream's ring
	int *lastpos;     // per stream with a lag: the column written for its newest row, -1 for NaN
};

// the choices of a cell, one byte each in a stream's ring: the whole call's three (wc_align_cost.hpp: AlArgs::choice) and the start
constexpr int AS_DIAG = 0, AS_UP = 1, AS_LEFT = 2, AS_START = 3;

// LAG: some stream of the launch has a ring.  A push whose streams have none runs the instantiation without the stores: the code
// of the kernel as it was before the ring.
template <bool LAG>
__global__ __launch_bounds__(64) void align_stream_rows_kernel(AsArgs A) {
	const AsWork w = A.work[blockIdx.x];
	const int lane = threadIdx.x;
	const double inf = __builtin_inf();
	const int m = w.m;
	const bool open_begin = (w.flags & WC_ALIGN_OPEN_BEGIN) != 0;
	int par = w.parity;
	for (int i0 = 0; i0 < w.n; i0 += 64) {  // (the trip counts of this loop and of the two below are the wavefront's)
		const int R = min(64, w.n - i0);    // rows of this pass
		const bool mine = lane < R, last = lane == R - 1;
		const bool has_prev = w.first + i0 > 0;      // a row of D lies above the pass
		const bool row0 = w.first + i0 + lane == 0;  // this lane's row is row 0 of the stream
		const double *__restrict__ src = A.state + w.st_off + (long long)par * A.max_m;
		double *__restrict__ dst = A.state + w.st_off + (long long)(par ^ 1) * A.max_m;
		const double *__restrict__ drow = A.d + w.d_off + (long long)(mine ? i0 + lane : i0) * m;
		// the ring row of this lane's row: absolute row % cap, indexed by the absolute column
		unsigned char *__restrict__ crow = LAG && w.ring ? w.ring + ((w.first + i0 + (mine ? lane : 0)) % A.ring_cap) * A.max_m : nullptr;
		double cur = inf;   // this lane's last result: D(i, j - 1), and what lane + 1 takes as D(i, j) one step later
		double diag = inf;  // what came from above one step ago: D(i - 1, j - 1)
		double best = inf;
		int bj = -1;
		const int steps = m + R - 1;
		for (int s0 = 0; s0 < steps; s0 += AL_CHUNK) {
			double dv[AL_CHUNK], sv[AL_CHUNK];
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				const int j = s0 + k - lane;
				const bool in = mine && j >= 0 && j < m;
				dv[k] = in ? drow[j] : 0.0;
				sv[k] = in && lane == 0 && has_prev ? src[j] : inf;
			}
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				double up = __shfl_up(cur, 1);  // D(i - 1, j): lane - 1 did column j one step ago (every lane is here at every step)
				if (lane == 0) up = sv[k];
				const int j = s0 + k - lane;
				if (mine && j >= 0 && j < m) {
					const double Dd = diag, Du = up, Dl = cur;
					double b;
					int c;
					if (Dd <= Du && Dd <= Dl) { b = Dd; c = AS_DIAG; }
					else if (Du <= Dl) { b = Du; c = AS_UP; }
					else { b = Dl; c = AS_LEFT; }
					const bool start = row0 && (open_begin || j == 0);
					const double D = start ? dv[k] : dv[k] + b;
					if (LAG && crow) crow[j] = (unsigned char)(start ? AS_START : c);
					if (D < best) { best = D; bj = j; }
					if (last) dst[j] = D;
					cur = D;
				}
				diag = up;
			}
		}
		if (mine) {  // the open-end scan of row i: the lowest column of the least D, or no winner (NaN or +inf throughout)
			const long long o = w.out_off + i0 + lane;
			A.cost[o] = bj >= 0 ? best : cur;  // (cur: D(i, m - 1))
			A.position[o] = bj >= 0 ? (double)bj : __builtin_nan("");
			if (LAG && w.ring && i0 + lane == w.n - 1) A.lastpos[w.u] = bj;  // (where wc_align_stream_tail_device starts)
		}
		par ^= 1;
		if (i0 + 64 < w.n) __threadfence();  // the new state row, before lane 0 of the next pass reads it
	}
}

constexpr int AW_CELLS = 4;  // local costs a lane computes side by side

struct AwWork {
	long long out_off;  // first pushed row of the stream in the packed rows and outputs
	long long b_off;    // first row of the stream's track
	long long d_off;    // the stream's local costs: row r of the push at r * m, column j of its window at j - lo
	long long st_off;   // the stream's two state rows (indexed by the absolute column)
	long long first;    // rows the stream had received before this push
	int u;              // the stream: its window record
	int n, m;           // rows pushed / rows of the track
	int parity;
	int flags;          // of the reset
	int W, back, hop;   // min(width, m), back, hop
	int monotone;
	unsigned char *ring;  // the stream's ring of choices, or null: the stream has no lag
};

// what the next row needs of the last: its window, its written position (-1: NaN) and the last position that was not NaN (0: none)
struct AwRec {
	int lo, w, pos, q;
};

struct AwArgs {
	const AwWork *work;
	const double *fa, *fb;
	double *d, *state;
	AwRec *rec;
	long long max_m;
	int dims, dim_begin, dim_end;
	double *position, *cost;
	int ring_cap;
	int *lastpos;
};

template <bool LAG>
__global__ __launch_bounds__(64) void align_window_rows_kernel(AwArgs A) {
	const AwWork w = A.work[blockIdx.x];
	const int lane = threadIdx.x;
	const double inf = __builtin_inf();
	const int m = w.m;
	const bool open_begin = (w.flags & WC_ALIGN_OPEN_BEGIN) != 0, monotone = w.monotone != 0;
	int par = w.parity;
	int plo = 0, pw = 0, ppos = -1, q = 0;  // the record of the row before the pass (uniform)
	if (w.first > 0) {
		const AwRec r = A.rec[w.u];
		plo = r.lo; pw = r.w; ppos = r.pos; q = r.q;
	}
	for (int i0 = 0; i0 < w.n;) {  // (every trip count below is the wavefront's, but for the loops that say otherwise)
		const long long abs0 = w.first + i0;
		const int in_epoch = (int)(abs0 % w.hop);
		const int R = min(w.n - i0, w.hop - in_epoch);  // rows of this pass: to the end of the push or of the epoch
		// (a) the window of the pass
		int lo = plo, wd = pw;
		if (abs0 == 0) {
			lo = 0; wd = open_begin ? m : w.W;
		} else if (in_epoch == 0) {
			lo = ppos < 0 ? plo : min(max(plo, ppos - w.back), m - w.W);
			wd = w.W;
		}
		// (b) the R x wd local costs
		double *dpass = A.d + w.d_off + (long long)i0 * m;
		const int cells = R * wd;  // (at most max_rows_per_push x max_track_frames <= 2^28)
		for (int base = 0; base < cells; base += 64 * AW_CELLS) {
			const double *pa[AW_CELLS], *pb[AW_CELLS];
			double v[AW_CELLS];
			long long at[AW_CELLS];
#pragma unroll
			for (int k = 0; k < AW_CELLS; ++k) {
				const int cell = base + 64 * k + lane;
				const int c = cell < cells ? cell : 0;  // (a lane without a cell computes cell 0 again and stores nothing)
				const int r = c / wd, jr = c - r * wd;
				pa[k] = A.fa + (w.out_off + i0 + r) * A.dims;
				pb[k] = A.fb + (w.b_off + lo + jr) * A.dims;
				at[k] = cell < cells ? (long long)r * m + jr : -1;
			}
			al_cell_costs<AW_CELLS>(pa, pb, A.dim_begin, A.dim_end, v);
#pragma unroll
			for (int k = 0; k < AW_CELLS; ++k)
				if (at[k] >= 0) dpass[at[k]] = v[k];
		}
		__threadfence();  // the local costs, before the lane of their row loads them
		// (c) the chain over the window
		const bool mine = lane < R, last = lane == R - 1;
		const bool has_prev = abs0 > 0;
		const bool row0 = abs0 + lane == 0;
		const bool post = monotone && R > 1;  // rows 1.. of the pass do not know their floor while the chain runs
		const int floor_j = monotone ? q : 0;
		const double *src = A.state + w.st_off + (long long)par * A.max_m;
		double *dst = A.state + w.st_off + (long long)(par ^ 1) * A.max_m;
		double *drow = dpass + (long long)(mine ? lane : 0) * m;
		unsigned char *crow = LAG && w.ring ? w.ring + ((abs0 + (mine ? lane : 0)) % A.ring_cap) * A.max_m : nullptr;
		double cur = inf;
		// D(i - 1, lo - 1): a cell of the window of the row before where the window has moved on, +inf otherwise
		double diag = lane == 0 && has_prev && lo - 1 >= plo && lo - 1 < plo + pw ? src[lo - 1] : inf;
		double best = inf;
		int bj = -1;
		const int steps = wd + R - 1;
		for (int s0 = 0; s0 < steps; s0 += AL_CHUNK) {
			double dv[AL_CHUNK], sv[AL_CHUNK];
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				const int jr = s0 + k - lane, j = lo + jr;
				const bool in = mine && jr >= 0 && jr < wd;
				dv[k] = in ? drow[jr] : 0.0;
				sv[k] = in && lane == 0 && has_prev && j >= plo && j < plo + pw ? src[j] : inf;
			}
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				double up = __shfl_up(cur, 1);
				if (lane == 0) up = sv[k];
				const int jr = s0 + k - lane, j = lo + jr;
				if (mine && jr >= 0 && jr < wd) {
					const double Dd = diag, Du = up, Dl = cur;
					double b;
					int c;
					if (Dd <= Du && Dd <= Dl) { b = Dd; c = AS_DIAG; }
					else if (Du <= Dl) { b = Du; c = AS_UP; }
					else { b = Dl; c = AS_LEFT; }
					const bool start = row0 && (open_begin || j == 0);
					const double D = start ? dv[k] : dv[k] + b;
					if (LAG && crow) crow[j] = (unsigned char)(start ? AS_START : c);
					if (j >= floor_j && D < best) { best = D; bj = j; }
					if (last) dst[j] = D;
					if (post) drow[jr] = D;
					cur = D;
				}
				diag = up;
			}
		}
		if (post) {  // the scans again, row after row under the floor the row before left: 64 columns at a time, the lowest column of the least D
			__threadfence();
			for (int r = 0; r < R; ++r) {
				const double *row = dpass + (long long)r * m;
				double b = inf;
				int at = -1;
				for (int jr = lane; jr < wd; jr += 64) {  // (the lane's own trip count: nothing crosses the lanes in here)
					const double D = row[jr];
					if (lo + jr >= q && D < b) { b = D; at = lo + jr; }
				}
#pragma unroll
				for (int off = 32; off > 0; off >>= 1) {
					const double ob = __shfl_xor(b, off);
					const int oa = __shfl_xor(at, off);
					if (ob < b || (ob == b && oa < at)) { b = ob; at = oa; }
				}
				if (lane == r) { best = b; bj = at; }
				if (at >= 0) q = at;
			}
		}
		if (mine) {
			const long long o = w.out_off + i0 + lane;
			A.cost[o] = bj >= 0 ? best : cur;  // (cur: D(i, lo + wd - 1))
			A.position[o] = bj >= 0 ? (double)bj : __builtin_nan("");
		}
		ppos = __builtin_amdgcn_readfirstlane(__shfl(bj, R - 1));
		if (monotone && !post && ppos >= 0) q = ppos;  // (a pass of one row)
		plo = lo; pw = wd;
		par ^= 1;
		i0 += R;
		if (i0 < w.n) __threadfence();  // the new state row, before lane 0 of the next pass reads it
	}
	if (lane == 0) {
		AwRec r;
		r.lo = plo; r.w = pw; r.pos = ppos; r.q = q;
		A.rec[w.u] = r;
		if (LAG && w.ring) A.lastpos[w.u] = ppos;
	}
}

// ---- settled positions from a lagged backtrack (include/world_class_align_lag.h) ----
//
// A stream with a lag keeps the choices of its last cap = max_lag + max_rows_per_push rows in a ring of bytes: the two kernels above
// store, for every cell they compute, which predecessor the three comparisons took (or AS_START), at ring row (absolute row) % cap and
// the absolute column.  A push of rows [f, f + n) walks back to rows >= f - L; the ring then holds rows f + n - cap .. f + n - 1,
// which covers them because n <= max_rows_per_push and L <= max_lag.
//
// Why stale ring bytes cannot show.  A walk starts at the winner of a row's scan, whose D is finite.  A cell's D is its cost plus the
// chosen predecessor, and where that sum is finite the predecessor is: the comparisons take a finite term over +inf and never a
// NaN.  So a path from a finite cell visits finite cells only -- cells that the stream computed since its reset, inside their rows'
// windows -- and never reads a byte from outside a row's window or from before the reset.  (The walks below still stop at a
// column below 0 or at a byte that is no choice, and give NaN: what a broken ring would cost is a wrong number, not a wild load.)
struct SeWork {
	long long out_off;  // settle: first pushed row of the stream in the packed outputs; tail: the stream's first entry of d_tail
	long long first;    // settle: rows received before this push; tail: rows received
	const unsigned char *ring;  // null (settle only): no lag, d_settled = d_position
	int u, n, lag;      // the stream; settle: rows pushed, tail: K entries to write; the lag
};

struct SeArgs {
	const SeWork *work;
	int n_work;       // (the tail's bound)
	long long max_m;  // bytes per ring row
	int ring_cap;
	const double *position;
	const int *lastpos;
	double *out;      // d_settled / d_tail
};

// the path's cells in one row: from (the row at ring slot `slot`, j) through the row's left steps to its lowest column, which
// replaces j.  The half-integer centre of the cells, or NaN where the walk breaks
__device__ inline double se_row(const SeArgs &A, const unsigned char *ring, int slot, int &j) {
	const unsigned char *row = ring + (long long)slot * A.max_m;
	const int jmax = j;
	while (row[j] == AS_LEFT) {  // (the lane's own trip count: nothing crosses the lanes in here)
		if (j == 0) return __builtin_nan("");
		--j;
	}
	return (j + jmax) * 0.5;
}

// one step up from the lowest cell (slot, j) of the path in a row: false where the byte is neither diagonal nor up
__device__ inline bool se_up(const SeArgs &A, const unsigned char *ring, int &slot, int &j) {
	const int c = ring[(long long)slot * A.max_m + j];
	if (c == AS_DIAG) {
		if (j == 0) return false;
		--j;
	} else if (c != AS_UP) {
		return false;
	}
	slot = slot == 0 ? A.ring_cap - 1 : slot - 1;
	return true;
}

// launched behind the row kernels of the same push, so that the order on the stream has made their choices and d_position
// visible: one 64-lane wavefront per stream that has rows, no barrier.  Lane l takes pushed rows l, l + 64, ..: from (i, j*_i) it
// walks its own path back to row t = max(i - L, 0) and through that row's left steps, and writes d_settled.  Every loop has the
// lane's own trip count (each step lowers the row or the column: at most L + m steps); nothing crosses the lanes.
__global__ __launch_bounds__(64) void align_stream_settle_kernel(SeArgs A) {
	const SeWork w = A.work[blockIdx.x];
	for (int r = threadIdx.x; r < w.n; r += 64) {
		const long long o = w.out_off + r;
		const double p = A.position[o];
		double s = p;
		if (w.ring && p == p) {
			const long long i = w.first + r;
			int up = (int)min(i, (long long)w.lag);  // rows to climb
			int slot = (int)(i % A.ring_cap), j = (int)p;
			s = se_row(A, w.ring, slot, j);
			while (up > 0 && s == s) {
				s = se_up(A, w.ring, slot, j) ? se_row(A, w.ring, slot, j) : __builtin_nan("");
				--up;
			}
		}
		A.out[o] = s;
	}
}

// wc_align_stream_tail_device: the same walk from the stream's newest row, one lane per wanted stream, writing every row it passes
__global__ __launch_bounds__(64) void align_stream_tail_kernel(SeArgs A) {
	const int k = blockIdx.x * 64 + threadIdx.x;
	if (k >= A.n_work) return;
	const SeWork w = A.work[k];
	double *out = A.out + w.out_off;
	int j = A.lastpos[w.u];
	int slot = (int)((w.first - 1) % A.ring_cap);
	bool ok = j >= 0;
	for (int e = w.n - 1; e >= 0; --e) {  // (entry e: row n - K + e)
		double s = __builtin_nan("");
		if (ok) {
			s = se_row(A, w.ring, slot, j);
			ok = s == s;
		}
		out[e] = s;
		if (ok && e > 0) ok = se_up(A, w.ring, slot, j);
	}
}

}  // namespace

struct wc_align_stream {
	int dims, dim_begin, dim_end, n_streams, n_tracks, max_m, max_rows;
	Device *dev;
	struct Stream {
		int track = -1;      // -1: never reset
		int flags = 0;
		int parity = 0;      // the state row that holds D of the newest row
		long long rows = 0;  // rows received since the reset
		int width = 0, back = 0, hop = 1, wflags = 0;  // the search window (world_class_align_window.h); width 0: none
		int lag = 0;         // the lag of the settled position (world_class_align_lag.h); 0: none
	};
	std::vector<Stream> st;
	std::vector<int> track_m;  // rows per slot, 0: empty
	DevBuf tracks;             // n_tracks x max_m rows of dims
	DevBuf d;                  // n_streams x max_rows x max_m local costs
	DevBuf state;              // n_streams x 2 x max_m
	DevBuf wrec;               // n_streams window records (AwRec)
	DevBuf ring;               // wc_align_stream_reserve_lag: n_streams x ring_cap x max_m choices, one byte each
	DevBuf lastpos;            // and n_streams ints: the column written for a stream's newest row
	int max_lag = 0, ring_cap = 0;  // 0: no reservation
	// the descriptors of a push: AlPair, then AsWork per plain stream with rows | AwWork per windowed stream with rows | SeWork per
	// stream with rows of a settled push; of a tail: SeWork per wanted stream
	RecPair rec;
};

namespace {

bool as_stream_ok(const wc_align_stream *h, int u) { return h && u >= 0 && u < h->n_streams; }
bool as_track_ok(const wc_align_stream *h, int t) { return h && t >= 0 && t < h->n_tracks; }

}  // namespace

extern "C" {

wc_align_stream *wc_align_stream_create(int dims, int dim_begin, int dim_end, int n_streams, int n_tracks, int max_track_frames,
										int max_rows_per_push) {
	if (dims < 1) { set_error("align stream: dims must be at least 1"); return nullptr; }
	if (dim_begin < 0 || dim_end > dims || dim_begin >= dim_end) { set_error("align stream: need 0 <= dim_begin < dim_end <= dims"); return nullptr; }
	if (n_streams < 1 || n_tracks < 1 || max_track_frames < 1 || max_rows_per_push < 1) {
		set_error("align stream: n_streams, n_tracks, max_track_frames and max_rows_per_push must be at least 1");
		return nullptr;
	}
	// (each factor is below 2^31 and the product of the first two is checked before the third comes in)
	const long long sr = (long long)n_streams * max_rows_per_push;
	if (sr > kAlignStreamMaxCells || sr * max_track_frames > kAlignStreamMaxCells) {
		set_error("align stream: n_streams x max_rows_per_push x max_track_frames above 2^28 cells");
		return nullptr;
	}
	const long long track_rows = (long long)n_tracks * max_track_frames;
	if (track_rows > kAlignStreamMaxCells || track_rows * dims > (1ll << 34)) {
		set_error("align stream: n_tracks x max_track_frames x dims too large");
		return nullptr;
	}
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	wc_align_stream *h = new wc_align_stream();
	h->dims = dims; h->dim_begin = dim_begin; h->dim_end = dim_end;
	h->n_streams = n_streams; h->n_tracks = n_tracks; h->max_m = max_track_frames; h->max_rows = max_rows_per_push;
	h->dev = dev;
	h->st.assign(n_streams, wc_align_stream::Stream());
	h->track_m.assign(n_tracks, 0);
	const size_t rec = (std::max(sizeof(AlPair) + sizeof(AsWork), sizeof(AwWork)) + sizeof(SeWork)) * (size_t)n_streams;
	if (h->wrec.reserve(sizeof(AwRec) * (size_t)n_streams) || h->tracks.reserve(sizeof(double) * (size_t)track_rows * dims) || h->d.reserve(sizeof(double) * (size_t)sr * max_track_frames) ||
		h->state.reserve(sizeof(double) * (size_t)2 * n_streams * max_track_frames) || h->rec.reserve(rec)) {
		wc_align_stream_destroy(h);
		return nullptr;
	}
	return h;
}

void wc_align_stream_destroy(wc_align_stream *h) {
	if (!h) return;
	h->dev->quiesce();
	h->tracks.release(); h->d.release(); h->state.release(); h->wrec.release(); h->ring.release(); h->lastpos.release(); h->rec.release();
	delete h;
}

int wc_align_stream_set_track_device(wc_align_stream *h, int track, int m, const double *d_feat_b) {
	if (!as_track_ok(h, track)) return fail(WC_ERR_INVALID, "align stream: bad track index");
	if (m < 1 || m > h->max_m) return fail(WC_ERR_INVALID, "align stream set_track: need 1 <= m <= max_track_frames");
	if (!d_feat_b) return fail(WC_ERR_INVALID, "align stream set_track: null rows");
	DeviceLock lock(h->dev);
	for (const auto &s : h->st)
		if (s.track == track && s.rows > 0)
			return fail(WC_ERR_INVALID, "align stream set_track: a stream that has received rows follows this track (reset it first)");
	WC_HIP(hipSetDevice(h->dev->id));
	double *to = h->tracks.as<double>() + (size_t)track * h->max_m * h->dims;
	WC_HIP(hipMemcpyAsync(to, d_feat_b, sizeof(double) * (size_t)m * h->dims, hipMemcpyDeviceToDevice, h->dev->active()));
	h->track_m[track] = m;
	return WC_OK;
}

int wc_align_stream_reset(wc_align_stream *h, int stream, int track, int flags) {
	if (!as_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "align stream: bad stream index");
	if (!as_track_ok(h, track)) return fail(WC_ERR_INVALID, "align stream: bad track index");
	if (flags != 0 && flags != WC_ALIGN_OPEN_BEGIN) return fail(WC_ERR_INVALID, "align stream reset: flags must be 0 or WC_ALIGN_OPEN_BEGIN");
	DeviceLock lock(h->dev);
	if (h->track_m[track] == 0) return fail(WC_ERR_INVALID, "align stream reset: the track has not been set");
	wc_align_stream::Stream &s = h->st[stream];
	s.track = track; s.flags = flags; s.rows = 0;  // (the parity stays: row 0 reads no state row)
	s.width = 0; s.back = 0; s.hop = 1; s.wflags = 0;
	s.lag = 0;
	return WC_OK;
}

}  // extern "C"

namespace {

// wc_align_stream_push_device (settle = false: d_settled is not looked at) and wc_align_stream_push_settled_device
int as_push(wc_align_stream *h, const int *n_rows, const double *d_feat_a, double *d_position, double *d_cost, double *d_settled, bool settle) {
	if (!h || !n_rows) return fail(WC_ERR_INVALID, "align stream push: null argument");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	long long total = 0;
	int plain = 0, windowed = 0;  // streams with rows: without / with a search window
	for (int u = 0; u < n; ++u) {
		if (n_rows[u] < 0) return fail(WC_ERR_INVALID, "align stream push: negative row count");
		if (n_rows[u] > h->max_rows) return fail(WC_ERR_INVALID, "align stream push: more than max_rows_per_push rows for one stream");
		if (n_rows[u] > 0 && h->st[u].track < 0) return fail(WC_ERR_INVALID, "align stream push: rows for a stream that was never reset onto a track");
		total += n_rows[u];
		if (n_rows[u] > 0) ++(h->st[u].width > 0 ? windowed : plain);
	}
	if (total == 0) return WC_OK;
	if (!d_feat_a || !d_position || !d_cost || (settle && !d_settled)) return fail(WC_ERR_INVALID, "align stream push: null array");
	// ---- the descriptors (no refusal is left) ----
	AlPair *pairs = h->rec.begin<AlPair>();
	if (!pairs) return WC_ERR_DEVICE;
	AsWork *work = reinterpret_cast<AsWork *>(pairs + plain);
	AwWork *wwork = reinterpret_cast<AwWork *>(work + plain);
	SeWork *swork = reinterpret_cast<SeWork *>(wwork + windowed);
	const int settled = settle ? plain + windowed : 0;  // a settled push: one item per stream with rows
	long long off = 0, tiles = 0;
	int k = 0, kw = 0, ks = 0;
	bool plain_lag = false, windowed_lag = false;  // a stream of the kind has rows and a ring
	for (int u = 0; u < n; ++u) {
		const int c = n_rows[u];
		if (c == 0) continue;
		const wc_align_stream::Stream &s = h->st[u];
		const int m = h->track_m[s.track];
		const long long b_off = (long long)s.track * h->max_m, d_off = (long long)u * h->max_rows * h->max_m;
		const long long st_off = (long long)u * 2 * h->max_m;
		unsigned char *ring = s.lag > 0 ? h->ring.as<unsigned char>() + (size_t)u * h->ring_cap * h->max_m : nullptr;
		if (settle) {
			SeWork &e = swork[ks++];
			e.out_off = off; e.first = s.rows; e.ring = ring;
			e.u = u; e.n = c; e.lag = s.lag;
		}
		if (s.width > 0) {
			AwWork &w = wwork[kw++];
			w.out_off = off; w.b_off = b_off; w.d_off = d_off; w.st_off = st_off; w.first = s.rows;
			w.u = u; w.n = c; w.m = m; w.parity = s.parity; w.flags = s.flags;
			w.W = std::min(s.width, m); w.back = s.back; w.hop = s.hop; w.monotone = (s.wflags & WC_ALIGN_WINDOW_MONOTONE) != 0;
			w.ring = ring;
			windowed_lag |= ring != nullptr;
			off += c;
			continue;
		}
		AlPair &q = pairs[k];
		q.a_off = off; q.b_off = b_off;
		q.cell_off = d_off;
		q.path_off = 0; q.tile_off = tiles; q.B = -1;
		q.n = c; q.m = m; q.W = m;
		q.tiles_j = (m + AL_TILE - 1) / AL_TILE;
		tiles += (long long)((c + AL_TILE - 1) / AL_TILE) * q.tiles_j;
		AsWork &w = work[k];
		w.out_off = off; w.d_off = d_off; w.st_off = st_off; w.first = s.rows;
		w.n = c; w.m = m; w.parity = s.parity; w.flags = s.flags;
		w.u = u; w.ring = ring;
		plain_lag |= ring != nullptr;
		off += c;
		++k;
	}
	// (tiles <= cells / 1024 + rows + columns: far below 2^31)
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	int rc;
	const size_t bytes = (sizeof(AlPair) + sizeof(AsWork)) * (size_t)plain + sizeof(AwWork) * (size_t)windowed + sizeof(SeWork) * (size_t)settled;
	const AlPair *d_pairs;
	if ((rc = h->rec.upload(hs, bytes, &d_pairs))) return rc;
	const AsWork *d_work = reinterpret_cast<const AsWork *>(d_pairs + plain);
	if (plain > 0) {
		AlArgs a = {};
		a.pairs = d_pairs;
		a.n_pairs = plain; a.dims = h->dims; a.dim_begin = h->dim_begin; a.dim_end = h->dim_end;
		a.fa = d_feat_a; a.fb = h->tracks.as<double>();
		a.cells = h->d.as<double>();
		AsArgs x;
		x.work = d_work;
		x.d = h->d.as<double>(); x.state = h->state.as<double>(); x.max_m = h->max_m;
		x.position = d_position; x.cost = d_cost;
		x.ring_cap = h->ring_cap; x.lastpos = h->lastpos.as<int>();
		if ((rc = h->dev->time_begin("align_stream_cost_kernel", hs))) return rc;
		hipLaunchKernelGGL(align_cost_kernel, dim3((unsigned)tiles), dim3(256), 0, hs, a);
		WC_HIP(hipGetLastError());
		if ((rc = h->dev->time_end("align_stream_cost_kernel", hs))) return rc;
		if ((rc = h->dev->time_begin("align_stream_rows_kernel", hs))) return rc;
		if (plain_lag) hipLaunchKernelGGL(align_stream_rows_kernel<true>, dim3((unsigned)plain), dim3(64), 0, hs, x);
		else hipLaunchKernelGGL(align_stream_rows_kernel<false>, dim3((unsigned)plain), dim3(64), 0, hs, x);
		WC_HIP(hipGetLastError());
		if ((rc = h->dev->time_end("align_stream_rows_kernel", hs))) return rc;
	}
	if (windowed > 0) {
		AwArgs x;
		x.work = reinterpret_cast<const AwWork *>(d_work + plain);
		x.fa = d_feat_a; x.fb = h->tracks.as<double>();
		x.d = h->d.as<double>(); x.state = h->state.as<double>(); x.rec = h->wrec.as<AwRec>(); x.max_m = h->max_m;
		x.dims = h->dims; x.dim_begin = h->dim_begin; x.dim_end = h->dim_end;
		x.position = d_position; x.cost = d_cost;
		x.ring_cap = h->ring_cap; x.lastpos = h->lastpos.as<int>();
		if ((rc = h->dev->time_begin("align_window_rows_kernel", hs))) return rc;
		if (windowed_lag) hipLaunchKernelGGL(align_window_rows_kernel<true>, dim3((unsigned)windowed), dim3(64), 0, hs, x);
		else hipLaunchKernelGGL(align_window_rows_kernel<false>, dim3((unsigned)windowed), dim3(64), 0, hs, x);
		WC_HIP(hipGetLastError());
		if ((rc = h->dev->time_end("align_window_rows_kernel", hs))) return rc;
	}
	if (settled > 0) {  // behind the row kernels: their choices and d_position are visible by the order on the stream
		SeArgs x = {};
		x.work = reinterpret_cast<const SeWork *>(reinterpret_cast<const AwWork *>(d_work + plain) + windowed);
		x.n_work = settled; x.max_m = h->max_m; x.ring_cap = h->ring_cap;
		x.position = d_position; x.lastpos = h->lastpos.as<int>(); x.out = d_settled;
		if ((rc = h->dev->time_begin("align_stream_settle_kernel", hs))) return rc;
		hipLaunchKernelGGL(align_stream_settle_kernel, dim3((unsigned)settled), dim3(64), 0, hs, x);
		WC_HIP(hipGetLastError());
		if ((rc = h->dev->time_end("align_stream_settle_kernel", hs))) return rc;
	}
	for (int u = 0; u < n; ++u) {
		wc_align_stream::Stream &s = h->st[u];
		if (n_rows[u] == 0) continue;
		// one flip per pass: of up to 64 rows, or under a window of the rows of one epoch
		const long long passes = s.width > 0 ? (s.rows + n_rows[u] - 1) / s.hop - s.rows / s.hop + 1 : (n_rows[u] + 63) / 64;
		s.rows += n_rows[u];
		s.parity ^= (int)(passes & 1);
	}
	return WC_OK;
}

}  // namespace

extern "C" {

int wc_align_stream_push_device(wc_align_stream *h, const int *n_rows, const double *d_feat_a, double *d_position, double *d_cost) {
	return as_push(h, n_rows, d_feat_a, d_position, d_cost, nullptr, false);
}

int wc_align_stream_push_settled_device(wc_align_stream *h, const int *n_rows, const double *d_feat_a, double *d_position, double *d_cost,
										double *d_settled) {
	return as_push(h, n_rows, d_feat_a, d_position, d_cost, d_settled, true);
}

int wc_align_stream_reserve_lag(wc_align_stream *h, int max_lag) {
	if (!h) return fail(WC_ERR_INVALID, "align stream reserve_lag: null handle");
	if (max_lag < 1) return fail(WC_ERR_INVALID, "align stream reserve_lag: max_lag must be at least 1");
	DeviceLock lock(h->dev);
	if (h->max_lag > 0) return fail(WC_ERR_INVALID, "align stream reserve_lag: the handle has a reservation");
	// (64-bit, a factor at a time: cap <= 2^32, n_streams x cap <= 2^60, and only a product within 2^30 meets the next factor)
	const long long cap = (long long)max_lag + h->max_rows, limit = 1ll << 30;
	if (cap > limit || cap * h->n_streams > limit || cap * h->n_streams * h->max_m > limit)
		return fail(WC_ERR_INVALID, "align stream reserve_lag: n_streams x (max_lag + max_rows_per_push) x max_track_frames above 2^30 bytes");
	WC_HIP(hipSetDevice(h->dev->id));
	if (h->ring.reserve((size_t)(cap * h->n_streams * h->max_m)) || h->lastpos.reserve(sizeof(int) * (size_t)h->n_streams)) {
		h->ring.release(); h->lastpos.release();
		return WC_ERR_DEVICE;
	}
	h->max_lag = max_lag; h->ring_cap = (int)cap;
	return WC_OK;
}

int wc_align_stream_set_lag(wc_align_stream *h, int stream, int lag) {
	if (!as_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "align stream: bad stream index");
	DeviceLock lock(h->dev);
	if (lag < 0 || lag > h->max_lag) return fail(WC_ERR_INVALID, "align stream set_lag: need 0 <= lag <= max_lag of wc_align_stream_reserve_lag");
	wc_align_stream::Stream &s = h->st[stream];
	if (s.track < 0) return fail(WC_ERR_INVALID, "align stream set_lag: the stream was never reset onto a track");
	if (s.rows > 0) return fail(WC_ERR_INVALID, "align stream set_lag: the stream has received rows (reset it first)");
	s.lag = lag;
	return WC_OK;
}

int wc_align_stream_get_lag(const wc_align_stream *h, int stream) {
	if (!as_stream_ok(h, stream)) return -1;
	return h->st[stream].lag;
}

int wc_align_stream_tail_device(wc_align_stream *h, const int *want, double *d_tail) {
	if (!h || !want || !d_tail) return fail(WC_ERR_INVALID, "align stream tail: null argument");
	DeviceLock lock(h->dev);
	int count = 0;
	for (int u = 0; u < h->n_streams; ++u) {
		if (!want[u]) continue;
		if (h->st[u].lag == 0) return fail(WC_ERR_INVALID, "align stream tail: a wanted stream has no lag");
		if (h->st[u].rows == 0) return fail(WC_ERR_INVALID, "align stream tail: a wanted stream has no rows");
		++count;
	}
	if (count == 0) return WC_OK;
	SeWork *work = h->rec.begin<SeWork>();
	if (!work) return WC_ERR_DEVICE;
	long long off = 0;
	int k = 0;
	for (int u = 0; u < h->n_streams; ++u) {
		if (!want[u]) continue;
		const wc_align_stream::Stream &s = h->st[u];
		SeWork &e = work[k++];
		e.out_off = off; e.first = s.rows;
		e.ring = h->ring.as<unsigned char>() + (size_t)u * h->ring_cap * h->max_m;
		e.u = u; e.n = (int)std::min<long long>(s.lag + 1, s.rows); e.lag = s.lag;
		off += e.n;
	}
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	int rc;
	SeArgs x = {};
	if ((rc = h->rec.upload(hs, sizeof(SeWork) * (size_t)count, &x.work))) return rc;
	x.n_work = count; x.max_m = h->max_m; x.ring_cap = h->ring_cap;
	x.lastpos = h->lastpos.as<int>(); x.out = d_tail;
	if ((rc = h->dev->time_begin("align_stream_tail_kernel", hs))) return rc;
	hipLaunchKernelGGL(align_stream_tail_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, hs, x);
	WC_HIP(hipGetLastError());
	if ((rc = h->dev->time_end("align_stream_tail_kernel", hs))) return rc;
	return WC_OK;
}

int wc_align_stream_set_window(wc_align_stream *h, int stream, int width, int back, int hop, int flags) {
	if (!as_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "align stream: bad stream index");
	if (width < 0 || back < 0 || (width > 0 ? back >= width : back != 0))
		return fail(WC_ERR_INVALID, "align stream set_window: need 0 <= back < width, or width = 0 and back = 0");
	if (hop < 1 || hop > 64 || (width == 0 && hop != 1)) return fail(WC_ERR_INVALID, "align stream set_window: need 1 <= hop <= 64, and hop = 1 with width = 0");
	if ((flags != 0 && flags != WC_ALIGN_WINDOW_MONOTONE) || (width == 0 && flags != 0))
		return fail(WC_ERR_INVALID, "align stream set_window: flags must be 0 or WC_ALIGN_WINDOW_MONOTONE, and 0 with width = 0");
	DeviceLock lock(h->dev);
	wc_align_stream::Stream &s = h->st[stream];
	if (s.track < 0) return fail(WC_ERR_INVALID, "align stream set_window: the stream was never reset onto a track");
	if (s.rows > 0) return fail(WC_ERR_INVALID, "align stream set_window: the stream has received rows (reset it first)");
	s.width = width; s.back = back; s.hop = hop; s.wflags = flags;
	return WC_OK;
}

int wc_align_stream_get_window(const wc_align_stream *h, int stream, int *width, int *back, int *hop, int *flags) {
	if (!as_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "align stream: bad stream index");
	if (!width || !back || !hop || !flags) return fail(WC_ERR_INVALID, "align stream get_window: null pointer");
	const wc_align_stream::Stream &s = h->st[stream];
	*width = s.width; *back = s.back; *hop = s.hop; *flags = s.wflags;
	return WC_OK;
}

long long wc_align_stream_rows_received(const wc_align_stream *h, int stream) {
	if (!as_stream_ok(h, stream)) return -1;
	return h->st[stream].rows;
}

int wc_align_stream_track_length(const wc_align_stream *h, int track) {
	if (!as_track_ok(h, track)) return -1;
	return h->track_m[track];
}

}  // extern "C"
