// The host half of the filter streams (wc_filter_stream.hip, include/world_class_filter_stream.h): the rule of that header on counts
// alone.  Which segments a push computes, which outputs it commits, what it keeps of the windows, and every refusal of create and of a
// push.  The centres c_t of both filter headers are stated here once (ff_centre), for the host and for the kernels of wc_filter.hip and
// wc_filter_stream.hip.
//
// Plain C++ with no HIP in it, so that a host compiler takes it alone (tests/cpp/filter_stream_plan_check.cpp).  A check gives its
// refusal's text, or nullptr; the translation unit puts its name in front and reports it.  A push is planned into steps (plan_push:
// host arithmetic only, nothing changes), the handle enqueues what the steps say, and then the steps become the state (commit).
//
//   The windows on the device.  A stream's sample window holds x[wb .. n) and its row window the rows rb - 1 .. F - 1, slot j for row
//   rb - 1 + j: wb = a_rb, and rb is the T the stream had in front of the push that wrote the window.  Slot 0 is the last row a done
//   segment used (nothing at rb == 0): the row a flush holds when no row is pending.  The next push skips what has been consumed since.
#pragma once
#include <cfloat>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define WC_FF_FN __host__ __device__ __forceinline__
#else
#define WC_FF_FN inline
#endif

namespace wc {

// c_t of THE rule of include/world_class_filter.h
WC_FF_FN long long ff_centre(long long t, double fp_ms, int fs) {
	return (long long)floor(((double)t * fp_ms) * (double)fs / 1000.0 + 0.5);
}
// a_t: where segment t starts
WC_FF_FN long long ff_start(long long t, double fp_ms, int fs) { return t ? ff_centre(t - 1, fp_ms, fs) + 1 : 0; }

inline double ff_hop(double fp_ms, int fs) { return fp_ms * (double)fs / 1000.0; }

// S of THE rule: the least count with c_{S-1} >= n - 1; 0 for n <= 0
inline long long ff_segments(long long n, double fp_ms, int fs) {
	if (n <= 0) return 0;
	long long t = (long long)ceil((double)(n - 1) / ff_hop(fp_ms, fs));
	while (ff_centre(t, fp_ms, fs) < n - 1) ++t;
	while (t > 0 && ff_centre(t - 1, fp_ms, fs) >= n - 1) --t;
	return t + 1;
}

// what wc_frame_filter_create refuses, and with it a stream's create
inline const char *ff_check_setting(int fs, bool fft_size_ok, int fft_size, double fp_ms) {
	if (!fft_size_ok) return "fft_size must be 512, 1024, 2048 or 4096";
	if (fs <= 0) return "fs must be positive";
	const double h = ff_hop(fp_ms, fs);
	if (!(h >= 1.0) || !(h <= DBL_MAX)) return "the hop frame_period_ms * fs / 1000 must be finite and at least 1";
	if (2.0 * ceil(h) - 1.0 > (double)(fft_size / 2)) return "the longest segment, 2 * ceil(hop) - 1 samples, must fit half the transform";
	return nullptr;
}

// T(n, F): the largest T with 0 <= T <= F and c_T <= n
inline long long fsp_segments_done(double fp_ms, int fs, long long n, long long F) {
	const double e = floor((double)n / ff_hop(fp_ms, fs));
	long long t = e >= (double)F ? F : (long long)e;
	if (t < 0) t = 0;
	while (t < F && ff_centre(t + 1, fp_ms, fs) <= n) ++t;
	while (t > 0 && ff_centre(t, fp_ms, fs) > n) --t;
	return t;
}
// C(T) = a_T
inline long long fsp_committed(double fp_ms, int fs, long long T) { return ff_start(T, fp_ms, fs); }

constexpr long long kFspMaxSamples = 2147483647ll;  // the rule's lengths are int
constexpr int kFspTile = 1024;                     // outputs, or window elements, of one workgroup

struct FspState {
	long long n = 0, F = 0, T = 0;  // samples and rows received, segments done
	long long C = 0;                // outputs committed: a_T, and n behind the flush
	long long wb = 0, rb = 0;       // the windows on the device start at sample wb and hold row rb - 1 in slot 0
	int cur = 0;                    // which of the pair holds the tail and the windows
	bool ended = false;             // flushed: samples and rows are refused until the reset
};

// what a push does with one stream
struct FspStep {
	bool active = false, flush = false;  // active: samples, rows or a flush; an idle stream is not touched
	long long n0 = 0, F0 = 0, T0 = 0, C0 = 0, n1 = 0, F1 = 0, T1 = 0, C1 = 0;
	int ns = 0, nr = 0;  // pushed
	int segs = 0, out = 0;  // T1 - T0 and C1 - C0
	int tail_n = 0;         // partial sums the old tail holds behind C0
};

struct FspPlan {
	int fs = 0, N = 0, n_streams = 0, max_s = 0, max_r = 0;
	double fp_ms = 0.0;
	std::vector<FspState> st;

	// nullptr, or why create refuses (the setting's own checks come first: ff_check_setting)
	static const char *check_create(int fs, int fft_size, double fp_ms, int kind, int n_streams, int max_s, int max_r) {
		if (kind != 0 && kind != 1) return "kind is 0 (power gains) or 1 (log amplitude gains)";
		if (n_streams < 1) return "n_streams must be at least 1";
		if ((double)max_s < 2.0 * ceil(ff_hop(fp_ms, fs))) return "max_pending_samples must be at least 2 * ceil(hop)";
		if (max_r < 1) return "max_pending_rows must be at least 1";
		// the pairs of windows and tails, the outputs of a push and its response rows (at most a segment per pending sample)
		const double streams = (double)n_streams, row = (double)(fft_size / 2 + 1);
		const double most = fmax(fmax(2.0 * streams * (double)max_s, 2.0 * streams * ((double)max_r + 1.0) * row), streams * (double)max_s * (double)fft_size);
		if (8.0 * most >= 9.0e18) return "a byte count leaves 63 bits";
		const double blocks = streams * fmax(((double)max_s + (double)fft_size) / kFspTile + 1.0, ((double)max_s + ((double)max_r + 1.0) * row) / kFspTile + 1.0);
		if (blocks >= 2.0e9) return "a launch grid leaves 31 bits";
		return nullptr;
	}
	void init(int fs_, int fft_size, double fp_ms_, int n_streams_, int max_s_, int max_r_) {
		fs = fs_; N = fft_size; fp_ms = fp_ms_; n_streams = n_streams_; max_s = max_s_; max_r = max_r_;
		st.assign((size_t)n_streams_, FspState());
	}
	bool ok(int u) const { return u >= 0 && u < n_streams; }
	int pending_samples(int u) const { return (int)(st[u].n - st[u].C); }
	int pending_rows(int u) const { return st[u].ended ? 0 : (int)(st[u].F - st[u].T); }
	void reset(int u) {  // a fresh stream; the pair's turn stays, T == 0 says that no tail is held
		const int cur = st[u].cur;
		st[u] = FspState();
		st[u].cur = cur;
	}

	// the refusal, or one step per stream and the call's totals; nothing changes
	const char *plan_push(const int *n_samples, const int *n_rows, const int *flush, std::vector<FspStep> &steps, long long *tot_s,
						  long long *tot_r, long long *tot_out, long long *tot_seg, int *n_active) const {
		*tot_s = *tot_r = *tot_out = *tot_seg = 0;
		*n_active = 0;
		steps.assign((size_t)n_streams, FspStep());
		for (int u = 0; u < n_streams; ++u) {
			const FspState &s = st[u];
			FspStep &p = steps[(size_t)u];
			p.ns = n_samples[u]; p.nr = n_rows[u];
			if (p.ns < 0 || p.nr < 0) return "a negative count";
			if (s.ended && (p.ns > 0 || p.nr > 0)) return "samples or rows for a stream that has ended (reset it first)";
			p.n0 = s.n; p.F0 = s.F; p.T0 = s.T;
			p.C0 = s.C;
			if ((s.n - p.C0) + p.ns > max_s || (s.F - s.T) + p.nr > max_r) return "a count that does not fit the windows (pending plus pushed)";
			if (s.n + p.ns > kFspMaxSamples) return "a stream would pass 2^31 - 1 samples";
			p.flush = flush && flush[u] && !s.ended;
			p.n1 = s.n + p.ns; p.F1 = s.F + p.nr;
			if (p.flush && p.n1 > 0 && p.F1 == 0) return "a flush of samples without a row";
			p.active = p.ns > 0 || p.nr > 0 || p.flush;
			p.T1 = p.T0; p.C1 = p.C0;
			if (!p.active) continue;
			p.T1 = p.flush ? ff_segments(p.n1, fp_ms, fs) : fsp_segments_done(fp_ms, fs, p.n1, p.F1);
			p.C1 = p.flush ? p.n1 : fsp_committed(fp_ms, fs, p.T1);
			p.segs = (int)(p.T1 - p.T0);
			p.out = (int)(p.C1 - p.C0);
			p.tail_n = p.T0 ? (int)(ff_start(p.T0 - 1, fp_ms, fs) + N - p.C0) : 0;
			*tot_s += p.ns; *tot_r += p.nr; *tot_out += p.out; *tot_seg += p.segs;
			*n_active += p.active ? 1 : 0;
		}
		return nullptr;
	}
	// everything of the call is enqueued
	void commit(const std::vector<FspStep> &steps) {
		for (int u = 0; u < n_streams; ++u) {
			const FspStep &p = steps[(size_t)u];
			if (!p.active) continue;
			FspState &s = st[u];
			s.n = p.n1; s.F = p.F1; s.T = p.T1; s.C = p.C1;
			s.wb = p.C0; s.rb = p.T0;
			s.cur = 1 - s.cur;
			s.ended = p.flush;
		}
	}
};

}  // namespace wc
