// The host half that the two lagged row streams share, stated once: wc_mlpg_stream (wc_mlpg_stream.hip, include/world_class_mlpg_stream.h)
// and wc_feature_stream (wc_feature_stream.hip, include/world_class_feature_stream.h).  It is the rule of those headers on counts alone:
// a stream reset with lag L that has received T rows has emitted E(T) = max(T - L, 0) frames; a push of k rows emits E(T + k) - E(T), a
// flush the T - E(T) rows that still wait, and it ends the stream until the next reset.  A handle derives from LagLedger<its State> and
// adds what the rule does not know: its kernels, its descriptors and how it fills them, its own checks, its enqueue, and what a reset
// keeps of a state.
//
// Plain C++ with no HIP in it, so that a host compiler takes it alone (tests/cpp/lag_ledger_check.cpp).  A check gives its refusal's
// text, or nullptr; the translation unit puts its name in front and reports it.  The order of the checks in an entry point is the
// order the public headers state.
//
// Not for the alignment streams' lag (include/world_class_align_lag.h): that one follows another rule -- its tail is lag + 1 entries,
// it has no ended state, and the lag is set behind a reset, not by it.  Nor for the warp streams' delay.
#pragma once
#include <vector>

namespace wc {

struct LagState {
	int lag = -1;  // -1: never reset
	bool ended = false;
	long long rows = 0, emitted = 0;
};

inline long long emitted_of(long long rows, int lag) { return rows < 0 || lag < 0 ? -1 : (rows > lag ? rows - lag : 0); }

// create's checks that both streams make alike, in two parts: a stream's own check of `orders` stands between them
inline const char *lag_check_dims(int nd, int n_ap) { return nd < 1 || n_ap < 0 ? ": nd must be at least 1 and n_ap not negative" : nullptr; }
// width: wc_model_feature_width of the rows; row_doubles: doubles of one ring row.  The ring has cap = max_lag + max_rows_per_push + 1
// rows per stream.  In 64 bits: a row and cap are looked at first, and up to 2^27 each their product in bytes stays within 2^57; under
// the bound the descriptor and block counts of a call stay far below 2^31 as well.
inline const char *lag_check_create(int width, int n_streams, int max_rows_per_push, int max_lag, unsigned long long row_doubles) {
	if (width < 0) return ": the row width leaves 31 bits";
	if (n_streams < 1 || max_rows_per_push < 1) return ": n_streams and max_rows_per_push must be at least 1";
	if (max_lag < 0) return ": max_lag must not be negative";
	const unsigned long long cap = (unsigned long long)max_lag + max_rows_per_push + 1, ring_bytes = 8ull * row_doubles * cap;  // of one stream
	if (row_doubles > (1ull << 27) || cap > (1ull << 27) || ring_bytes > (1ull << 30) || ring_bytes * (unsigned long long)n_streams > (1ull << 30))
		return ": the ring exceeds 2^30 bytes";
	return nullptr;
}

template <class State> struct LagLedger {
	int n_streams = 0, max_rows = 0, max_lag = 0;
	int cap = 0;  // ring slots per stream: the absolute row index modulo cap (each handle says why the one slot of margin)
	std::vector<State> st;

	void init(int n_streams_, int max_rows_per_push, int max_lag_) {
		n_streams = n_streams_; max_rows = max_rows_per_push; max_lag = max_lag_;
		cap = max_lag_ + max_rows_per_push + 1;
		st.assign((size_t)n_streams_, State());
	}
	// a push of n_rows[u] rows per stream: the refusal, or the rows it takes and the frames it emits over all streams
	const char *scan_push(const int *n_rows, long long *total_rows, long long *total_out) const {
		*total_rows = 0; *total_out = 0;
		for (int u = 0; u < n_streams; ++u) {
			const State &s = st[u];
			if (n_rows[u] < 0 || n_rows[u] > max_rows) return " push: a count outside 0 .. max_rows_per_push";
			if (n_rows[u] > 0 && (s.lag < 0 || s.ended)) return " push: rows for a stream that was never reset or has ended (reset it first)";
			*total_rows += n_rows[u];
			*total_out += push_frames(u, n_rows[u]);
		}
		return nullptr;
	}
	// the flush of the streams with want[u] != 0: the refusal, or the frames it emits over all streams
	const char *scan_flush(const int *want, long long *total_out) const {
		*total_out = 0;
		for (int u = 0; u < n_streams; ++u) {
			if (want[u] && (st[u].lag < 0 || st[u].ended)) return " flush: a wanted stream was never reset or has ended";
			*total_out += flush_frames(u, want[u]);
		}
		return nullptr;
	}
	// a stream's frames_out: behind k more rows, and in a flush -- min(lag, rows)
	int push_frames(int u, int k) const { return k > 0 ? (int)(emitted_of(st[u].rows + k, st[u].lag) - st[u].emitted) : 0; }
	int flush_frames(int u, int want) const { return want ? (int)(st[u].rows - st[u].emitted) : 0; }
	// everything of the call is enqueued
	void commit_push(const int *n_rows, const int *frames_out) {
		for (int u = 0; u < n_streams; ++u) {
			st[u].rows += n_rows[u];
			st[u].emitted += frames_out[u];  // (0 where no rows came)
		}
	}
	void commit_flush(const int *want, const int *frames_out) {
		for (int u = 0; u < n_streams; ++u) {
			if (!want[u]) continue;
			st[u].emitted += frames_out[u];
			st[u].ended = true;
		}
	}
};

// ---- what the entry points ask of a handle that may be null ----
template <class L> bool lag_stream_ok(const L *h, int stream) { return h && stream >= 0 && stream < h->n_streams; }
template <class L> const char *lag_check_reset(const L *h, int stream, int lag) {
	if (!lag_stream_ok(h, stream)) return " reset: bad stream index";
	if (lag < 0 || lag > h->max_lag) return " reset: a lag outside 0 .. max_lag";
	return nullptr;
}
template <class L> int lag_max_frames_per_push(const L *h, int none) { return h ? h->max_rows : none; }
template <class L> int lag_max_frames_per_flush(const L *h, int none) { return h ? h->max_lag : none; }
template <class L> long long lag_rows_received(const L *h, int stream) { return lag_stream_ok(h, stream) ? h->st[stream].rows : -1; }
template <class L> long long lag_frames_emitted(const L *h, int stream) { return lag_stream_ok(h, stream) ? h->st[stream].emitted : -1; }
template <class L> int lag_get_lag(const L *h, int stream) { return lag_stream_ok(h, stream) ? h->st[stream].lag : -1; }

}  // namespace wc
