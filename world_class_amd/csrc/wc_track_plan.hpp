// The host half of the track-morph streams, stated once for the two handles that follow it: wc_track_morph (wc_track_morph.hip, full
// rows) and wc_track_morph_coded (wc_track_morph_coded.hip, coded rows).  It is the rule of include/world_class_track_morph.h on
// counts alone: which rows of the live voice form frames in a call, where each of them sits (a row of the push or a ring slot), which
// rows the call must keep, and every refusal.  A handle derives from TrackPlan and adds what the rule does not know: its row widths,
// its device arrays and their allocation, its kernels and the order it enqueues them in.  `name` leads every message.
//
//   The ring.  Row i of a stream with delay D forms frame i - D when row i's position arrives, so after a push the rows
//   max(n - D, 0) .. n - 1 wait: at most D.  Every row that is ever kept takes the next number of a sequence per stream and sits in
//   slot number % cap, cap = max_delay + min(max_delay, max_frames_per_push) -- wc_morph_stream's numbering: the rows a state holds
//   carry consecutive numbers, at most max_delay of them, and a push adds at most min(max_delay, max_frames_per_push) behind them,
//   so the new rows never land on a slot the state before the push still needs and a push that fails on the device leaves the rows
//   of the last good push.
//
//   A call plans in the record pair's staging and `next` (plan_push / plan_flush: host arithmetic, every refusal in front of the first
//   enqueue), uploads the records with one asynchronous copy (upload), enqueues its kernels, and the plan becomes the state (commit).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "wc_stages.hpp"

namespace wc {

struct TrackFrame {
	int row;    // voice A's row: >= 0 a row of the push's packed arrays, < 0 the ring slot ~row (counted over the whole handle)
	int pos;    // index of the frame's position in d_position_b (a push) or d_tail (the flush)
	int owner;  // the frame's stream: its settings and its track
	int pad;
};
struct TrackSet {  // a stream's settings at this call
	double w, wf, ra, rb;
	long long track_row;  // first row of the stream's track among the handle's track rows
	int m, pad;           // the track's rows
};
struct TrackKeep {
	int row, slot;  // row of the push's packed arrays -> ring slot
};

struct TrackState {
	int track = -1;      // -1: never reset onto a track
	int delay = 0;
	bool ended = false;  // flushed: rows are refused until the next reset
	long long n = 0;     // rows of the live voice received
	long long seq = 0;   // sequence number of row keep(): row r >= keep sits in slot (seq + r - keep) % cap
	double w = 0.0, wf = 0.0, ra = 0.0, rb = 0.0;
	long long keep() const { return ended ? n : std::max(n - delay, 0ll); }  // frames formed = the first row still waiting
};

// what a call planned: frames to form, rows to keep, and whether a stream that forms frames has a ratio
struct TrackCall {
	long long total_out = 0, n_keep = 0;
	bool stretch = false;
};
struct TrackRecs {  // the records of a call on the device
	const TrackSet *sets;
	const TrackFrame *frames;
	const TrackKeep *keeps;
};

struct TrackPlan {
	const char *name;  // "track morph" / "coded track morph"
	int fs, fft_size, n_streams, n_tracks, max_m, max_frames, max_delay, cap;  // cap: ring slots per stream
	Device *dev;
	std::vector<TrackState> st, next;  // next: the states a call plans, kept if it succeeds
	std::vector<int> track_m, cnt;
	RecPair rec;                 // the records of a call (reserved by the handle)
	TrackSet *staged = nullptr;  // the staging the call's plan took

	size_t frames_cap() const { return (size_t)n_streams * std::max(max_frames, max_delay); }
	size_t keeps_cap() const { return (size_t)n_streams * std::min(max_delay, max_frames); }
	// the records of a call, in the staging and on the device: the settings of every stream | the frames | the rows to keep
	size_t rec_bytes() const { return sizeof(TrackSet) * n_streams + sizeof(TrackFrame) * frames_cap() + sizeof(TrackKeep) * keeps_cap(); }
	int refuse(const char *what) const { return fail(WC_ERR_INVALID, std::string(name) + what); }

	// the arguments of create that both handles check alike: the refusal's text, or empty
	static std::string check(const char *name, int fs, int fft_size, int n_streams, int n_tracks, int max_track_frames, int max_frames_per_push,
							 int max_delay) {
		const std::string p = std::string(name) + ": ";
		if (!fft_size_supported(fft_size)) return p + "fft_size must be 512, 1024, 2048 or 4096";
		if (fs <= 0) return p + "fs must be positive";
		if (n_streams < 1 || n_tracks < 1 || max_track_frames < 1 || max_frames_per_push < 1)
			return p + "n_streams, n_tracks, max_track_frames and max_frames_per_push must be at least 1";
		if (max_delay < 0) return p + "max_delay must not be negative";
		return std::string();
	}
	// row and slot numbers are ints in the records: per_frame x frames of a call, the ring slots and the track rows fit one
	static bool fits(int n_streams, int n_tracks, int max_track_frames, int max_frames_per_push, int max_delay, long long per_frame) {
		const long long cap = (long long)max_delay + std::min(max_delay, max_frames_per_push);
		return per_frame * n_streams * std::max(max_frames_per_push, max_delay) <= 0x7fffffffll && (long long)n_streams * cap <= 0x7fffffffll &&
			   (long long)n_tracks * max_track_frames <= 0x7fffffffll;
	}
	void init(const char *name_, Device *dev_, int fs_, int fft_size_, int n_streams_, int n_tracks_, int max_track_frames, int max_frames_per_push,
			  int max_delay_) {
		name = name_; dev = dev_; fs = fs_; fft_size = fft_size_; n_streams = n_streams_; n_tracks = n_tracks_; max_m = max_track_frames;
		max_frames = max_frames_per_push; max_delay = max_delay_; cap = max_delay_ + std::min(max_delay_, max_frames_per_push);
		st.assign(n_streams, TrackState());
		next.reserve(n_streams);
		track_m.assign(n_tracks, 0);
		cnt.assign(n_streams, 0);
	}
	TrackSet *sets() const { return staged; }
	TrackFrame *frames() const { return reinterpret_cast<TrackFrame *>(sets() + n_streams); }
	TrackKeep *keeps() const { return reinterpret_cast<TrackKeep *>(frames() + frames_cap()); }  // (moved up behind the frames by upload)
	void set(const TrackState &q, TrackSet &s) const {
		s.w = q.w; s.wf = q.wf; s.ra = q.ra; s.rb = q.rb;
		s.track_row = q.track < 0 ? 0 : (long long)q.track * max_m;
		s.m = q.track < 0 ? 1 : track_m[q.track];
		s.pad = 0;
	}

	// A push of n_a[u] rows per stream, under the device's lock.  in_ok / out_ok: the call's input arrays / its position and output
	// arrays are all there.  Refuses, or fills the staging, `next`, frames_out and c; a call with nothing to enqueue is committed here.
	int plan_push(const int *n_a, bool in_ok, bool out_ok, int *frames_out, TrackCall *c) {
		const int n = n_streams;
		long long in = 0;
		for (int u = 0; u < n; ++u) {
			if (n_a[u] < 0) return refuse(" push: negative row count");
			if (n_a[u] > max_frames) return refuse(" push: more than max_frames_per_push rows for one stream");
			if (n_a[u] > 0 && st[u].track < 0) return refuse(" push: rows for a stream that was never reset onto a track");
			if (n_a[u] > 0 && st[u].ended) return refuse(" push: rows for a stream that has ended (reset it first)");
			in += n_a[u];
		}
		if (in > 0 && !in_ok) return refuse(" push: null input array");
		if (!(staged = rec.begin<TrackSet>())) return WC_ERR_DEVICE;
		TrackSet *sp = sets();
		TrackFrame *fr = frames();
		TrackKeep *kp = keeps();
		next = st;
		long long total_out = 0, n_keep = 0, off = 0;
		bool stretch = false;
		for (int u = 0; u < n; ++u) {
			const TrackState &old = st[u];
			TrackState &q = next[u];
			set(q, sp[u]);
			const int c_in = n_a[u];
			if (c_in == 0) { cnt[u] = 0; continue; }
			q.n = old.n + c_in;
			const long long keep_old = old.keep(), keep_new = q.keep(), base = (long long)u * cap;
			const int k_out = (int)(keep_new - keep_old);  // frames keep_old .. keep_new - 1: <= c_in <= max_frames_per_push
			for (int k = 0; k < k_out; ++k) {
				const long long t = keep_old + k;
				TrackFrame &f = fr[total_out + k];
				// row t of the voice: a row of this push, or the slot the state before the push holds it in (t - keep_old < delay <= cap)
				f.row = t >= old.n ? (int)(off + (t - old.n)) : ~(int)(base + (old.seq + (t - keep_old)) % cap);
				f.pos = (int)(off + (t + q.delay - old.n));  // the entry of row t + delay, which is a row of this push
				f.owner = u; f.pad = 0;
			}
			if (k_out > 0 && (q.ra != 0.0 || q.rb != 0.0)) stretch = true;
			const long long fresh = old.seq + (old.n - keep_old);  // the next unused number
			q.seq = keep_new < old.n ? old.seq + (keep_new - keep_old) : fresh;
			for (long long r = std::max(keep_new, old.n); r < q.n; ++r) {
				TrackKeep &k = kp[n_keep++];
				k.row = (int)(off + (r - old.n));
				k.slot = (int)(base + (q.seq + (r - keep_new)) % cap);
			}
			off += c_in;
			cnt[u] = k_out;
			total_out += k_out;
		}
		if (total_out > 0 && !out_ok) return refuse(" push: null position or output array");
		std::copy(cnt.begin(), cnt.end(), frames_out);  // (no refusal is left)
		if (total_out + n_keep == 0) st.swap(next);
		c->total_out = total_out; c->n_keep = n_keep; c->stretch = stretch;
		return WC_OK;
	}

	// The flush of the streams with want[u] != 0, under the device's lock.  out_ok: the tail and the output arrays are all there.
	int plan_flush(const int *want, bool out_ok, int *frames_out, TrackCall *c) {
		const int n = n_streams;
		for (int u = 0; u < n; ++u) {
			if (!want[u]) continue;
			const TrackState &s = st[u];
			if (s.track < 0 || s.ended) return refuse(" flush: a wanted stream is not attached or has ended");
			if (s.delay == 0 || s.n == 0) return refuse(" flush: a wanted stream has no delay or no rows");
		}
		if (!(staged = rec.begin<TrackSet>())) return WC_ERR_DEVICE;
		TrackSet *sp = sets();
		TrackFrame *fr = frames();
		next = st;
		long long total_out = 0, toff = 0;
		bool stretch = false;
		for (int u = 0; u < n; ++u) {
			TrackState &q = next[u];
			set(q, sp[u]);
			cnt[u] = 0;
			if (!want[u]) continue;
			const long long keep = q.keep(), base = (long long)u * cap;
			const int k_out = (int)(q.n - keep);                       // min(delay, n) rows wait
			const int K = (int)std::min<long long>(q.delay + 1, q.n);  // the stream's entries of d_tail: K - k_out in front belong to formed frames
			for (int k = 0; k < k_out; ++k) {
				TrackFrame &f = fr[total_out + k];
				f.row = ~(int)(base + (q.seq + k) % cap);
				f.pos = (int)(toff + (K - k_out) + k);
				f.owner = u; f.pad = 0;
			}
			if (q.ra != 0.0 || q.rb != 0.0) stretch = true;
			q.seq += k_out;
			q.ended = true;
			toff += K;
			cnt[u] = k_out;
			total_out += k_out;
		}
		if (total_out > 0 && !out_ok) return refuse(" flush: null tail or output array");
		std::copy(cnt.begin(), cnt.end(), frames_out);
		c->total_out = total_out; c->n_keep = 0; c->stretch = stretch;
		return WC_OK;
	}

	// the planned records to the device on hs: the keep records follow the frame records of this call in the staging and on the device
	int upload(hipStream_t hs, const TrackCall &c, TrackRecs *r) {
		std::memmove(frames() + c.total_out, keeps(), sizeof(TrackKeep) * (size_t)c.n_keep);
		const size_t bytes = sizeof(TrackSet) * (size_t)n_streams + sizeof(TrackFrame) * (size_t)c.total_out + sizeof(TrackKeep) * (size_t)c.n_keep;
		if (int rc = rec.upload(hs, bytes, &r->sets)) return rc;
		r->frames = reinterpret_cast<const TrackFrame *>(r->sets + n_streams);
		r->keeps = reinterpret_cast<const TrackKeep *>(r->frames + c.total_out);
		return WC_OK;
	}
	// everything of the call is enqueued: the plan becomes the state
	void commit() { st.swap(next); }
};

// ---- the bodies of the entry points that differ in nothing but the handle's name; h may be null, so the name comes with the call ----
inline int track_plan_refuse(const char *name, const char *what) { return fail(WC_ERR_INVALID, std::string(name) + what); }
inline bool track_plan_stream_ok(const TrackPlan *h, int u) { return h && u >= 0 && u < h->n_streams; }
inline bool track_plan_track_ok(const TrackPlan *h, int t) { return h && t >= 0 && t < h->n_tracks; }

// set_track's refusals and bookkeeping around the handle's own copies: copy(hs, first) enqueues the m rows to track row `first`
template <class Copy>
int track_plan_set_track(const char *name, TrackPlan *h, int track, int m, bool rows_ok, Copy copy) {
	if (!track_plan_track_ok(h, track)) return track_plan_refuse(name, ": bad track index");
	if (m < 1 || m > h->max_m) return h->refuse(" set_track: need 1 <= m <= max_track_frames");
	if (!rows_ok) return h->refuse(" set_track: null rows");
	DeviceLock lock(h->dev);
	for (const auto &s : h->st)
		if (s.track == track && s.n > 0) return h->refuse(" set_track: a stream that has received rows is attached to this track (reset it first)");
	WC_HIP(hipSetDevice(h->dev->id));
	if (int rc = copy(h->dev->active(), (size_t)track * h->max_m)) return rc;
	h->track_m[track] = m;
	return WC_OK;
}

inline int track_plan_reset(const char *name, TrackPlan *h, int stream, int track, int delay) {
	if (!track_plan_stream_ok(h, stream)) return track_plan_refuse(name, ": bad stream index");
	if (!track_plan_track_ok(h, track)) return h->refuse(": bad track index");
	if (delay < 0 || delay > h->max_delay) return h->refuse(" reset: need 0 <= delay <= max_delay");
	DeviceLock lock(h->dev);
	if (h->track_m[track] == 0) return h->refuse(" reset: the track has not been set");
	TrackState &s = h->st[stream];
	s = TrackState();  // (no row is held across a reset: the numbering may start again)
	s.track = track;
	s.delay = delay;
	return WC_OK;
}

inline int track_plan_set_weight(const char *name, TrackPlan *h, int stream, double weight, double f0_weight) {
	const auto finite = [](double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; };
	if (!track_plan_stream_ok(h, stream)) return track_plan_refuse(name, ": bad stream index");
	if (!(finite(weight) && finite(f0_weight))) return h->refuse(": the weight and the F0 weight must be finite");
	DeviceLock lock(h->dev);
	h->st[stream].w = weight;
	h->st[stream].wf = f0_weight;
	return WC_OK;
}

inline int track_plan_set_ratios(const char *name, TrackPlan *h, int stream, double ratio_a, double ratio_b) {
	if (!track_plan_stream_ok(h, stream)) return track_plan_refuse(name, ": bad stream index");
	if (!((ratio_a == 0.0 || frame_ratio_valid(ratio_a, h->fft_size)) && (ratio_b == 0.0 || frame_ratio_valid(ratio_b, h->fft_size))))
		return h->refuse(": a ratio must be 0 (none) or finite and >= 2.0 / fft_size");
	DeviceLock lock(h->dev);
	h->st[stream].ra = ratio_a;
	h->st[stream].rb = ratio_b;
	return WC_OK;
}

inline long long track_plan_frames_received(const TrackPlan *h, int stream) { return track_plan_stream_ok(h, stream) ? h->st[stream].n : -1; }
inline long long track_plan_frames_formed(const TrackPlan *h, int stream) { return track_plan_stream_ok(h, stream) ? h->st[stream].keep() : -1; }
inline int track_plan_pending(const TrackPlan *h, int stream) {
	return track_plan_stream_ok(h, stream) ? (int)(h->st[stream].n - h->st[stream].keep()) : WC_ERR_INVALID;
}
inline int track_plan_get_delay(const TrackPlan *h, int stream) { return track_plan_stream_ok(h, stream) ? h->st[stream].delay : -1; }
inline int track_plan_track_length(const TrackPlan *h, int track) { return track_plan_track_ok(h, track) ? h->track_m[track] : -1; }

}  // namespace wc
