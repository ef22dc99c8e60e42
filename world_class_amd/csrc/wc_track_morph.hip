// Track-morph streams (include/world_class_track_morph.h: wc_track_morph): a live voice arrives push by push and is morphed with a
// track that is resident in the handle, at positions in the track that the kernel reads from device memory -- the settled positions
// of an alignment stream (world_class_align_lag.h) as they are written, without a trip to the host.  The handle sits in front of a
// synthesis stream as wc_morph_stream does (wc_morph_stream.hip) and is the streaming form of wc_morph_parameters_device
// (wc_morph.hip) at d_position_a = the frame's own index.
//
//   track_morph_kernel<STRETCH>   one workgroup of RT_T lanes per formed frame.  The workgroup reads its position itself (one double
//     of d_position_b or d_tail at an index the host wrote, the same for every lane), places it in the track with rt_place -- the
//     clamp to [0, m - 1] and the frame that is all NaN for a position that is not finite are morph_kernel's -- and blends with the
//     expressions of wc_retime_rows.hpp and wc_morph_rows.hpp in morph_kernel's order, so it has that kernel's bits.  Voice A's side
//     is those expressions at a whole position (a = 0, w0 = 1: rt_pair / rt_row / rt_f0 / rt_log_row return the row itself); its row
//     is a row of the push's packed arrays or a ring slot, resolved by the host, which knows it from counts alone.  Voice B's two
//     rows are rows of the stream's track.  Workgroups behind the formed frames copy the rows each stream must keep (TmKeep) into
//     ring slots that no workgroup of the launch reads.  STRETCH = false: no LDS; chosen by the host when no stream that forms frames
//     in the call has a ratio.
//
//   The ring.  Row i of a stream with delay D forms frame i - D when row i's position arrives, so after a push the rows
//   max(n - D, 0) .. n - 1 wait: at most D.  Every row that is ever kept takes the next number of a sequence per stream and sits in
//   slot number % cap, cap = max_delay + min(max_delay, max_frames_per_push) -- wc_morph_stream's numbering: the rows a state holds
//   carry consecutive numbers, at most max_delay of them, and a push adds at most min(max_delay, max_frames_per_push) behind them,
//   so the new rows never land on a slot the state before the push still needs and a push that fails on the device leaves the rows
//   of the last good push.
//
//   A push is host arithmetic on counts (the rule, every refusal), one asynchronous copy of the settings, frame and keep records out
//   of page-locked staging, and one launch.  No host code looks at a position.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/world_class_stream.h"
#include "wc_morph_rows.hpp"
#include "wc_retime_rows.hpp"
#include "wc_stages.hpp"

using namespace wc;

namespace {

struct TmFrame {
	int row;    // voice A's row: >= 0 a row of the push's packed arrays, < 0 the ring slot ~row (counted over the whole handle)
	int pos;    // index of the frame's position in d_position_b (a push) or d_tail (the flush)
	int owner;  // the frame's stream: its settings and its track
	int pad;
};
struct TmSet {  // a stream's settings at this call
	double w, wf, ra, rb;
	long long track_row;  // first row of the stream's track among the handle's track rows
	int m, pad;           // the track's rows
};
struct TmKeep {
	int row, slot;  // row of the push's packed arrays -> ring slot
};

struct TmArgs {
	const TmSet *sets;
	const TmFrame *frames;
	const TmKeep *keeps;
	long long total_out;
	int fs, fft_size;
	const double *f0_a, *sp_a, *ap_a;  // the push's packed rows of the live voice
	const double *pos;                 // d_position_b / d_tail
	const double *tf0, *tsp, *tap;     // the tracks
	double *rf0, *rsp, *rap;           // the ring: F0 and both rows per slot
	double *f0_out, *sp_out, *ap_out;
};

template <bool STRETCH>
__global__ __launch_bounds__(RT_T) void track_morph_kernel(TmArgs A) {
	const int tid = threadIdx.x;
	const long long g = blockIdx.x;
	const int bins = A.fft_size / 2 + 1;
	if (g >= A.total_out) {  // a row of the push goes to the ring
		const TmKeep k = A.keeps[g - A.total_out];
		if (tid == 0) A.rf0[k.slot] = A.f0_a[k.row];
		const long long from = (long long)k.row * bins, to = (long long)k.slot * bins;
		rt_row(A.sp_a + from, A.sp_a + from, 1.0, 0.0, A.rsp + to, bins, tid);
		rt_row(A.ap_a + from, A.ap_a + from, 1.0, 0.0, A.rap + to, bins, tid);
		return;
	}
	const TmFrame f = A.frames[g];
	const TmSet set = A.sets[f.owner];
	const RtPlace qb = rt_place(A.pos[f.pos], set.m);  // (qb.i, qb.j in [0, m - 1] whatever the position holds)
	const double w = set.w, w0 = 1.0 - w;
	const bool finite = qb.finite;  // (voice A's position is a frame index and the setter keeps the weight finite)
	// voice A at a whole position: rt_place gives a = 0, w0 = 1, j = i
	constexpr double aa = 0.0, wa0 = 1.0;
	const bool ring = f.row < 0;
	const long long ra_ = ring ? ~f.row : f.row;
	const long long ib = set.track_row + qb.i, jb = set.track_row + qb.j;

	if (tid == 0) {
		double v = __builtin_nan("");
		if (finite) {
			const double fa = (ring ? A.rf0 : A.f0_a)[ra_];
			v = mp_f0(rt_f0(fa, fa, wa0, aa), rt_f0(A.tf0[ib], A.tf0[jb], qb.w0, qb.a), set.wf);
		}
		A.f0_out[g] = v;
	}
	{
		double *__restrict__ out = A.ap_out + g * bins;
		const double *__restrict__ ai = (ring ? A.rap : A.ap_a) + ra_ * bins;
		const double *__restrict__ bi = A.tap + ib * bins, *__restrict__ bj = A.tap + jb * bins;
		if (!finite) rt_nan_row(out, bins, tid);
		else if (w == 0.0) rt_row(ai, ai, wa0, aa, out, bins, tid);
		else if (w == 1.0) rt_row(bi, bj, qb.w0, qb.a, out, bins, tid);
		else {
			for (int t = tid; t < bins / 2; t += RT_T) {
				const d2u x = rt_pair(ai, ai, wa0, aa, 2 * t), y = rt_pair(bi, bj, qb.w0, qb.a, 2 * t);
				*reinterpret_cast<d2u *>(out + 2 * t) = w0 * x + w * y;
			}
			if (tid == 0) out[bins - 1] = w0 * rt_one(ai, ai, wa0, aa, bins - 1) + w * rt_one(bi, bj, qb.w0, qb.a, bins - 1);
		}
	}
	double *__restrict__ out = A.sp_out + g * bins;
	const double *__restrict__ ai = (ring ? A.rsp : A.sp_a) + ra_ * bins;
	const double *__restrict__ bi = A.tsp + ib * bins, *__restrict__ bj = A.tsp + jb * bins;
	if (!finite) {
		rt_nan_row(out, bins, tid);
		return;
	}
	if constexpr (STRETCH) {
		__shared__ double lga[kMaxBins], lgb[kMaxBins];
		__shared__ double fill;
		const double ra = set.ra, rb = set.rb;  // 0 or valid: the setter refuses the others
		if (w == 0.0 || w == 1.0) {  // the one source's row as retime_kernel<true> writes it
			const bool first = w == 0.0;
			const double r = first ? ra : rb, a = first ? aa : qb.a, a0 = first ? wa0 : qb.w0;
			const double *__restrict__ ri = first ? ai : bi, *__restrict__ rj = first ? ai : bj;
			if (r == 0.0) rt_row(ri, rj, a0, a, out, bins, tid);
			else rt_stretched_row(ri, rj, a0, a, out, r, A.fs, A.fft_size, tid, lga, &fill);
			return;
		}
		rt_log_row(ai, ai, wa0, aa, lga, bins, tid);
		rt_log_row(bi, bj, qb.w0, qb.a, lgb, bins, tid);
		__syncthreads();
		const MpLog la = mp_log(lga, ra, A.fs, A.fft_size), lb = mp_log(lgb, rb, A.fs, A.fft_size);
		for (int b = tid; b < bins; b += RT_T) out[b] = exp(w0 * la.at(b) + w * lb.at(b));
	} else {
		if (w == 0.0) rt_row(ai, ai, wa0, aa, out, bins, tid);
		else if (w == 1.0) rt_row(bi, bj, qb.w0, qb.a, out, bins, tid);
		else {
			for (int t = tid; t < bins / 2; t += RT_T) {
				const d2u x = rt_pair(ai, ai, wa0, aa, 2 * t), y = rt_pair(bi, bj, qb.w0, qb.a, 2 * t);
				d2u v;
				v.x = exp(w0 * log(x.x) + w * log(y.x));
				v.y = exp(w0 * log(x.y) + w * log(y.y));
				*reinterpret_cast<d2u *>(out + 2 * t) = v;
			}
			if (tid == 0)
				out[bins - 1] = exp(w0 * log(rt_one(ai, ai, wa0, aa, bins - 1)) + w * log(rt_one(bi, bj, qb.w0, qb.a, bins - 1)));
		}
	}
}

// ---- the host half: the rule of the header ----
struct TmState {
	int track = -1;      // -1: never reset onto a track
	int delay = 0;
	bool ended = false;  // flushed: rows are refused until the next reset
	long long n = 0;     // rows of the live voice received
	long long seq = 0;   // sequence number of row keep(): row r >= keep sits in slot (seq + r - keep) % cap
	double w = 0.0, wf = 0.0, ra = 0.0, rb = 0.0;
	long long keep() const { return ended ? n : std::max(n - delay, 0ll); }  // frames formed = the first row still waiting
};

}  // namespace

struct wc_track_morph {
	int fs, fft_size, n_streams, n_tracks, max_m, max_frames, max_delay, cap;  // cap: ring slots per stream
	Device *dev;
	std::vector<TmState> st, next;  // next: the states a call plans, kept if it succeeds
	std::vector<int> track_m, cnt;
	DevBuf tf0, tsp, tap;  // the tracks: n_tracks x max_track_frames rows
	DevBuf rf0, rsp, rap;  // the ring: n_streams x cap slots
	DevBuf drec;           // the records of a call
	HostBuf h_rec[2];      // their page-locked staging: a pair, so that a call waits for the copy of the call before the last only
	int parity = 0;
	size_t frames_cap() const { return (size_t)n_streams * std::max(max_frames, max_delay); }
	size_t keeps_cap() const { return (size_t)n_streams * std::min(max_delay, max_frames); }
	// the records of a call, in the staging and on the device: the settings of every stream | the frames | the rows to keep
	size_t rec_bytes() const { return sizeof(TmSet) * n_streams + sizeof(TmFrame) * frames_cap() + sizeof(TmKeep) * keeps_cap(); }
};

namespace {

bool tm_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }
bool tm_stream_ok(const wc_track_morph *h, int u) { return h && u >= 0 && u < h->n_streams; }
bool tm_track_ok(const wc_track_morph *h, int t) { return h && t >= 0 && t < h->n_tracks; }

void tm_set(const wc_track_morph *h, const TmState &q, TmSet &s) {
	s.w = q.w; s.wf = q.wf; s.ra = q.ra; s.rb = q.rb;
	s.track_row = q.track < 0 ? 0 : (long long)q.track * h->max_m;
	s.m = q.track < 0 ? 1 : h->track_m[q.track];
	s.pad = 0;
}

// the records are planned in h_rec[parity] and h->next; copy, launch, and the plan becomes the state
int tm_enqueue(wc_track_morph *h, long long total_out, long long n_keep, bool stretch, const double *d_f0_a, const double *d_sp_a,
			   const double *d_ap_a, const double *d_pos, double *d_f0_out, double *d_sp_out, double *d_ap_out) {
	const int n = h->n_streams;
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	TmSet *set = h->h_rec[h->parity].as<TmSet>();
	TmFrame *fr = reinterpret_cast<TmFrame *>(set + n);
	TmKeep *kp = reinterpret_cast<TmKeep *>(fr + h->frames_cap());
	// the keep records follow the frame records of this call in the staging and on the device
	std::memmove(fr + total_out, kp, sizeof(TmKeep) * (size_t)n_keep);
	const size_t bytes = sizeof(TmSet) * (size_t)n + sizeof(TmFrame) * (size_t)total_out + sizeof(TmKeep) * (size_t)n_keep;
	WC_HIP(hipMemcpyAsync(h->drec.p, set, bytes, hipMemcpyHostToDevice, hs));
	int rc;
	if ((rc = h->h_rec[h->parity].mark(hs))) return rc;
	TmArgs a;
	a.sets = h->drec.as<TmSet>();
	a.frames = reinterpret_cast<const TmFrame *>(a.sets + n);
	a.keeps = reinterpret_cast<const TmKeep *>(a.frames + total_out);
	a.total_out = total_out; a.fs = h->fs; a.fft_size = h->fft_size;
	a.f0_a = d_f0_a; a.sp_a = d_sp_a; a.ap_a = d_ap_a; a.pos = d_pos;
	a.tf0 = h->tf0.as<double>(); a.tsp = h->tsp.as<double>(); a.tap = h->tap.as<double>();
	a.rf0 = h->rf0.as<double>(); a.rsp = h->rsp.as<double>(); a.rap = h->rap.as<double>();
	a.f0_out = d_f0_out; a.sp_out = d_sp_out; a.ap_out = d_ap_out;
	if ((rc = h->dev->time_begin("track_morph_kernel", hs))) return rc;
	const dim3 grid((unsigned)(total_out + n_keep));
	if (stretch) hipLaunchKernelGGL(track_morph_kernel<true>, grid, dim3(RT_T), 0, hs, a);
	else hipLaunchKernelGGL(track_morph_kernel<false>, grid, dim3(RT_T), 0, hs, a);
	WC_HIP(hipGetLastError());
	if ((rc = h->dev->time_end("track_morph_kernel", hs))) return rc;
	h->st.swap(h->next);
	h->parity = 1 - h->parity;
	return WC_OK;
}

}  // namespace

extern "C" {

wc_track_morph *wc_track_morph_create(int fs, int fft_size, int n_streams, int n_tracks, int max_track_frames, int max_frames_per_push,
									  int max_delay) {
	if (!fft_size_supported(fft_size)) { set_error("track morph: fft_size must be 512, 1024, 2048 or 4096"); return nullptr; }
	if (fs <= 0) { set_error("track morph: fs must be positive"); return nullptr; }
	if (n_streams < 1 || n_tracks < 1 || max_track_frames < 1 || max_frames_per_push < 1) {
		set_error("track morph: n_streams, n_tracks, max_track_frames and max_frames_per_push must be at least 1");
		return nullptr;
	}
	if (max_delay < 0) { set_error("track morph: max_delay must not be negative"); return nullptr; }
	// (row and slot numbers are ints in the records)
	const long long cap = (long long)max_delay + std::min(max_delay, max_frames_per_push);
	if ((long long)n_streams * std::max(max_frames_per_push, max_delay) > 0x7fffffffll || (long long)n_streams * cap > 0x7fffffffll ||
		(long long)n_tracks * max_track_frames > 0x7fffffffll) {
		set_error("track morph: n_streams x max_frames_per_push, n_streams x ring slots or n_tracks x max_track_frames too large");
		return nullptr;
	}
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	wc_track_morph *h = new wc_track_morph();
	h->fs = fs; h->fft_size = fft_size; h->n_streams = n_streams; h->n_tracks = n_tracks; h->max_m = max_track_frames;
	h->max_frames = max_frames_per_push; h->max_delay = max_delay; h->cap = (int)cap;
	h->dev = dev;
	h->st.assign(n_streams, TmState());
	h->next.reserve(n_streams);
	h->track_m.assign(n_tracks, 0);
	h->cnt.assign(n_streams, 0);
	const size_t bins = fft_size / 2 + 1, rows = (size_t)n_tracks * max_track_frames, slots = (size_t)n_streams * (size_t)cap;
	const size_t rec = h->rec_bytes();
	if (h->tf0.reserve(sizeof(double) * rows) || h->tsp.reserve(sizeof(double) * rows * bins) || h->tap.reserve(sizeof(double) * rows * bins) ||
		(slots > 0 && (h->rf0.reserve(sizeof(double) * slots) || h->rsp.reserve(sizeof(double) * slots * bins) || h->rap.reserve(sizeof(double) * slots * bins))) ||
		h->drec.reserve(rec) || h->h_rec[0].reserve(rec) || h->h_rec[1].reserve(rec)) {
		wc_track_morph_destroy(h);
		return nullptr;
	}
	return h;
}

void wc_track_morph_destroy(wc_track_morph *h) {
	if (!h) return;
	h->dev->quiesce();
	h->tf0.release(); h->tsp.release(); h->tap.release(); h->rf0.release(); h->rsp.release(); h->rap.release();
	h->drec.release(); h->h_rec[0].release(); h->h_rec[1].release();
	delete h;
}

int wc_track_morph_set_track_device(wc_track_morph *h, int track, int m, const double *d_f0_b, const double *d_sp_b, const double *d_ap_b) {
	if (!tm_track_ok(h, track)) return fail(WC_ERR_INVALID, "track morph: bad track index");
	if (m < 1 || m > h->max_m) return fail(WC_ERR_INVALID, "track morph set_track: need 1 <= m <= max_track_frames");
	if (!d_f0_b || !d_sp_b || !d_ap_b) return fail(WC_ERR_INVALID, "track morph set_track: null rows");
	DeviceLock lock(h->dev);
	for (const auto &s : h->st)
		if (s.track == track && s.n > 0)
			return fail(WC_ERR_INVALID, "track morph set_track: a stream that has received rows is attached to this track (reset it first)");
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	const size_t bins = h->fft_size / 2 + 1, first = (size_t)track * h->max_m;
	WC_HIP(hipMemcpyAsync(h->tf0.as<double>() + first, d_f0_b, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, hs));
	WC_HIP(hipMemcpyAsync(h->tsp.as<double>() + first * bins, d_sp_b, sizeof(double) * (size_t)m * bins, hipMemcpyDeviceToDevice, hs));
	WC_HIP(hipMemcpyAsync(h->tap.as<double>() + first * bins, d_ap_b, sizeof(double) * (size_t)m * bins, hipMemcpyDeviceToDevice, hs));
	h->track_m[track] = m;
	return WC_OK;
}

int wc_track_morph_reset(wc_track_morph *h, int stream, int track, int delay) {
	if (!tm_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "track morph: bad stream index");
	if (!tm_track_ok(h, track)) return fail(WC_ERR_INVALID, "track morph: bad track index");
	if (delay < 0 || delay > h->max_delay) return fail(WC_ERR_INVALID, "track morph reset: need 0 <= delay <= max_delay");
	DeviceLock lock(h->dev);
	if (h->track_m[track] == 0) return fail(WC_ERR_INVALID, "track morph reset: the track has not been set");
	TmState &s = h->st[stream];
	s = TmState();  // (no row is held across a reset: the numbering may start again)
	s.track = track;
	s.delay = delay;
	return WC_OK;
}

int wc_track_morph_set_weight(wc_track_morph *h, int stream, double weight, double f0_weight) {
	if (!tm_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "track morph: bad stream index");
	if (!(tm_finite(weight) && tm_finite(f0_weight))) return fail(WC_ERR_INVALID, "track morph: the weight and the F0 weight must be finite");
	DeviceLock lock(h->dev);
	h->st[stream].w = weight;
	h->st[stream].wf = f0_weight;
	return WC_OK;
}

int wc_track_morph_set_ratios(wc_track_morph *h, int stream, double ratio_a, double ratio_b) {
	if (!tm_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "track morph: bad stream index");
	if (!((ratio_a == 0.0 || frame_ratio_valid(ratio_a, h->fft_size)) && (ratio_b == 0.0 || frame_ratio_valid(ratio_b, h->fft_size))))
		return fail(WC_ERR_INVALID, "track morph: a ratio must be 0 (none) or finite and >= 2.0 / fft_size");
	DeviceLock lock(h->dev);
	h->st[stream].ra = ratio_a;
	h->st[stream].rb = ratio_b;
	return WC_OK;
}

int wc_track_morph_push_device(wc_track_morph *h, const int *n_a, const double *d_f0_a, const double *d_sp_a, const double *d_ap_a,
							   const double *d_position_b, double *d_f0_out, double *d_sp_out, double *d_ap_out, int *frames_out) {
	if (!h || !n_a || !frames_out) return fail(WC_ERR_INVALID, "track morph push: null argument");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	long long in = 0;
	for (int u = 0; u < n; ++u) {
		if (n_a[u] < 0) return fail(WC_ERR_INVALID, "track morph push: negative row count");
		if (n_a[u] > h->max_frames) return fail(WC_ERR_INVALID, "track morph push: more than max_frames_per_push rows for one stream");
		if (n_a[u] > 0 && h->st[u].track < 0) return fail(WC_ERR_INVALID, "track morph push: rows for a stream that was never reset onto a track");
		if (n_a[u] > 0 && h->st[u].ended) return fail(WC_ERR_INVALID, "track morph push: rows for a stream that has ended (reset it first)");
		in += n_a[u];
	}
	if (in > 0 && !(d_f0_a && d_sp_a && d_ap_a)) return fail(WC_ERR_INVALID, "track morph push: null input array");
	// ---- the plan: host arithmetic on counts, every refusal in front of the first enqueue ----
	if (h->h_rec[h->parity].reserve(0)) return WC_ERR_DEVICE;  // (the copy of the call before the last has read this staging)
	TmSet *set = h->h_rec[h->parity].as<TmSet>();
	TmFrame *fr = reinterpret_cast<TmFrame *>(set + n);
	TmKeep *kp = reinterpret_cast<TmKeep *>(fr + h->frames_cap());  // (moved up behind the frames once their number is known)
	h->next = h->st;
	long long total_out = 0, n_keep = 0, off = 0;
	bool stretch = false;
	for (int u = 0; u < n; ++u) {
		const TmState &old = h->st[u];
		TmState &q = h->next[u];
		tm_set(h, q, set[u]);
		const int c_in = n_a[u];
		if (c_in == 0) { h->cnt[u] = 0; continue; }
		q.n = old.n + c_in;
		const long long keep_old = old.keep(), keep_new = q.keep(), base = (long long)u * h->cap;
		const int c = (int)(keep_new - keep_old);  // frames keep_old .. keep_new - 1: <= c_in <= max_frames_per_push
		for (int k = 0; k < c; ++k) {
			const long long t = keep_old + k;
			TmFrame &f = fr[total_out + k];
			// row t of the voice: a row of this push, or the slot the state before the push holds it in (t - keep_old < delay <= cap)
			f.row = t >= old.n ? (int)(off + (t - old.n)) : ~(int)(base + (old.seq + (t - keep_old)) % h->cap);
			f.pos = (int)(off + (t + q.delay - old.n));  // the entry of row t + delay, which is a row of this push
			f.owner = u; f.pad = 0;
		}
		if (c > 0 && (q.ra != 0.0 || q.rb != 0.0)) stretch = true;
		const long long fresh = old.seq + (old.n - keep_old);  // the next unused number
		q.seq = keep_new < old.n ? old.seq + (keep_new - keep_old) : fresh;
		for (long long r = std::max(keep_new, old.n); r < q.n; ++r) {
			TmKeep &k = kp[n_keep++];
			k.row = (int)(off + (r - old.n));
			k.slot = (int)(base + (q.seq + (r - keep_new)) % h->cap);
		}
		off += c_in;
		h->cnt[u] = c;
		total_out += c;
	}
	if (total_out > 0 && !(d_position_b && d_f0_out && d_sp_out && d_ap_out)) return fail(WC_ERR_INVALID, "track morph push: null position or output array");
	std::copy(h->cnt.begin(), h->cnt.end(), frames_out);  // (no refusal is left)
	if (total_out + n_keep == 0) { h->st.swap(h->next); return WC_OK; }
	return tm_enqueue(h, total_out, n_keep, stretch, d_f0_a, d_sp_a, d_ap_a, d_position_b, d_f0_out, d_sp_out, d_ap_out);
}

int wc_track_morph_flush_device(wc_track_morph *h, const int *want, const double *d_tail, double *d_f0_out, double *d_sp_out,
								double *d_ap_out, int *frames_out) {
	if (!h || !want || !frames_out) return fail(WC_ERR_INVALID, "track morph flush: null argument");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	for (int u = 0; u < n; ++u) {
		if (!want[u]) continue;
		const TmState &s = h->st[u];
		if (s.track < 0 || s.ended) return fail(WC_ERR_INVALID, "track morph flush: a wanted stream is not attached or has ended");
		if (s.delay == 0 || s.n == 0) return fail(WC_ERR_INVALID, "track morph flush: a wanted stream has no delay or no rows");
	}
	if (h->h_rec[h->parity].reserve(0)) return WC_ERR_DEVICE;
	TmSet *set = h->h_rec[h->parity].as<TmSet>();
	TmFrame *fr = reinterpret_cast<TmFrame *>(set + n);
	h->next = h->st;
	long long total_out = 0, toff = 0;
	bool stretch = false;
	for (int u = 0; u < n; ++u) {
		TmState &q = h->next[u];
		tm_set(h, q, set[u]);
		h->cnt[u] = 0;
		if (!want[u]) continue;
		const long long keep = q.keep(), base = (long long)u * h->cap;
		const int c = (int)(q.n - keep);                          // min(delay, n) rows wait
		const int K = (int)std::min<long long>(q.delay + 1, q.n);  // the stream's entries of d_tail: K - c in front belong to formed frames
		for (int k = 0; k < c; ++k) {
			TmFrame &f = fr[total_out + k];
			f.row = ~(int)(base + (q.seq + k) % h->cap);
			f.pos = (int)(toff + (K - c) + k);
			f.owner = u; f.pad = 0;
		}
		if (q.ra != 0.0 || q.rb != 0.0) stretch = true;
		q.seq += c;
		q.ended = true;
		toff += K;
		h->cnt[u] = c;
		total_out += c;
	}
	if (total_out > 0 && !(d_tail && d_f0_out && d_sp_out && d_ap_out)) return fail(WC_ERR_INVALID, "track morph flush: null tail or output array");
	std::copy(h->cnt.begin(), h->cnt.end(), frames_out);
	if (total_out == 0) return WC_OK;
	return tm_enqueue(h, total_out, 0, stretch, nullptr, nullptr, nullptr, d_tail, d_f0_out, d_sp_out, d_ap_out);
}

long long wc_track_morph_frames_received(const wc_track_morph *h, int stream) {
	if (!tm_stream_ok(h, stream)) return -1;
	return h->st[stream].n;
}

long long wc_track_morph_frames_formed(const wc_track_morph *h, int stream) {
	if (!tm_stream_ok(h, stream)) return -1;
	return h->st[stream].keep();
}

int wc_track_morph_pending(const wc_track_morph *h, int stream) {
	if (!tm_stream_ok(h, stream)) return WC_ERR_INVALID;
	return (int)(h->st[stream].n - h->st[stream].keep());
}

int wc_track_morph_get_delay(const wc_track_morph *h, int stream) {
	if (!tm_stream_ok(h, stream)) return -1;
	return h->st[stream].delay;
}

int wc_track_morph_track_length(const wc_track_morph *h, int track) {
	if (!tm_track_ok(h, track)) return -1;
	return h->track_m[track];
}

}  // extern "C"
