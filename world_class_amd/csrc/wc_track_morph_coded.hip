// Coded track-morph streams (include/world_class_track_morph_coded.h: wc_track_morph_coded): wc_track_morph (wc_track_morph.hip) with
// its tracks, its ring and its live rows held as coded features -- number_of_dimensions + GetNumberOfAperiodicities(fs) doubles per
// row instead of 2 x (fft_size/2 + 1).  The rule, the ring's numbering, the refusals and the records are that file's, restated here
// so that it compiles to what it compiled to; the outputs are full rows with the bits of that handle on the decoded rows.
//
//   track_gather_coded_kernel   one wavefront per formed frame g or kept row.  For a frame it reads the frame's position itself (one
//     double of d_position_b or d_tail at an index the host wrote, the same for every lane), places it in the track with rt_place --
//     qb.i, qb.j lie in [0, m - 1] whatever the double holds -- and copies three coded rows, sp and ap part, into the handle's
//     scratch: A's row (a row of the push's packed arrays or a ring slot) to slot 3g, track rows i and j to slots 3g + 1 and 3g + 2.
//     For a kept row (TcKeep) it copies the coded row and its F0 into a ring slot that no workgroup of the call reads.  Coded rows
//     are 8-byte aligned only (nd may be odd, n_ap is 1, 3 or 5): every access is one double.
//
//   wc::decode_features_enqueue (wc_synth_coded.hip), unchanged, over the 3 x frames scratch slots: the one-wavefront kernel at
//     fft 2048, the codec's two workgroup kernels at the other sizes.
//
//   track_morph_coded_kernel<STRETCH>   track_morph_kernel's launch shape and blend, statement by statement, on the decoded slots:
//     A's row is slot 3g, B's rows are slots 3g + 1 and 3g + 2, the weights come from rt_place on the same double, its `finite`
//     gives the frame that is NaN throughout; F0 comes from the push or the ring for A and from the resident track's F0 for B.
//     STRETCH = false: no LDS; chosen by the host when no stream that forms frames in the call has a ratio.
//
//   A push is host arithmetic on counts (the rule, every refusal), one asynchronous copy of the settings, frame and keep records out
//   of page-locked staging, and the three enqueues (the gather alone when the push only keeps rows).  No host code looks at a position.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/world_class_track_morph_coded.h"
#include "wc_morph_rows.hpp"
#include "wc_retime_rows.hpp"
#include "wc_stages.hpp"

using namespace wc;

namespace {

constexpr int TC_W = 64;  // the gather's workgroup: one wavefront

struct TcFrame {
	int row;    // voice A's row: >= 0 a row of the push's packed arrays, < 0 the ring slot ~row (counted over the whole handle)
	int pos;    // index of the frame's position in d_position_b (a push) or d_tail (the flush)
	int owner;  // the frame's stream: its settings and its track
	int pad;
};
struct TcSet {  // a stream's settings at this call
	double w, wf, ra, rb;
	long long track_row;  // first row of the stream's track among the handle's track rows
	int m, pad;           // the track's rows
};
struct TcKeep {
	int row, slot;  // row of the push's packed arrays -> ring slot
};

struct TcArgs {
	const TcSet *sets;
	const TcFrame *frames;
	const TcKeep *keeps;
	long long total_out;
	int fs, fft_size, nd, n_ap;
	const double *f0_a, *csp_a, *cap_a;  // the push's packed coded rows of the live voice
	const double *pos;                   // d_position_b / d_tail
	const double *tf0, *tcsp, *tcap;     // the tracks
	double *rf0, *rcsp, *rcap;           // the ring: F0 and both coded rows per slot
	double *scsp, *scap;                 // the scratch: three coded rows per formed frame ...
	double *ssp, *sap;                   // ... and what the decoder makes of them
	double *f0_out, *sp_out, *ap_out;
};

__device__ __forceinline__ void tc_copy(const double *__restrict__ from, double *__restrict__ to, int n, int lane) {
	for (int c = lane; c < n; c += TC_W) to[c] = from[c];
}

__global__ __launch_bounds__(TC_W) void track_gather_coded_kernel(TcArgs A) {
	const int lane = threadIdx.x;
	const long long g = blockIdx.x;
	const int nd = A.nd, n_ap = A.n_ap;
	if (g >= A.total_out) {  // a row of the push goes to the ring
		const TcKeep k = A.keeps[g - A.total_out];
		if (lane == 0) A.rf0[k.slot] = A.f0_a[k.row];
		tc_copy(A.csp_a + (long long)k.row * nd, A.rcsp + (long long)k.slot * nd, nd, lane);
		tc_copy(A.cap_a + (long long)k.row * n_ap, A.rcap + (long long)k.slot * n_ap, n_ap, lane);
		return;
	}
	const TcFrame f = A.frames[g];
	const TcSet set = A.sets[f.owner];
	const RtPlace qb = rt_place(A.pos[f.pos], set.m);  // (qb.i, qb.j in [0, m - 1] whatever the position holds)
	const bool ring = f.row < 0;
	const long long ra_ = ring ? ~f.row : f.row;
	const long long ib = set.track_row + qb.i, jb = set.track_row + qb.j;
	tc_copy((ring ? A.rcsp : A.csp_a) + ra_ * nd, A.scsp + (3 * g) * nd, nd, lane);
	tc_copy(A.tcsp + ib * nd, A.scsp + (3 * g + 1) * nd, nd, lane);
	tc_copy(A.tcsp + jb * nd, A.scsp + (3 * g + 2) * nd, nd, lane);
	tc_copy((ring ? A.rcap : A.cap_a) + ra_ * n_ap, A.scap + (3 * g) * n_ap, n_ap, lane);
	tc_copy(A.tcap + ib * n_ap, A.scap + (3 * g + 1) * n_ap, n_ap, lane);
	tc_copy(A.tcap + jb * n_ap, A.scap + (3 * g + 2) * n_ap, n_ap, lane);
}

template <bool STRETCH>
__global__ __launch_bounds__(RT_T) void track_morph_coded_kernel(TcArgs A) {
	const int tid = threadIdx.x;
	const long long g = blockIdx.x;
	const int bins = A.fft_size / 2 + 1;
	const TcFrame f = A.frames[g];
	const TcSet set = A.sets[f.owner];
	const RtPlace qb = rt_place(A.pos[f.pos], set.m);  // the gather's placement: the same double, the same m
	const double w = set.w, w0 = 1.0 - w;
	const bool finite = qb.finite;  // (voice A's position is a frame index and the setter keeps the weight finite)
	// voice A at a whole position: rt_place gives a = 0, w0 = 1, j = i
	constexpr double aa = 0.0, wa0 = 1.0;
	const bool ring = f.row < 0;
	const long long ra_ = ring ? ~f.row : f.row;
	const long long ib = set.track_row + qb.i, jb = set.track_row + qb.j;
	const long long sa = 3 * g * bins, si = sa + bins, sj = si + bins;  // the frame's three decoded slots

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
		const double *__restrict__ ai = A.sap + sa;
		const double *__restrict__ bi = A.sap + si, *__restrict__ bj = A.sap + sj;
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
	const double *__restrict__ ai = A.ssp + sa;
	const double *__restrict__ bi = A.ssp + si, *__restrict__ bj = A.ssp + sj;
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

// ---- the host half: the rule of the header (wc_track_morph.hip's plan) ----
struct TcState {
	int track = -1;      // -1: never reset onto a track
	int delay = 0;
	bool ended = false;  // flushed: rows are refused until the next reset
	long long n = 0;     // rows of the live voice received
	long long seq = 0;   // sequence number of row keep(): row r >= keep sits in slot (seq + r - keep) % cap
	double w = 0.0, wf = 0.0, ra = 0.0, rb = 0.0;
	long long keep() const { return ended ? n : std::max(n - delay, 0ll); }  // frames formed = the first row still waiting
};

}  // namespace

struct wc_track_morph_coded {
	int fs, fft_size, nd, n_ap, n_streams, n_tracks, max_m, max_frames, max_delay, cap;  // cap: ring slots per stream
	Device *dev;
	std::vector<TcState> st, next;  // next: the states a call plans, kept if it succeeds
	std::vector<int> track_m, cnt;
	DevBuf tf0, tcsp, tcap;          // the tracks: n_tracks x max_track_frames coded rows
	DevBuf rf0, rcsp, rcap;          // the ring: n_streams x cap slots
	DevBuf scsp, scap, ssp, sap;     // the scratch: 3 x frames_cap() slots, coded and decoded
	DevBuf drec;                     // the records of a call
	HostBuf h_rec[2];                // their page-locked staging: a pair, so that a call waits for the copy of the call before the last only
	int parity = 0;
	long long device_bytes = 0;
	size_t frames_cap() const { return (size_t)n_streams * std::max(max_frames, max_delay); }
	size_t keeps_cap() const { return (size_t)n_streams * std::min(max_delay, max_frames); }
	// the records of a call, in the staging and on the device: the settings of every stream | the frames | the rows to keep
	size_t rec_bytes() const { return sizeof(TcSet) * n_streams + sizeof(TcFrame) * frames_cap() + sizeof(TcKeep) * keeps_cap(); }
};

namespace {

bool tc_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }
bool tc_stream_ok(const wc_track_morph_coded *h, int u) { return h && u >= 0 && u < h->n_streams; }
bool tc_track_ok(const wc_track_morph_coded *h, int t) { return h && t >= 0 && t < h->n_tracks; }

// create allocates every array once and exactly (rounded up to 256 bytes): DevBuf::reserve's head-room is for buffers that grow
int tc_alloc(wc_track_morph_coded *h, DevBuf &b, size_t bytes) {
	if (bytes == 0) return WC_OK;
	const size_t want = (bytes + 255) / 256 * 256;
	WC_HIP(hipMalloc(&b.p, want));
	b.cap = want;
	h->device_bytes += (long long)want;
	return WC_OK;
}

void tc_set(const wc_track_morph_coded *h, const TcState &q, TcSet &s) {
	s.w = q.w; s.wf = q.wf; s.ra = q.ra; s.rb = q.rb;
	s.track_row = q.track < 0 ? 0 : (long long)q.track * h->max_m;
	s.m = q.track < 0 ? 1 : h->track_m[q.track];
	s.pad = 0;
}

// the records are planned in h_rec[parity] and h->next; copy, gather, decode, blend, and the plan becomes the state
int tc_enqueue(wc_track_morph_coded *h, long long total_out, long long n_keep, bool stretch, const double *d_f0_a, const double *d_csp_a,
			   const double *d_cap_a, const double *d_pos, double *d_f0_out, double *d_sp_out, double *d_ap_out) {
	const int n = h->n_streams;
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	TcSet *set = h->h_rec[h->parity].as<TcSet>();
	TcFrame *fr = reinterpret_cast<TcFrame *>(set + n);
	TcKeep *kp = reinterpret_cast<TcKeep *>(fr + h->frames_cap());
	// the keep records follow the frame records of this call in the staging and on the device
	std::memmove(fr + total_out, kp, sizeof(TcKeep) * (size_t)n_keep);
	const size_t bytes = sizeof(TcSet) * (size_t)n + sizeof(TcFrame) * (size_t)total_out + sizeof(TcKeep) * (size_t)n_keep;
	WC_HIP(hipMemcpyAsync(h->drec.p, set, bytes, hipMemcpyHostToDevice, hs));
	int rc;
	if ((rc = h->h_rec[h->parity].mark(hs))) return rc;
	TcArgs a;
	a.sets = h->drec.as<TcSet>();
	a.frames = reinterpret_cast<const TcFrame *>(a.sets + n);
	a.keeps = reinterpret_cast<const TcKeep *>(a.frames + total_out);
	a.total_out = total_out; a.fs = h->fs; a.fft_size = h->fft_size; a.nd = h->nd; a.n_ap = h->n_ap;
	a.f0_a = d_f0_a; a.csp_a = d_csp_a; a.cap_a = d_cap_a; a.pos = d_pos;
	a.tf0 = h->tf0.as<double>(); a.tcsp = h->tcsp.as<double>(); a.tcap = h->tcap.as<double>();
	a.rf0 = h->rf0.as<double>(); a.rcsp = h->rcsp.as<double>(); a.rcap = h->rcap.as<double>();
	a.scsp = h->scsp.as<double>(); a.scap = h->scap.as<double>(); a.ssp = h->ssp.as<double>(); a.sap = h->sap.as<double>();
	a.f0_out = d_f0_out; a.sp_out = d_sp_out; a.ap_out = d_ap_out;
	if ((rc = h->dev->time_begin("track_gather_coded_kernel", hs))) return rc;
	hipLaunchKernelGGL(track_gather_coded_kernel, dim3((unsigned)(total_out + n_keep)), dim3(TC_W), 0, hs, a);
	WC_HIP(hipGetLastError());
	if ((rc = h->dev->time_end("track_gather_coded_kernel", hs))) return rc;
	if (total_out > 0) {
		if ((rc = h->dev->time_begin("track_morph_coded_decode", hs))) return rc;
		if ((rc = decode_features_enqueue(h->dev, hs, h->fs, h->fft_size, 3 * total_out, h->nd, a.scsp, a.scap, nullptr, a.ssp, a.sap))) return rc;
		if ((rc = h->dev->time_end("track_morph_coded_decode", hs))) return rc;
		if ((rc = h->dev->time_begin("track_morph_coded_kernel", hs))) return rc;
		const dim3 grid((unsigned)total_out);
		if (stretch) hipLaunchKernelGGL(track_morph_coded_kernel<true>, grid, dim3(RT_T), 0, hs, a);
		else hipLaunchKernelGGL(track_morph_coded_kernel<false>, grid, dim3(RT_T), 0, hs, a);
		WC_HIP(hipGetLastError());
		if ((rc = h->dev->time_end("track_morph_coded_kernel", hs))) return rc;
	}
	h->st.swap(h->next);
	h->parity = 1 - h->parity;
	return WC_OK;
}

}  // namespace

extern "C" {

wc_track_morph_coded *wc_track_morph_coded_create(int fs, int fft_size, int number_of_dimensions, int n_streams, int n_tracks,
												  int max_track_frames, int max_frames_per_push, int max_delay) {
	if (!fft_size_supported(fft_size)) { set_error("coded track morph: fft_size must be 512, 1024, 2048 or 4096"); return nullptr; }
	if (fs <= 0) { set_error("coded track morph: fs must be positive"); return nullptr; }
	if (n_streams < 1 || n_tracks < 1 || max_track_frames < 1 || max_frames_per_push < 1) {
		set_error("coded track morph: n_streams, n_tracks, max_track_frames and max_frames_per_push must be at least 1");
		return nullptr;
	}
	if (max_delay < 0) { set_error("coded track morph: max_delay must not be negative"); return nullptr; }
	if (const char *why = decode_features_check(fs, fft_size, number_of_dimensions)) { set_error(std::string("coded track morph: ") + why); return nullptr; }
	// (row and slot numbers are ints in the records, and the decoder's grid is the three scratch slots of every frame)
	const long long cap = (long long)max_delay + std::min(max_delay, max_frames_per_push);
	if (3ll * n_streams * std::max(max_frames_per_push, max_delay) > 0x7fffffffll || (long long)n_streams * cap > 0x7fffffffll ||
		(long long)n_tracks * max_track_frames > 0x7fffffffll) {
		set_error("coded track morph: 3 x n_streams x max_frames_per_push, n_streams x ring slots or n_tracks x max_track_frames too large");
		return nullptr;
	}
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	const CodecPlan *pl;
	if (codec_plan(dev, fs, fft_size, false, &pl)) return nullptr;  // (built here: no push is the first use, which may wait for the device)
	wc_track_morph_coded *h = new wc_track_morph_coded();
	h->fs = fs; h->fft_size = fft_size; h->nd = number_of_dimensions; h->n_ap = GetNumberOfAperiodicities(fs);
	h->n_streams = n_streams; h->n_tracks = n_tracks; h->max_m = max_track_frames;
	h->max_frames = max_frames_per_push; h->max_delay = max_delay; h->cap = (int)cap;
	h->dev = dev;
	h->st.assign(n_streams, TcState());
	h->next.reserve(n_streams);
	h->track_m.assign(n_tracks, 0);
	h->cnt.assign(n_streams, 0);
	const size_t bins = fft_size / 2 + 1, rows = (size_t)n_tracks * max_track_frames, slots = (size_t)n_streams * (size_t)cap;
	const size_t nd = h->nd, n_ap = h->n_ap, scr = 3 * h->frames_cap(), d = sizeof(double);
	const size_t rec = h->rec_bytes();
	if (hipSetDevice(dev->id) != hipSuccess || tc_alloc(h, h->tf0, d * rows) || tc_alloc(h, h->tcsp, d * rows * nd) || tc_alloc(h, h->tcap, d * rows * n_ap) ||
		tc_alloc(h, h->rf0, d * slots) || tc_alloc(h, h->rcsp, d * slots * nd) || tc_alloc(h, h->rcap, d * slots * n_ap) ||
		tc_alloc(h, h->scsp, d * scr * nd) || tc_alloc(h, h->scap, d * scr * n_ap) || tc_alloc(h, h->ssp, d * scr * bins) ||
		tc_alloc(h, h->sap, d * scr * bins) || tc_alloc(h, h->drec, rec) || h->h_rec[0].reserve(rec) || h->h_rec[1].reserve(rec)) {
		wc_track_morph_coded_destroy(h);
		return nullptr;
	}
	return h;
}

void wc_track_morph_coded_destroy(wc_track_morph_coded *h) {
	if (!h) return;
	h->dev->quiesce();
	h->tf0.release(); h->tcsp.release(); h->tcap.release(); h->rf0.release(); h->rcsp.release(); h->rcap.release();
	h->scsp.release(); h->scap.release(); h->ssp.release(); h->sap.release();
	h->drec.release(); h->h_rec[0].release(); h->h_rec[1].release();
	delete h;
}

int wc_track_morph_coded_set_track_device(wc_track_morph_coded *h, int track, int m, const double *d_f0_b, const double *d_coded_sp_b,
										  const double *d_coded_ap_b) {
	if (!tc_track_ok(h, track)) return fail(WC_ERR_INVALID, "coded track morph: bad track index");
	if (m < 1 || m > h->max_m) return fail(WC_ERR_INVALID, "coded track morph set_track: need 1 <= m <= max_track_frames");
	if (!d_f0_b || !d_coded_sp_b || !d_coded_ap_b) return fail(WC_ERR_INVALID, "coded track morph set_track: null rows");
	DeviceLock lock(h->dev);
	for (const auto &s : h->st)
		if (s.track == track && s.n > 0)
			return fail(WC_ERR_INVALID, "coded track morph set_track: a stream that has received rows is attached to this track (reset it first)");
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	const size_t nd = h->nd, n_ap = h->n_ap, first = (size_t)track * h->max_m;
	WC_HIP(hipMemcpyAsync(h->tf0.as<double>() + first, d_f0_b, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, hs));
	WC_HIP(hipMemcpyAsync(h->tcsp.as<double>() + first * nd, d_coded_sp_b, sizeof(double) * (size_t)m * nd, hipMemcpyDeviceToDevice, hs));
	WC_HIP(hipMemcpyAsync(h->tcap.as<double>() + first * n_ap, d_coded_ap_b, sizeof(double) * (size_t)m * n_ap, hipMemcpyDeviceToDevice, hs));
	h->track_m[track] = m;
	return WC_OK;
}

int wc_track_morph_coded_reset(wc_track_morph_coded *h, int stream, int track, int delay) {
	if (!tc_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "coded track morph: bad stream index");
	if (!tc_track_ok(h, track)) return fail(WC_ERR_INVALID, "coded track morph: bad track index");
	if (delay < 0 || delay > h->max_delay) return fail(WC_ERR_INVALID, "coded track morph reset: need 0 <= delay <= max_delay");
	DeviceLock lock(h->dev);
	if (h->track_m[track] == 0) return fail(WC_ERR_INVALID, "coded track morph reset: the track has not been set");
	TcState &s = h->st[stream];
	s = TcState();  // (no row is held across a reset: the numbering may start again)
	s.track = track;
	s.delay = delay;
	return WC_OK;
}

int wc_track_morph_coded_set_weight(wc_track_morph_coded *h, int stream, double weight, double f0_weight) {
	if (!tc_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "coded track morph: bad stream index");
	if (!(tc_finite(weight) && tc_finite(f0_weight))) return fail(WC_ERR_INVALID, "coded track morph: the weight and the F0 weight must be finite");
	DeviceLock lock(h->dev);
	h->st[stream].w = weight;
	h->st[stream].wf = f0_weight;
	return WC_OK;
}

int wc_track_morph_coded_set_ratios(wc_track_morph_coded *h, int stream, double ratio_a, double ratio_b) {
	if (!tc_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "coded track morph: bad stream index");
	if (!((ratio_a == 0.0 || frame_ratio_valid(ratio_a, h->fft_size)) && (ratio_b == 0.0 || frame_ratio_valid(ratio_b, h->fft_size))))
		return fail(WC_ERR_INVALID, "coded track morph: a ratio must be 0 (none) or finite and >= 2.0 / fft_size");
	DeviceLock lock(h->dev);
	h->st[stream].ra = ratio_a;
	h->st[stream].rb = ratio_b;
	return WC_OK;
}

int wc_track_morph_coded_push_device(wc_track_morph_coded *h, const int *n_a, const double *d_f0_a, const double *d_coded_sp_a,
									 const double *d_coded_ap_a, const double *d_position_b, double *d_f0_out, double *d_sp_out,
									 double *d_ap_out, int *frames_out) {
	if (!h || !n_a || !frames_out) return fail(WC_ERR_INVALID, "coded track morph push: null argument");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	long long in = 0;
	for (int u = 0; u < n; ++u) {
		if (n_a[u] < 0) return fail(WC_ERR_INVALID, "coded track morph push: negative row count");
		if (n_a[u] > h->max_frames) return fail(WC_ERR_INVALID, "coded track morph push: more than max_frames_per_push rows for one stream");
		if (n_a[u] > 0 && h->st[u].track < 0) return fail(WC_ERR_INVALID, "coded track morph push: rows for a stream that was never reset onto a track");
		if (n_a[u] > 0 && h->st[u].ended) return fail(WC_ERR_INVALID, "coded track morph push: rows for a stream that has ended (reset it first)");
		in += n_a[u];
	}
	if (in > 0 && !(d_f0_a && d_coded_sp_a && d_coded_ap_a)) return fail(WC_ERR_INVALID, "coded track morph push: null input array");
	// ---- the plan: host arithmetic on counts, every refusal in front of the first enqueue ----
	if (h->h_rec[h->parity].reserve(0)) return WC_ERR_DEVICE;  // (the copy of the call before the last has read this staging)
	TcSet *set = h->h_rec[h->parity].as<TcSet>();
	TcFrame *fr = reinterpret_cast<TcFrame *>(set + n);
	TcKeep *kp = reinterpret_cast<TcKeep *>(fr + h->frames_cap());  // (moved up behind the frames once their number is known)
	h->next = h->st;
	long long total_out = 0, n_keep = 0, off = 0;
	bool stretch = false;
	for (int u = 0; u < n; ++u) {
		const TcState &old = h->st[u];
		TcState &q = h->next[u];
		tc_set(h, q, set[u]);
		const int c_in = n_a[u];
		if (c_in == 0) { h->cnt[u] = 0; continue; }
		q.n = old.n + c_in;
		const long long keep_old = old.keep(), keep_new = q.keep(), base = (long long)u * h->cap;
		const int c = (int)(keep_new - keep_old);  // frames keep_old .. keep_new - 1: <= c_in <= max_frames_per_push
		for (int k = 0; k < c; ++k) {
			const long long t = keep_old + k;
			TcFrame &f = fr[total_out + k];
			// row t of the voice: a row of this push, or the slot the state before the push holds it in (t - keep_old < delay <= cap)
			f.row = t >= old.n ? (int)(off + (t - old.n)) : ~(int)(base + (old.seq + (t - keep_old)) % h->cap);
			f.pos = (int)(off + (t + q.delay - old.n));  // the entry of row t + delay, which is a row of this push
			f.owner = u; f.pad = 0;
		}
		if (c > 0 && (q.ra != 0.0 || q.rb != 0.0)) stretch = true;
		const long long fresh = old.seq + (old.n - keep_old);  // the next unused number
		q.seq = keep_new < old.n ? old.seq + (keep_new - keep_old) : fresh;
		for (long long r = std::max(keep_new, old.n); r < q.n; ++r) {
			TcKeep &k = kp[n_keep++];
			k.row = (int)(off + (r - old.n));
			k.slot = (int)(base + (q.seq + (r - keep_new)) % h->cap);
		}
		off += c_in;
		h->cnt[u] = c;
		total_out += c;
	}
	if (total_out > 0 && !(d_position_b && d_f0_out && d_sp_out && d_ap_out))
		return fail(WC_ERR_INVALID, "coded track morph push: null position or output array");
	std::copy(h->cnt.begin(), h->cnt.end(), frames_out);  // (no refusal is left)
	if (total_out + n_keep == 0) { h->st.swap(h->next); return WC_OK; }
	return tc_enqueue(h, total_out, n_keep, stretch, d_f0_a, d_coded_sp_a, d_coded_ap_a, d_position_b, d_f0_out, d_sp_out, d_ap_out);
}

int wc_track_morph_coded_flush_device(wc_track_morph_coded *h, const int *want, const double *d_tail, double *d_f0_out, double *d_sp_out,
									  double *d_ap_out, int *frames_out) {
	if (!h || !want || !frames_out) return fail(WC_ERR_INVALID, "coded track morph flush: null argument");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	for (int u = 0; u < n; ++u) {
		if (!want[u]) continue;
		const TcState &s = h->st[u];
		if (s.track < 0 || s.ended) return fail(WC_ERR_INVALID, "coded track morph flush: a wanted stream is not attached or has ended");
		if (s.delay == 0 || s.n == 0) return fail(WC_ERR_INVALID, "coded track morph flush: a wanted stream has no delay or no rows");
	}
	if (h->h_rec[h->parity].reserve(0)) return WC_ERR_DEVICE;
	TcSet *set = h->h_rec[h->parity].as<TcSet>();
	TcFrame *fr = reinterpret_cast<TcFrame *>(set + n);
	h->next = h->st;
	long long total_out = 0, toff = 0;
	bool stretch = false;
	for (int u = 0; u < n; ++u) {
		TcState &q = h->next[u];
		tc_set(h, q, set[u]);
		h->cnt[u] = 0;
		if (!want[u]) continue;
		const long long keep = q.keep(), base = (long long)u * h->cap;
		const int c = (int)(q.n - keep);                          // min(delay, n) rows wait
		const int K = (int)std::min<long long>(q.delay + 1, q.n);  // the stream's entries of d_tail: K - c in front belong to formed frames
		for (int k = 0; k < c; ++k) {
			TcFrame &f = fr[total_out + k];
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
	if (total_out > 0 && !(d_tail && d_f0_out && d_sp_out && d_ap_out)) return fail(WC_ERR_INVALID, "coded track morph flush: null tail or output array");
	std::copy(h->cnt.begin(), h->cnt.end(), frames_out);
	if (total_out == 0) return WC_OK;
	return tc_enqueue(h, total_out, 0, stretch, nullptr, nullptr, nullptr, d_tail, d_f0_out, d_sp_out, d_ap_out);
}

long long wc_track_morph_coded_frames_received(const wc_track_morph_coded *h, int stream) {
	if (!tc_stream_ok(h, stream)) return -1;
	return h->st[stream].n;
}

long long wc_track_morph_coded_frames_formed(const wc_track_morph_coded *h, int stream) {
	if (!tc_stream_ok(h, stream)) return -1;
	return h->st[stream].keep();
}

int wc_track_morph_coded_pending(const wc_track_morph_coded *h, int stream) {
	if (!tc_stream_ok(h, stream)) return WC_ERR_INVALID;
	return (int)(h->st[stream].n - h->st[stream].keep());
}

int wc_track_morph_coded_get_delay(const wc_track_morph_coded *h, int stream) {
	if (!tc_stream_ok(h, stream)) return -1;
	return h->st[stream].delay;
}

int wc_track_morph_coded_track_length(const wc_track_morph_coded *h, int track) {
	if (!tc_track_ok(h, track)) return -1;
	return h->track_m[track];
}

long long wc_track_morph_coded_device_bytes(const wc_track_morph_coded *h) {
	if (!h) return -1;
	return h->device_bytes;
}

}  // extern "C"
