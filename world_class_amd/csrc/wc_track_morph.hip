// Track-morph streams (include/world_class_track_morph.h: wc_track_morph): a live voice arrives push by push and is morphed with a
// track that is resident in the handle, at positions in the track that the kernel reads from device memory -- the settled positions
// of an alignment stream (world_class_align_lag.h) as they are written, without a trip to the host.  The handle sits in front of a
// synthesis stream as wc_morph_stream does (wc_morph_stream.hip) and is the streaming form of wc_morph_parameters_device
// (wc_morph.hip) at d_position_a = the frame's own index.
//
//   track_morph_kernel<STRETCH>   one workgroup of RT_T lanes per formed frame.  The workgroup reads its position itself (one double
//     of d_position_b or d_tail at an index the host wrote, the same for every lane), places it in the track with rt_place -- the
//     clamp to [0, m - 1] and the frame that is all NaN for a position that is not finite are morph_kernel's -- and blends with
//     morph_kernel's mp_f0 / mp_ap_row / mp_sp_row (wc_morph_rows.hpp).  Voice A's side is a whole position (a = 0, w0 = 1, j = i:
//     rt_pair / rt_row / rt_f0 / rt_log_row return the row itself); its row is a row of the push's packed arrays or a ring slot,
//     resolved by the host, which knows it from counts alone.  Voice B's two rows are rows of the stream's track.  Workgroups behind
//     the formed frames copy the rows each stream must keep (TrackKeep) into ring slots that no workgroup of the launch reads.
//     STRETCH = false: no LDS; chosen by the host when no stream that forms frames in the call has a ratio.
//
//   The rule, the ring's numbering, the records and every refusal are wc_track_plan.hpp's, shared with wc_track_morph_coded.hip; this
//   file adds the full-row arrays, the kernel and its launch.
//
//   A push is host arithmetic on counts (the rule, every refusal), one asynchronous copy of the settings, frame and keep records out
//   of page-locked staging, and one launch.  No host code looks at a position.
#include <hip/hip_runtime.h>

#include "../../include/world_class_stream.h"
#include "wc_morph_rows.hpp"
#include "wc_retime_rows.hpp"
#include "wc_stages.hpp"
#include "wc_track_plan.hpp"

using namespace wc;

namespace {

constexpr const char *kName = "track morph";

struct TmArgs {
	const TrackSet *sets;
	const TrackFrame *frames;
	const TrackKeep *keeps;
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
		const TrackKeep k = A.keeps[g - A.total_out];
		if (tid == 0) A.rf0[k.slot] = A.f0_a[k.row];
		const long long from = (long long)k.row * bins, to = (long long)k.slot * bins;
		rt_row(A.sp_a + from, A.sp_a + from, 1.0, 0.0, A.rsp + to, bins, tid);
		rt_row(A.ap_a + from, A.ap_a + from, 1.0, 0.0, A.rap + to, bins, tid);
		return;
	}
	const TrackFrame f = A.frames[g];
	const TrackSet set = A.sets[f.owner];
	const RtPlace qb = rt_place(A.pos[f.pos], set.m);  // (qb.i, qb.j in [0, m - 1] whatever the position holds)
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
		const double *ai = (ring ? A.rap : A.ap_a) + ra_ * bins;
		const MpRow pa{ai, ai, wa0, aa}, pb{A.tap + ib * bins, A.tap + jb * bins, qb.w0, qb.a};
		if (!finite) rt_nan_row(out, bins, tid);
		else mp_ap_row(pa, pb, set.w, out, bins, tid);
	}
	double *__restrict__ out = A.sp_out + g * bins;
	if (!finite) {
		rt_nan_row(out, bins, tid);
		return;
	}
	const double *ai = (ring ? A.rsp : A.sp_a) + ra_ * bins;
	const MpRow sa{ai, ai, wa0, aa}, sb{A.tsp + ib * bins, A.tsp + jb * bins, qb.w0, qb.a};
	// (the ratios are 0 or valid: the setter refuses the others)
	mp_sp_row<STRETCH>(sa, sb, set.w, set.ra, set.rb, out, A.fs, A.fft_size, tid);
}

}  // namespace

struct wc_track_morph : TrackPlan {
	DevBuf tf0, tsp, tap;  // the tracks: n_tracks x max_track_frames rows
	DevBuf rf0, rsp, rap;  // the ring: n_streams x cap slots
};

namespace {

// the call is planned (c); upload, launch, and the plan becomes the state
int tm_enqueue(wc_track_morph *h, const TrackCall &c, const double *d_f0_a, const double *d_sp_a, const double *d_ap_a, const double *d_pos,
			   double *d_f0_out, double *d_sp_out, double *d_ap_out) {
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	TrackRecs r;
	int rc;
	if ((rc = h->upload(hs, c, &r))) return rc;
	TmArgs a;
	a.sets = r.sets; a.frames = r.frames; a.keeps = r.keeps;
	a.total_out = c.total_out; a.fs = h->fs; a.fft_size = h->fft_size;
	a.f0_a = d_f0_a; a.sp_a = d_sp_a; a.ap_a = d_ap_a; a.pos = d_pos;
	a.tf0 = h->tf0.as<double>(); a.tsp = h->tsp.as<double>(); a.tap = h->tap.as<double>();
	a.rf0 = h->rf0.as<double>(); a.rsp = h->rsp.as<double>(); a.rap = h->rap.as<double>();
	a.f0_out = d_f0_out; a.sp_out = d_sp_out; a.ap_out = d_ap_out;
	if ((rc = h->dev->time_begin("track_morph_kernel", hs))) return rc;
	const dim3 grid((unsigned)(c.total_out + c.n_keep));
	if (c.stretch) hipLaunchKernelGGL(track_morph_kernel<true>, grid, dim3(RT_T), 0, hs, a);
	else hipLaunchKernelGGL(track_morph_kernel<false>, grid, dim3(RT_T), 0, hs, a);
	WC_HIP(hipGetLastError());
	if ((rc = h->dev->time_end("track_morph_kernel", hs))) return rc;
	h->commit();
	return WC_OK;
}

}  // namespace

extern "C" {

wc_track_morph *wc_track_morph_create(int fs, int fft_size, int n_streams, int n_tracks, int max_track_frames, int max_frames_per_push,
									  int max_delay) {
	const std::string why = TrackPlan::check(kName, fs, fft_size, n_streams, n_tracks, max_track_frames, max_frames_per_push, max_delay);
	if (!why.empty()) { set_error(why); return nullptr; }
	if (!TrackPlan::fits(n_streams, n_tracks, max_track_frames, max_frames_per_push, max_delay, 1)) {
		set_error("track morph: n_streams x max_frames_per_push, n_streams x ring slots or n_tracks x max_track_frames too large");
		return nullptr;
	}
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	wc_track_morph *h = new wc_track_morph();
	h->init(kName, dev, fs, fft_size, n_streams, n_tracks, max_track_frames, max_frames_per_push, max_delay);
	const size_t bins = fft_size / 2 + 1, rows = (size_t)n_tracks * max_track_frames, slots = (size_t)n_streams * (size_t)h->cap;
	const size_t rec = h->rec_bytes();
	if (h->tf0.reserve(sizeof(double) * rows) || h->tsp.reserve(sizeof(double) * rows * bins) || h->tap.reserve(sizeof(double) * rows * bins) ||
		(slots > 0 && (h->rf0.reserve(sizeof(double) * slots) || h->rsp.reserve(sizeof(double) * slots * bins) || h->rap.reserve(sizeof(double) * slots * bins))) ||
		h->rec.reserve(rec)) {
		wc_track_morph_destroy(h);
		return nullptr;
	}
	return h;
}

void wc_track_morph_destroy(wc_track_morph *h) {
	if (!h) return;
	h->dev->quiesce();
	h->tf0.release(); h->tsp.release(); h->tap.release(); h->rf0.release(); h->rsp.release(); h->rap.release();
	h->rec.release();
	delete h;
}

int wc_track_morph_set_track_device(wc_track_morph *h, int track, int m, const double *d_f0_b, const double *d_sp_b, const double *d_ap_b) {
	return track_plan_set_track(kName, h, track, m, d_f0_b && d_sp_b && d_ap_b, [&](hipStream_t hs, size_t first) {
		const size_t bins = h->fft_size / 2 + 1;
		WC_HIP(hipMemcpyAsync(h->tf0.as<double>() + first, d_f0_b, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, hs));
		WC_HIP(hipMemcpyAsync(h->tsp.as<double>() + first * bins, d_sp_b, sizeof(double) * (size_t)m * bins, hipMemcpyDeviceToDevice, hs));
		WC_HIP(hipMemcpyAsync(h->tap.as<double>() + first * bins, d_ap_b, sizeof(double) * (size_t)m * bins, hipMemcpyDeviceToDevice, hs));
		return (int)WC_OK;
	});
}

int wc_track_morph_reset(wc_track_morph *h, int stream, int track, int delay) { return track_plan_reset(kName, h, stream, track, delay); }

int wc_track_morph_set_weight(wc_track_morph *h, int stream, double weight, double f0_weight) {
	return track_plan_set_weight(kName, h, stream, weight, f0_weight);
}

int wc_track_morph_set_ratios(wc_track_morph *h, int stream, double ratio_a, double ratio_b) {
	return track_plan_set_ratios(kName, h, stream, ratio_a, ratio_b);
}

int wc_track_morph_push_device(wc_track_morph *h, const int *n_a, const double *d_f0_a, const double *d_sp_a, const double *d_ap_a,
							   const double *d_position_b, double *d_f0_out, double *d_sp_out, double *d_ap_out, int *frames_out) {
	if (!h || !n_a || !frames_out) return fail(WC_ERR_INVALID, "track morph push: null argument");
	DeviceLock lock(h->dev);
	TrackCall c;
	if (int rc = h->plan_push(n_a, d_f0_a && d_sp_a && d_ap_a, d_position_b && d_f0_out && d_sp_out && d_ap_out, frames_out, &c)) return rc;
	if (c.total_out + c.n_keep == 0) return WC_OK;
	return tm_enqueue(h, c, d_f0_a, d_sp_a, d_ap_a, d_position_b, d_f0_out, d_sp_out, d_ap_out);
}

int wc_track_morph_flush_device(wc_track_morph *h, const int *want, const double *d_tail, double *d_f0_out, double *d_sp_out,
								double *d_ap_out, int *frames_out) {
	if (!h || !want || !frames_out) return fail(WC_ERR_INVALID, "track morph flush: null argument");
	DeviceLock lock(h->dev);
	TrackCall c;
	if (int rc = h->plan_flush(want, d_tail && d_f0_out && d_sp_out && d_ap_out, frames_out, &c)) return rc;
	if (c.total_out == 0) return WC_OK;
	return tm_enqueue(h, c, nullptr, nullptr, nullptr, d_tail, d_f0_out, d_sp_out, d_ap_out);
}

long long wc_track_morph_frames_received(const wc_track_morph *h, int stream) { return track_plan_frames_received(h, stream); }
long long wc_track_morph_frames_formed(const wc_track_morph *h, int stream) { return track_plan_frames_formed(h, stream); }
int wc_track_morph_pending(const wc_track_morph *h, int stream) { return track_plan_pending(h, stream); }
int wc_track_morph_get_delay(const wc_track_morph *h, int stream) { return track_plan_get_delay(h, stream); }
int wc_track_morph_track_length(const wc_track_morph *h, int track) { return track_plan_track_length(h, track); }

}  // extern "C"
