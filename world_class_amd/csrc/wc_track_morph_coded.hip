// Coded track-morph streams (include/world_class_track_morph_coded.h: wc_track_morph_coded): wc_track_morph (wc_track_morph.hip) with
// its tracks, its ring and its live rows held as coded features -- number_of_dimensions + GetNumberOfAperiodicities(fs) doubles per
// row instead of 2 x (fft_size/2 + 1).  The rule, the ring's numbering, the refusals and the records are wc_track_plan.hpp's, the
// plan both handles follow; the outputs are full rows with the bits of that handle on the decoded rows.
//
//   track_gather_coded_kernel   one wavefront per formed frame g or kept row.  For a frame it reads the frame's position itself (one
//     double of d_position_b or d_tail at an index the host wrote, the same for every lane), places it in the track with rt_place --
//     qb.i, qb.j lie in [0, m - 1] whatever the double holds -- and copies three coded rows, sp and ap part, into the handle's
//     scratch: A's row (a row of the push's packed arrays or a ring slot) to slot 3g, track rows i and j to slots 3g + 1 and 3g + 2.
//     For a kept row (TrackKeep) it copies the coded row and its F0 into a ring slot that no workgroup of the call reads.  Coded rows
//     are 8-byte aligned only (nd may be odd, n_ap is 1, 3 or 5): every access is one double.
//
//   wc::decode_features_enqueue (wc_synth_coded.hip), unchanged, over the 3 x frames scratch slots: the one-wavefront kernel at
//     fft 2048, the codec's two workgroup kernels at the other sizes.
//
//   track_morph_coded_kernel<STRETCH>   track_morph_kernel's launch shape and its blend (mp_f0 / mp_ap_row / mp_sp_row,
//     wc_morph_rows.hpp) on the decoded slots: A's row is slot 3g, B's rows are slots 3g + 1 and 3g + 2, the weights come from rt_place on the same double, its `finite`
//     gives the frame that is NaN throughout; F0 comes from the push or the ring for A and from the resident track's F0 for B.
//     STRETCH = false: no LDS; chosen by the host when no stream that forms frames in the call has a ratio.
//
//   A push is host arithmetic on counts (the rule, every refusal), one asynchronous copy of the settings, frame and keep records out
//   of page-locked staging, and the three enqueues (the gather alone when the push only keeps rows).  No host code looks at a position.
#include <hip/hip_runtime.h>

#include "../../include/world_class_track_morph_coded.h"
#include "wc_morph_rows.hpp"
#include "wc_retime_rows.hpp"
#include "wc_stages.hpp"
#include "wc_track_plan.hpp"

using namespace wc;

namespace {

constexpr int TC_W = 64;  // the gather's workgroup: one wavefront

constexpr const char *kName = "coded track morph";

struct TcArgs {
	const TrackSet *sets;
	const TrackFrame *frames;
	const TrackKeep *keeps;
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
		const TrackKeep k = A.keeps[g - A.total_out];
		if (lane == 0) A.rf0[k.slot] = A.f0_a[k.row];
		tc_copy(A.csp_a + (long long)k.row * nd, A.rcsp + (long long)k.slot * nd, nd, lane);
		tc_copy(A.cap_a + (long long)k.row * n_ap, A.rcap + (long long)k.slot * n_ap, n_ap, lane);
		return;
	}
	const TrackFrame f = A.frames[g];
	const TrackSet set = A.sets[f.owner];
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
	const TrackFrame f = A.frames[g];
	const TrackSet set = A.sets[f.owner];
	const RtPlace qb = rt_place(A.pos[f.pos], set.m);  // the gather's placement: the same double, the same m
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
		const MpRow pa{A.sap + sa, A.sap + sa, wa0, aa}, pb{A.sap + si, A.sap + sj, qb.w0, qb.a};
		if (!finite) rt_nan_row(out, bins, tid);
		else mp_ap_row(pa, pb, set.w, out, bins, tid);
	}
	double *__restrict__ out = A.sp_out + g * bins;
	if (!finite) {
		rt_nan_row(out, bins, tid);
		return;
	}
	const MpRow ea{A.ssp + sa, A.ssp + sa, wa0, aa}, eb{A.ssp + si, A.ssp + sj, qb.w0, qb.a};
	// (the ratios are 0 or valid: the setter refuses the others)
	mp_sp_row<STRETCH>(ea, eb, set.w, set.ra, set.rb, out, A.fs, A.fft_size, tid);
}

}  // namespace

struct wc_track_morph_coded : TrackPlan {
	int nd, n_ap;
	DevBuf tf0, tcsp, tcap;       // the tracks: n_tracks x max_track_frames coded rows
	DevBuf rf0, rcsp, rcap;       // the ring: n_streams x cap slots
	DevBuf scsp, scap, ssp, sap;  // the scratch: 3 x frames_cap() slots, coded and decoded
	long long device_bytes = 0;
};

namespace {

// create allocates every array once and exactly (rounded up to 256 bytes): DevBuf::reserve's head-room is for buffers that grow
int tc_alloc(wc_track_morph_coded *h, DevBuf &b, size_t bytes) {
	if (bytes == 0) return WC_OK;
	const size_t want = (bytes + 255) / 256 * 256;
	WC_HIP(hipMalloc(&b.p, want));
	b.cap = want;
	h->device_bytes += (long long)want;
	return WC_OK;
}

// the call is planned (c); upload, gather, decode, blend, and the plan becomes the state
int tc_enqueue(wc_track_morph_coded *h, const TrackCall &c, const double *d_f0_a, const double *d_csp_a, const double *d_cap_a,
			   const double *d_pos, double *d_f0_out, double *d_sp_out, double *d_ap_out) {
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	TrackRecs r;
	int rc;
	if ((rc = h->upload(hs, c, &r))) return rc;
	TcArgs a;
	a.sets = r.sets; a.frames = r.frames; a.keeps = r.keeps;
	a.total_out = c.total_out; a.fs = h->fs; a.fft_size = h->fft_size; a.nd = h->nd; a.n_ap = h->n_ap;
	a.f0_a = d_f0_a; a.csp_a = d_csp_a; a.cap_a = d_cap_a; a.pos = d_pos;
	a.tf0 = h->tf0.as<double>(); a.tcsp = h->tcsp.as<double>(); a.tcap = h->tcap.as<double>();
	a.rf0 = h->rf0.as<double>(); a.rcsp = h->rcsp.as<double>(); a.rcap = h->rcap.as<double>();
	a.scsp = h->scsp.as<double>(); a.scap = h->scap.as<double>(); a.ssp = h->ssp.as<double>(); a.sap = h->sap.as<double>();
	a.f0_out = d_f0_out; a.sp_out = d_sp_out; a.ap_out = d_ap_out;
	if ((rc = h->dev->time_begin("track_gather_coded_kernel", hs))) return rc;
	hipLaunchKernelGGL(track_gather_coded_kernel, dim3((unsigned)(c.total_out + c.n_keep)), dim3(TC_W), 0, hs, a);
	WC_HIP(hipGetLastError());
	if ((rc = h->dev->time_end("track_gather_coded_kernel", hs))) return rc;
	if (c.total_out > 0) {
		if ((rc = h->dev->time_begin("track_morph_coded_decode", hs))) return rc;
		if ((rc = decode_features_enqueue(h->dev, hs, h->fs, h->fft_size, 3 * c.total_out, h->nd, a.scsp, a.scap, nullptr, a.ssp, a.sap))) return rc;
		if ((rc = h->dev->time_end("track_morph_coded_decode", hs))) return rc;
		if ((rc = h->dev->time_begin("track_morph_coded_kernel", hs))) return rc;
		const dim3 grid((unsigned)c.total_out);
		if (c.stretch) hipLaunchKernelGGL(track_morph_coded_kernel<true>, grid, dim3(RT_T), 0, hs, a);
		else hipLaunchKernelGGL(track_morph_coded_kernel<false>, grid, dim3(RT_T), 0, hs, a);
		WC_HIP(hipGetLastError());
		if ((rc = h->dev->time_end("track_morph_coded_kernel", hs))) return rc;
	}
	h->commit();
	return WC_OK;
}

}  // namespace

extern "C" {

wc_track_morph_coded *wc_track_morph_coded_create(int fs, int fft_size, int number_of_dimensions, int n_streams, int n_tracks,
												  int max_track_frames, int max_frames_per_push, int max_delay) {
	const std::string bad = TrackPlan::check(kName, fs, fft_size, n_streams, n_tracks, max_track_frames, max_frames_per_push, max_delay);
	if (!bad.empty()) { set_error(bad); return nullptr; }
	if (const char *why = decode_features_check(fs, fft_size, number_of_dimensions)) { set_error(std::string("coded track morph: ") + why); return nullptr; }
	// (the decoder's grid is the three scratch slots of every frame)
	if (!TrackPlan::fits(n_streams, n_tracks, max_track_frames, max_frames_per_push, max_delay, 3)) {
		set_error("coded track morph: 3 x n_streams x max_frames_per_push, n_streams x ring slots or n_tracks x max_track_frames too large");
		return nullptr;
	}
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	const CodecPlan *pl;
	if (codec_plan(dev, fs, fft_size, false, &pl)) return nullptr;  // (built here: no push is the first use, which may wait for the device)
	wc_track_morph_coded *h = new wc_track_morph_coded();
	h->init(kName, dev, fs, fft_size, n_streams, n_tracks, max_track_frames, max_frames_per_push, max_delay);
	h->nd = number_of_dimensions; h->n_ap = GetNumberOfAperiodicities(fs);
	const size_t bins = fft_size / 2 + 1, rows = (size_t)n_tracks * max_track_frames, slots = (size_t)n_streams * (size_t)h->cap;
	const size_t nd = h->nd, n_ap = h->n_ap, scr = 3 * h->frames_cap(), d = sizeof(double);
	const size_t rec = h->rec_bytes();
	if (hipSetDevice(dev->id) != hipSuccess || tc_alloc(h, h->tf0, d * rows) || tc_alloc(h, h->tcsp, d * rows * nd) || tc_alloc(h, h->tcap, d * rows * n_ap) ||
		tc_alloc(h, h->rf0, d * slots) || tc_alloc(h, h->rcsp, d * slots * nd) || tc_alloc(h, h->rcap, d * slots * n_ap) ||
		tc_alloc(h, h->scsp, d * scr * nd) || tc_alloc(h, h->scap, d * scr * n_ap) || tc_alloc(h, h->ssp, d * scr * bins) ||
		tc_alloc(h, h->sap, d * scr * bins) || tc_alloc(h, h->rec.d, rec) || h->rec.reserve(rec)) {  // (the device half is accounted; reserve finds it there)
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
	h->rec.release();
	delete h;
}

int wc_track_morph_coded_set_track_device(wc_track_morph_coded *h, int track, int m, const double *d_f0_b, const double *d_coded_sp_b,
										  const double *d_coded_ap_b) {
	return track_plan_set_track(kName, h, track, m, d_f0_b && d_coded_sp_b && d_coded_ap_b, [&](hipStream_t hs, size_t first) {
		const size_t nd = h->nd, n_ap = h->n_ap;
		WC_HIP(hipMemcpyAsync(h->tf0.as<double>() + first, d_f0_b, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, hs));
		WC_HIP(hipMemcpyAsync(h->tcsp.as<double>() + first * nd, d_coded_sp_b, sizeof(double) * (size_t)m * nd, hipMemcpyDeviceToDevice, hs));
		WC_HIP(hipMemcpyAsync(h->tcap.as<double>() + first * n_ap, d_coded_ap_b, sizeof(double) * (size_t)m * n_ap, hipMemcpyDeviceToDevice, hs));
		return (int)WC_OK;
	});
}

int wc_track_morph_coded_reset(wc_track_morph_coded *h, int stream, int track, int delay) { return track_plan_reset(kName, h, stream, track, delay); }

int wc_track_morph_coded_set_weight(wc_track_morph_coded *h, int stream, double weight, double f0_weight) {
	return track_plan_set_weight(kName, h, stream, weight, f0_weight);
}

int wc_track_morph_coded_set_ratios(wc_track_morph_coded *h, int stream, double ratio_a, double ratio_b) {
	return track_plan_set_ratios(kName, h, stream, ratio_a, ratio_b);
}

int wc_track_morph_coded_push_device(wc_track_morph_coded *h, const int *n_a, const double *d_f0_a, const double *d_coded_sp_a,
									 const double *d_coded_ap_a, const double *d_position_b, double *d_f0_out, double *d_sp_out,
									 double *d_ap_out, int *frames_out) {
	if (!h || !n_a || !frames_out) return fail(WC_ERR_INVALID, "coded track morph push: null argument");
	DeviceLock lock(h->dev);
	TrackCall c;
	if (int rc = h->plan_push(n_a, d_f0_a && d_coded_sp_a && d_coded_ap_a, d_position_b && d_f0_out && d_sp_out && d_ap_out, frames_out, &c)) return rc;
	if (c.total_out + c.n_keep == 0) return WC_OK;
	return tc_enqueue(h, c, d_f0_a, d_coded_sp_a, d_coded_ap_a, d_position_b, d_f0_out, d_sp_out, d_ap_out);
}

int wc_track_morph_coded_flush_device(wc_track_morph_coded *h, const int *want, const double *d_tail, double *d_f0_out, double *d_sp_out,
									  double *d_ap_out, int *frames_out) {
	if (!h || !want || !frames_out) return fail(WC_ERR_INVALID, "coded track morph flush: null argument");
	DeviceLock lock(h->dev);
	TrackCall c;
	if (int rc = h->plan_flush(want, d_tail && d_f0_out && d_sp_out && d_ap_out, frames_out, &c)) return rc;
	if (c.total_out == 0) return WC_OK;
	return tc_enqueue(h, c, nullptr, nullptr, nullptr, d_tail, d_f0_out, d_sp_out, d_ap_out);
}

long long wc_track_morph_coded_frames_received(const wc_track_morph_coded *h, int stream) { return track_plan_frames_received(h, stream); }
long long wc_track_morph_coded_frames_formed(const wc_track_morph_coded *h, int stream) { return track_plan_frames_formed(h, stream); }
int wc_track_morph_coded_pending(const wc_track_morph_coded *h, int stream) { return track_plan_pending(h, stream); }
int wc_track_morph_coded_get_delay(const wc_track_morph_coded *h, int stream) { return track_plan_get_delay(h, stream); }
int wc_track_morph_coded_track_length(const wc_track_morph_coded *h, int track) { return track_plan_track_length(h, track); }
long long wc_track_morph_coded_device_bytes(const wc_track_morph_coded *h) { return h ? h->device_bytes : -1; }

}  // extern "C"
