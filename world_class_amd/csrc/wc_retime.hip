// Time-scale modification (include/world_class_io.h: wc_retime_parameters_device; world_class_c.h:
// wc_synthesis_compute_coded_retimed_device): the frames of a packed batch resampled along a position per OUTPUT frame.
//
//   retime_kernel<STRETCH>   one workgroup per output frame, one launch for the whole batch, out of place.  Output frame k of an
//     utterance with n source frames sits at p = clamp(pos[k], 0, n - 1) source frames: i = floor(p), a = p - i; a == 0 copies
//     frame i, a > 0 writes (1 - a) * row[i] + a * row[i + 1] for both rows (the interpolation reference src/synthesis.cpp:346-393
//     applies between two frames, without its fabs and its aperiodicity clamp) and an F0 that is voiced exactly where Synthesis'
//     own interpolated voicing (:200-204) is; a position that is not finite makes its own frame NaN.  A gather bound by memory
//     traffic: up to four rows in, two out, two bins per lane and access (a row of fft_size/2+1 doubles starts on a 16-byte
//     boundary on every other frame only, so the 16-byte accesses are issued with 8-byte alignment and the row's odd last bin is
//     peeled); consecutive output frames sit on consecutive workgroups, so the source row two neighbours share comes out of L2.
//     STRETCH: the interpolated row of sp goes to LDS as its logarithm and is stretched by the frame's ratio (wc::stretched_bin,
//     wc_stretch.hpp: the rule of stretch_kernel, wc_io.hip) before its one write.
//   retime_stream_kernel<STRETCH>   the same frame for the synthesis streams (wc_synth_stream_set_speed): positions in absolute source
//     frames of a stream, the source rows those of one push plus one carried row per stream; it also keeps each stream's newest
//     source row for the next push.  rt_pair / rt_row / rt_f0 / rt_stretched_row (wc_retime_rows.hpp) are shared by both kernels
//     and by morph_kernel (wc_morph.hip).
//   A workgroup of retime_kernel finds its utterance by bisection in the descriptors (one of retime_stream_kernel reads its stream's
//   index from a per-frame array of the host), which go up through page-locked staging kept per
//   (device, stream): a call only enqueues.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <string>

#include "../../include/world_class_c.h"
#include "../../include/world_class_io.h"
#include "wc_retime_rows.hpp"
#include "wc_stages.hpp"

using namespace wc;

namespace {

struct RtUtt {
	long long in_off, out_off;  // first source / output frame in the packed arrays
	int n;                      // source frames
};

struct RtArgs {
	const RtUtt *utts;
	int n_utt, fs, fft_size;
	const double *pos, *f0_in, *sp_in, *ap_in, *scale, *ratio;
	double *f0_out, *sp_out, *ap_out;
};

struct RtStreamArgs {
	const RtStreamDesc *desc;
	const int *owner;
	int n_desc, fs, fft_size;
	long long total_out;
	const double *pos, *f0_in, *sp_in, *ap_in, *scale, *ratio;
	double *f0_out, *sp_out, *ap_out;
};

// the stretched row on this translation unit's one LDS row (rt_stretched_row, wc_retime_rows.hpp)
__device__ __forceinline__ void rt_stretched_row_tu(const double *__restrict__ ri, const double *__restrict__ rj, double w0, double a,
												 double *__restrict__ out, double ratio, int fs, int fft_size, int tid) {
	__shared__ double lg[kMaxBins];
	__shared__ double fill;
	rt_stretched_row(ri, rj, w0, a, out, ratio, fs, fft_size, tid, lg, &fill);
}

template <bool STRETCH>
__global__ __launch_bounds__(RT_T) void retime_kernel(RtArgs A) {
	const int tid = threadIdx.x;
	const long long g = blockIdx.x;
	int lo = 0, hi = A.n_utt;  // the last utterance that starts at or before g (empty ones in front of it share its offset)
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (A.utts[mid].out_off <= g) lo = mid;
		else hi = mid;
	}
	const RtUtt u = A.utts[lo];
	const int bins = A.fft_size / 2 + 1;
	const RtPlace q = rt_place(A.pos[g], u.n);
	const bool finite = q.finite;
	const int i = q.i, j = q.j;
	const double a = q.a, w0 = q.w0;

	if (A.f0_out && tid == 0) {
		double v = __builtin_nan("");
		if (finite) v = rt_f0(A.f0_in[u.in_off + i], A.f0_in[u.in_off + j], w0, a);
		if (A.scale) v *= A.scale[g];
		A.f0_out[g] = v;
	}
	if (A.ap_out) {
		double *__restrict__ out = A.ap_out + g * bins;
		if (!finite) rt_nan_row(out, bins, tid);
		else rt_row(A.ap_in + (u.in_off + i) * bins, A.ap_in + (u.in_off + j) * bins, w0, a, out, bins, tid);
	}
	if (!A.sp_out) return;
	double *__restrict__ out = A.sp_out + g * bins;
	const double *__restrict__ ri = A.sp_in + (u.in_off + i) * bins, *__restrict__ rj = A.sp_in + (u.in_off + j) * bins;
	const double ratio = STRETCH ? A.ratio[g] : 0.0;
	if (!finite || (STRETCH && ratio != 0.0 && !frame_ratio_valid(ratio, A.fft_size))) {
		rt_nan_row(out, bins, tid);
		return;
	}
	if (!STRETCH || ratio == 0.0) {
		rt_row(ri, rj, w0, a, out, bins, tid);
		return;
	}
	if constexpr (STRETCH) rt_stretched_row_tu(ri, rj, w0, a, out, ratio, A.fs, A.fft_size, tid);
}

// The streaming form (wc_synth_stream_set_speed, include/world_class_stream.h): the same frame at the same position, but the source
// rows of a stream are the rows of this push and, for the frame before them, the stream's carried row.  Workgroups behind the
// synthesis frames keep each stream's newest source row for the next push (the other side of the handle's ping-pong pair).
template <bool STRETCH>
__global__ __launch_bounds__(RT_T) void retime_stream_kernel(RtStreamArgs A) {
	const int tid = threadIdx.x;
	const long long g = blockIdx.x;
	const int bins = A.fft_size / 2 + 1;
	if (g >= A.total_out) {  // the newest source row of stream g - total_out is kept
		const RtStreamDesc u = A.desc[g - A.total_out];
		if (!u.keep_sp) return;
		const long long r = u.in_off + u.n_in - 1;
		if (tid == 0) *u.keep_f0 = A.f0_in[r];
		rt_row(A.sp_in + r * bins, A.sp_in + r * bins, 1.0, 0.0, u.keep_sp, bins, tid);
		rt_row(A.ap_in + r * bins, A.ap_in + r * bins, 1.0, 0.0, u.keep_ap, bins, tid);
		return;
	}
	// the frame's stream comes from the host (no bisection: at fft 1024 a workgroup moves a few KB, and the chain of dependent
	// loads in front of its rows is what it would wait for)
	const RtStreamDesc u = A.desc[A.owner[g]];
	const double p = A.pos[g];  // absolute source frames; the host keeps f_before - 1 <= floor(p) and ceil(p) < f_before + n_in
	const long long i = static_cast<long long>(floor(p));
	const double a = p - i;
	const double w0 = 1.0 - a;
	const long long ki = i - u.f_before, kj = a > 0.0 ? ki + 1 : ki;  // rows of this push; -1: the carried row
	const double *__restrict__ fi = ki < 0 ? u.carry_f0 : A.f0_in + u.in_off + ki, *__restrict__ fj = kj < 0 ? u.carry_f0 : A.f0_in + u.in_off + kj;
	if (tid == 0) A.f0_out[g] = rt_f0(*fi, *fj, w0, a) * A.scale[g];
	{
		const double *__restrict__ ri = ki < 0 ? u.carry_ap : A.ap_in + (u.in_off + ki) * bins;
		const double *__restrict__ rj = kj < 0 ? u.carry_ap : A.ap_in + (u.in_off + kj) * bins;
		rt_row(ri, rj, w0, a, A.ap_out + g * bins, bins, tid);
	}
	double *__restrict__ out = A.sp_out + g * bins;
	const double *__restrict__ ri = ki < 0 ? u.carry_sp : A.sp_in + (u.in_off + ki) * bins;
	const double *__restrict__ rj = kj < 0 ? u.carry_sp : A.sp_in + (u.in_off + kj) * bins;
	const double ratio = STRETCH ? A.ratio[g] : 0.0;
	if (STRETCH && ratio != 0.0 && !frame_ratio_valid(ratio, A.fft_size)) {
		rt_nan_row(out, bins, tid);
		return;
	}
	if (!STRETCH || ratio == 0.0) {
		rt_row(ri, rj, w0, a, out, bins, tid);
		return;
	}
	if constexpr (STRETCH) rt_stretched_row_tu(ri, rj, w0, a, out, ratio, A.fs, A.fft_size, tid);
}

// descriptor staging per (device, stream): calls on one stream are ordered behind each other, calls on different streams never
// share a buffer.  A few dozen bytes per utterance, kept for the life of the process like the decoder's plans.
std::mutex g_stage_mu;
std::map<std::pair<int, hipStream_t>, Staging *> g_stage;

}  // namespace

const char *wc::retime_check(int fs, int fft_size, int n_utt, const int *in_length, const int *out_length, long long *total_out) {
	if (!fft_size_supported(fft_size)) return "retime: fft_size must be 512, 1024, 2048 or 4096";
	if (fs <= 0) return "retime: fs must be positive";
	if (n_utt < 0) return "retime: negative n_utt";
	if (n_utt > 0 && (!in_length || !out_length)) return "retime: null length array";
	long long ti = 0, to = 0;
	for (int u = 0; u < n_utt; ++u) {
		if (in_length[u] < 0 || out_length[u] < 0) return "retime: negative length";
		if (out_length[u] > 0 && in_length[u] < 1) return "retime: output frames of an utterance without source frames";
		ti += in_length[u];
		to += out_length[u];
	}
	if (ti > 0xffffffffll || to > 0xffffffffll) return "retime: more than 2^32 - 1 frames";
	*total_out = to;
	return nullptr;
}

int wc::retime_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, int n_utt, const int *in_length, const double *d_f0_in,
					   const double *d_sp_in, const double *d_ap_in, const int *out_length, const double *d_position,
					   const double *d_f0_scale, const double *d_spectral_ratio, double *d_f0_out, double *d_sp_out, double *d_ap_out,
					   long long total_out) {
	if (total_out == 0 || (!d_f0_out && !d_sp_out && !d_ap_out)) return WC_OK;
	// WC_RETIME_MOD=route: scale and stretch as wc_modify_parameters_frames_device behind the plain kernel (the measurement of
	// DESIGN.md section 10)
	static const bool route_mod = [] { const char *e = getenv("WC_RETIME_MOD"); return e && std::string(e) == "route"; }();
	Staging *st;
	{
		std::lock_guard<std::mutex> g(g_stage_mu);
		Staging *&slot = g_stage[{dev->id, s}];
		if (!slot) slot = new Staging();
		st = slot;
	}
	int rc;
	const size_t bytes = sizeof(RtUtt) * (size_t)n_utt;
	if ((rc = st->h.reserve(bytes))) return rc;
	if ((rc = st->d.reserve(bytes))) return rc;
	RtUtt *h = st->h.as<RtUtt>();
	long long fi = 0, fo = 0;
	for (int u = 0; u < n_utt; ++u) {
		h[u].in_off = fi; h[u].out_off = fo; h[u].n = in_length[u];
		fi += in_length[u];
		fo += out_length[u];
	}
	WC_HIP(hipMemcpyAsync(st->d.p, h, bytes, hipMemcpyHostToDevice, s));
	if ((rc = st->h.mark(s))) return rc;
	RtArgs a;
	a.utts = st->d.as<RtUtt>();
	a.n_utt = n_utt; a.fs = fs; a.fft_size = fft_size;
	a.pos = d_position; a.f0_in = d_f0_in; a.sp_in = d_sp_in; a.ap_in = d_ap_in;
	a.f0_out = d_f0_out; a.sp_out = d_sp_out; a.ap_out = d_ap_out;
	a.scale = route_mod ? nullptr : d_f0_scale;
	a.ratio = route_mod ? nullptr : d_spectral_ratio;
	if (a.ratio && d_sp_out) hipLaunchKernelGGL(retime_kernel<true>, dim3((unsigned)total_out), dim3(RT_T), 0, s, a);
	else hipLaunchKernelGGL(retime_kernel<false>, dim3((unsigned)total_out), dim3(RT_T), 0, s, a);
	WC_HIP(hipGetLastError());
	if (route_mod) return modify_frames_enqueue(s, fs, fft_size, total_out, d_f0_out, d_sp_out, d_f0_scale, d_spectral_ratio);
	return WC_OK;
}

int wc::retime_stream_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, int n_desc, const RtStreamDesc *d_desc, const int *d_owner,
							  long long total_out, const double *d_position, const double *d_f0_scale, const double *d_spectral_ratio, const double *d_f0_in,
							  const double *d_sp_in, const double *d_ap_in, double *d_f0_out, double *d_sp_out, double *d_ap_out) {
	if (n_desc <= 0) return WC_OK;
	RtStreamArgs a;
	a.desc = d_desc;
	a.owner = d_owner;
	a.n_desc = n_desc; a.fs = fs; a.fft_size = fft_size; a.total_out = total_out;
	a.pos = d_position; a.f0_in = d_f0_in; a.sp_in = d_sp_in; a.ap_in = d_ap_in; a.scale = d_f0_scale; a.ratio = d_spectral_ratio;
	a.f0_out = d_f0_out; a.sp_out = d_sp_out; a.ap_out = d_ap_out;
	int rc;
	if ((rc = dev->time_begin("retime_stream_kernel", s))) return rc;
	const dim3 grid((unsigned)(total_out + n_desc));
	if (a.ratio) hipLaunchKernelGGL(retime_stream_kernel<true>, grid, dim3(RT_T), 0, s, a);
	else hipLaunchKernelGGL(retime_stream_kernel<false>, grid, dim3(RT_T), 0, s, a);
	WC_HIP(hipGetLastError());
	return dev->time_end("retime_stream_kernel", s);
}

extern "C" int wc_retime_parameters_device(int fs, int fft_size, int n_utt, const int *in_length, const double *d_f0_in, const double *d_sp_in,
										   const double *d_ap_in, const int *out_length, const double *d_position, const double *d_f0_scale,
										   const double *d_spectral_ratio, double *d_f0_out, double *d_sp_out, double *d_ap_out) {
	long long total_out = 0;
	if (const char *why = retime_check(fs, fft_size, n_utt, in_length, out_length, &total_out)) return fail(WC_ERR_INVALID, why);
	const double *const in[3] = {d_f0_in, d_sp_in, d_ap_in}, *const out[3] = {d_f0_out, d_sp_out, d_ap_out};
	for (int k = 0; k < 3; ++k) {
		if (!in[k] != !out[k]) return fail(WC_ERR_INVALID, "retime: an input without its output (or the reverse)");
		if (in[k] && in[k] == out[k]) return fail(WC_ERR_INVALID, "retime: in place is not supported (the output must not be the input)");
	}
	if (total_out > 0 && !d_position) return fail(WC_ERR_INVALID, "retime: null position array");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	return retime_enqueue(dev, dev->active(), fs, fft_size, n_utt, in_length, d_f0_in, d_sp_in, d_ap_in, out_length, d_position, d_f0_scale,
						  d_spectral_ratio, d_f0_out, d_sp_out, d_ap_out, total_out);
}
