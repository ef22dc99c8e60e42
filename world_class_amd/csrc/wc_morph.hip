// Voice morphing (include/world_class_io.h: wc_morph_parameters_device; world_class_c.h:
// wc_synthesis_compute_coded_morphed_device): every output frame of a packed batch of pairs takes a position in utterance A, a
// position in utterance B and a weight, and is the blend of the two retimed frames.
//
//   morph_kernel<STRETCH>   one workgroup per output frame, one launch for the whole batch, out of place.  The two frames are
//     those of retime_kernel at the two positions (rt_place / rt_pair / rt_row / rt_f0, wc_retime_rows.hpp: the same products and
//     sums).  ap = (1 - w) * apA + w * apB; sp = exp((1 - w) * la + w * lb) on the two log envelopes; F0 = exp of the same blend of
//     the two log F0 where both frames are voiced, the nearer source's F0 (or 0) where one is, 0 where neither is.  w == 0 and
//     w == 1 write the one source's retimed frame bit for bit (the paths of retime_kernel).  A gather bound by memory traffic or by
//     its two log and one exp per bin: up to eight rows in, two out, two bins per lane and access.  The blend itself (mp_f0,
//     mp_ap_row, mp_sp_row<STRETCH>) is stated in wc_morph_rows.hpp, shared with the stream kernels (wc_morph_stream.hip,
//     wc_track_morph.hip, wc_track_morph_coded.hip); this kernel's own are the bisection, the outputs that may be absent, and the
//     frame that is NaN: a position or weight that is not finite, or (the sp row only) an invalid ratio of either source.
//     STRETCH = false: no LDS.  STRETCH: two LDS rows of kMaxBins doubles hold the sources' log envelopes, stretched by that source's
//     ratio for this frame (wc::stretched_log_bin, wc_stretch.hpp), a ratio of 0 the row's own logarithm.
//   A workgroup finds its pair by bisection in the descriptors, which go up through page-locked staging kept per (device, stream):
//   a call only enqueues.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

#include "../../include/world_class_c.h"
#include "../../include/world_class_io.h"
#include "wc_morph_rows.hpp"
#include "wc_retime_rows.hpp"
#include "wc_stages.hpp"

using namespace wc;

namespace {

struct MpPair {
	long long a_off, b_off, out_off;  // first source frame of A / of B, first output frame in the packed arrays
	int na, nb;                       // source frames of A / of B
};

struct MpArgs {
	const MpPair *pairs;
	int n_pairs, fs, fft_size;
	const double *pos_a, *pos_b, *w, *wf, *ratio_a, *ratio_b;
	const double *f0_a, *sp_a, *ap_a, *f0_b, *sp_b, *ap_b;
	double *f0_out, *sp_out, *ap_out;
};

template <bool STRETCH>
__global__ __launch_bounds__(RT_T) void morph_kernel(MpArgs A) {
	const int tid = threadIdx.x;
	const long long g = blockIdx.x;
	int lo = 0, hi = A.n_pairs;  // the last pair that starts at or before g (empty ones in front of it share its offset)
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (A.pairs[mid].out_off <= g) lo = mid;
		else hi = mid;
	}
	const MpPair u = A.pairs[lo];
	const int bins = A.fft_size / 2 + 1;
	const RtPlace qa = rt_place(A.pos_a[g], u.na), qb = rt_place(A.pos_b[g], u.nb);
	const double w = A.w[g];
	const bool finite = qa.finite && qb.finite && mp_finite(w);
	const long long ia = u.a_off + qa.i, ja = u.a_off + qa.j, ib = u.b_off + qb.i, jb = u.b_off + qb.j;

	if (A.f0_out && tid == 0) {
		double v = __builtin_nan("");
		if (finite)
			v = mp_f0(rt_f0(A.f0_a[ia], A.f0_a[ja], qa.w0, qa.a), rt_f0(A.f0_b[ib], A.f0_b[jb], qb.w0, qb.a), A.wf ? A.wf[g] : w);
		A.f0_out[g] = v;
	}
	if (A.ap_out) {
		double *__restrict__ out = A.ap_out + g * bins;
		const MpRow pa{A.ap_a + ia * bins, A.ap_a + ja * bins, qa.w0, qa.a}, pb{A.ap_b + ib * bins, A.ap_b + jb * bins, qb.w0, qb.a};
		if (!finite) rt_nan_row(out, bins, tid);
		else mp_ap_row(pa, pb, w, out, bins, tid);
	}
	if (!A.sp_out) return;
	double *__restrict__ out = A.sp_out + g * bins;
	const double ra = STRETCH && A.ratio_a ? A.ratio_a[g] : 0.0, rb = STRETCH && A.ratio_b ? A.ratio_b[g] : 0.0;
	if (!finite || (STRETCH && ((ra != 0.0 && !frame_ratio_valid(ra, A.fft_size)) || (rb != 0.0 && !frame_ratio_valid(rb, A.fft_size))))) {
		rt_nan_row(out, bins, tid);
		return;
	}
	const MpRow sa{A.sp_a + ia * bins, A.sp_a + ja * bins, qa.w0, qa.a}, sb{A.sp_b + ib * bins, A.sp_b + jb * bins, qb.w0, qb.a};
	mp_sp_row<STRETCH>(sa, sb, w, ra, rb, out, A.fs, A.fft_size, tid);
}

// descriptor staging per (device, stream), as for retime: calls on one stream are ordered behind each other, calls on different
// streams never share a buffer.  A few dozen bytes per pair, kept for the life of the process.
std::mutex g_stage_mu;
std::map<std::pair<int, hipStream_t>, Staging *> g_stage;

}  // namespace

const char *wc::morph_check(int fs, int fft_size, int n_pairs, const int *a_length, const int *b_length, const int *out_length,
							long long *total_out) {
	if (!fft_size_supported(fft_size)) return "morph: fft_size must be 512, 1024, 2048 or 4096";
	if (fs <= 0) return "morph: fs must be positive";
	if (n_pairs < 0) return "morph: negative n_pairs";
	if (n_pairs > 0 && (!a_length || !b_length || !out_length)) return "morph: null length array";
	long long ta = 0, tb = 0, to = 0;
	for (int u = 0; u < n_pairs; ++u) {
		if (a_length[u] < 0 || b_length[u] < 0 || out_length[u] < 0) return "morph: negative length";
		if (out_length[u] > 0 && (a_length[u] < 1 || b_length[u] < 1)) return "morph: output frames of a pair with a source without frames";
		ta += a_length[u];
		tb += b_length[u];
		to += out_length[u];
	}
	if (ta > 0xffffffffll || tb > 0xffffffffll || to > 0xffffffffll) return "morph: more than 2^32 - 1 frames";
	*total_out = to;
	return nullptr;
}

int wc::morph_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, int n_pairs, const int *a_length, const double *d_f0_a,
					  const double *d_sp_a, const double *d_ap_a, const int *b_length, const double *d_f0_b, const double *d_sp_b,
					  const double *d_ap_b, const int *out_length, const double *d_position_a, const double *d_position_b,
					  const double *d_weight, const double *d_f0_weight, const double *d_ratio_a, const double *d_ratio_b, double *d_f0_out,
					  double *d_sp_out, double *d_ap_out, long long total_out) {
	if (total_out == 0 || (!d_f0_out && !d_sp_out && !d_ap_out)) return WC_OK;
	Staging *st;
	{
		std::lock_guard<std::mutex> g(g_stage_mu);
		Staging *&slot = g_stage[{dev->id, s}];
		if (!slot) slot = new Staging();
		st = slot;
	}
	int rc;
	const size_t bytes = sizeof(MpPair) * (size_t)n_pairs;
	if ((rc = st->h.reserve(bytes))) return rc;
	if ((rc = st->d.reserve(bytes))) return rc;
	MpPair *h = st->h.as<MpPair>();
	long long fa = 0, fb = 0, fo = 0;
	for (int u = 0; u < n_pairs; ++u) {
		h[u].a_off = fa; h[u].b_off = fb; h[u].out_off = fo; h[u].na = a_length[u]; h[u].nb = b_length[u];
		fa += a_length[u];
		fb += b_length[u];
		fo += out_length[u];
	}
	WC_HIP(hipMemcpyAsync(st->d.p, h, bytes, hipMemcpyHostToDevice, s));
	if ((rc = st->h.mark(s))) return rc;
	MpArgs a;
	a.pairs = st->d.as<MpPair>();
	a.n_pairs = n_pairs; a.fs = fs; a.fft_size = fft_size;
	a.pos_a = d_position_a; a.pos_b = d_position_b; a.w = d_weight; a.wf = d_f0_weight; a.ratio_a = d_ratio_a; a.ratio_b = d_ratio_b;
	a.f0_a = d_f0_a; a.sp_a = d_sp_a; a.ap_a = d_ap_a; a.f0_b = d_f0_b; a.sp_b = d_sp_b; a.ap_b = d_ap_b;
	a.f0_out = d_f0_out; a.sp_out = d_sp_out; a.ap_out = d_ap_out;
	if ((d_ratio_a || d_ratio_b) && d_sp_out) hipLaunchKernelGGL(morph_kernel<true>, dim3((unsigned)total_out), dim3(RT_T), 0, s, a);
	else hipLaunchKernelGGL(morph_kernel<false>, dim3((unsigned)total_out), dim3(RT_T), 0, s, a);
	WC_HIP(hipGetLastError());
	return WC_OK;
}

extern "C" int wc_morph_parameters_device(int fs, int fft_size, int n_pairs, const int *a_length, const double *d_f0_a, const double *d_sp_a,
										  const double *d_ap_a, const int *b_length, const double *d_f0_b, const double *d_sp_b,
										  const double *d_ap_b, const int *out_length, const double *d_position_a, const double *d_position_b,
										  const double *d_weight, const double *d_f0_weight, const double *d_ratio_a, const double *d_ratio_b,
										  double *d_f0_out, double *d_sp_out, double *d_ap_out) {
	long long total_out = 0;
	if (const char *why = morph_check(fs, fft_size, n_pairs, a_length, b_length, out_length, &total_out)) return fail(WC_ERR_INVALID, why);
	const double *const ina[3] = {d_f0_a, d_sp_a, d_ap_a}, *const inb[3] = {d_f0_b, d_sp_b, d_ap_b}, *const out[3] = {d_f0_out, d_sp_out, d_ap_out};
	for (int k = 0; k < 3; ++k) {
		if (!ina[k] != !out[k] || !inb[k] != !out[k]) return fail(WC_ERR_INVALID, "morph: the two inputs and the output of a part must be given or NULL together");
		if (out[k] && (ina[k] == out[k] || inb[k] == out[k]))
			return fail(WC_ERR_INVALID, "morph: in place is not supported (the output must not be one of its inputs)");
	}
	if (total_out > 0 && (!d_position_a || !d_position_b || !d_weight)) return fail(WC_ERR_INVALID, "morph: null position or weight array");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	return morph_enqueue(dev, dev->active(), fs, fft_size, n_pairs, a_length, d_f0_a, d_sp_a, d_ap_a, b_length, d_f0_b, d_sp_b, d_ap_b, out_length,
						 d_position_a, d_position_b, d_weight, d_f0_weight, d_ratio_a, d_ratio_b, d_f0_out, d_sp_out, d_ap_out, total_out);
}
