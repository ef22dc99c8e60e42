// Model features (include/world_class_features.h): continuous log-F0, deltas and MLPG on the device.
//
//   feat_lf0_kernel     one wavefront per utterance walks it in chunks of 64 frames, twice: backwards with a suffix min-scan of the
//                       voiced indices (the least voiced index >= i, carried from chunk to chunk), forwards with a prefix max-scan (the
//                       greatest voiced index <= i) and the interpolation.  Both walks are bounded by the utterance's length: no lane
//                       ever searches for a voiced frame.
//   feat_pack_kernel    a thread per (frame, static column): the static and its deltas from the frame's neighbours, neighbouring
//                       threads on neighbouring columns of a row.
//   mlpg_kernel         a lane per system (utterance, static column), the lanes of a wavefront on neighbouring static columns of one
//                       utterance: the L D L^T sweep in ascending t parks l1, l2 and z / d, the back-substitution reads them in
//                       descending t.  Both loops are bounded by n; both ask for their rows a chunk of frames ahead.
//   feat_unpack_kernel  a thread per (frame, static column).
// Every expression below follows the header's rule operation for operation (the tree is built with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <map>
#include <mutex>

#include "../../include/world_class_features.h"
#include "wc_features_batch.hpp"
#include "wc_features_rows.hpp"
#include "wc_internal.hpp"

using namespace wc;

namespace {

constexpr int kPackFrames = 8;  // frames of one block of feat_pack_kernel
constexpr long long kMaxFrames = 4294967295ll;

__global__ __launch_bounds__(64) void feat_lf0_kernel(const FtUtt *__restrict__ utt, const double *__restrict__ f0, double lf0_fill,
													  double *__restrict__ lf0, int *__restrict__ right) {
	const FtUtt u = utt[blockIdx.x];
	const int n = u.n, lane = threadIdx.x;
	if (n <= 0) return;
	const double *f = f0 + u.f_off;
	double *out = lf0 + u.f_off;
	int *R = right + u.f_off;
	const int chunks = (n + 63) / 64;
	int carry = n;  // n: no voiced frame at or behind
	for (int c = chunks - 1; c >= 0; --c) {
		const int i = c * 64 + lane;
		int m = (i < n && ft_voiced(f[i])) ? i : n;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const int t = __shfl_down(m, o, 64);
			if (lane + o < 64) m = min(m, t);
		}
		m = min(m, carry);
		if (i < n) R[i] = m;
		carry = __shfl(m, 0, 64);
	}
	carry = -1;  // -1: no voiced frame at or before
	for (int c = 0; c < chunks; ++c) {
		const int i = c * 64 + lane;
		int m = (i < n && ft_voiced(f[i])) ? i : -1;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const int t = __shfl_up(m, o, 64);
			if (lane >= o) m = max(m, t);
		}
		m = max(m, carry);
		carry = __shfl(m, 63, 64);
		if (i < n) {
			const int L = m, Rr = R[i];  // (written by this lane in the first walk)
			double v;
			if (L < 0 && Rr >= n) {
				v = lf0_fill;
			} else if (L == i) {
				v = log(f[i]);
			} else if (L < 0) {
				v = log(f[Rr]);
			} else if (Rr >= n) {
				v = log(f[L]);
			} else {
				const double a = (double)(i - L) / (double)(Rr - L);
				const double lo = log(f[L]), hi = log(f[Rr]);
				v = (1.0 - a) * lo + a * hi;
			}
			out[i] = v;
		}
	}
}

template <class T>
__global__ __launch_bounds__(256) void feat_pack_kernel(const FtUtt *__restrict__ utt, int n_utt, long long total, int nd, int n_ap, int orders,
														const double *__restrict__ f0, const double *__restrict__ sp,
														const double *__restrict__ ap, const double *__restrict__ lf0, T *__restrict__ rows) {
	__shared__ int s_t[kPackFrames], s_n[kPackFrames];
	const int tid = threadIdx.x;
	const long long g0 = (long long)blockIdx.x * kPackFrames;
	if (tid < kPackFrames && g0 + tid < total) {
		const long long g = g0 + tid;
		int lo = 0, hi = n_utt - 1;  // the greatest u with f_off <= g: the utterance that holds frame g
		while (lo < hi) {
			const int mid = lo + (hi - lo + 1) / 2;
			if (utt[mid].f_off <= g) lo = mid;
			else hi = mid - 1;
		}
		s_t[tid] = (int)(g - utt[lo].f_off);
		s_n[tid] = utt[lo].n;
	}
	__syncthreads();
	const int S = nd + 1 + n_ap;
	const size_t W = (size_t)orders * S + 1;
	for (int idx = tid; idx < kPackFrames * (S + 1); idx += 256) {
		const int fr = idx / (S + 1), c = idx - fr * (S + 1);
		const long long g = g0 + fr;
		if (g >= total) break;
		T *row = rows + (size_t)g * W;
		if (c == S) {
			row[(size_t)orders * (nd + 1)] = (T)(ft_voiced(f0[g]) ? 1.0 : 0.0);
			continue;
		}
		const int t = s_t[fr], n = s_n[fr];
		int col0, cstep;
		ft_column(c, nd, n_ap, orders, &col0, &cstep);
		const double *x;
		long long stride;
		if (c < nd) { x = sp + (size_t)g * nd + c; stride = nd; }
		else if (c == nd) { x = lf0 + g; stride = 1; }
		else { x = ap + (size_t)g * n_ap + (c - nd - 1); stride = n_ap; }
		const double x0 = x[0];
		row[col0] = (T)x0;
		if (orders >= 2) {
			const double xm = t > 0 ? x[-stride] : 0.0, xp = t + 1 < n ? x[stride] : 0.0;
			row[col0 + cstep] = (T)(0.5 * (xp - xm));
			if (orders == 3) row[col0 + 2 * cstep] = (T)((xm + xp) - 2.0 * x0);
		}
	}
}

struct FtPQ {
	double p0, p1, p2, q0, q1, q2;
};
struct FtRaw {
	double m0, m1, m2, v0, v1, v2;
};
struct FtPark {
	double l1, l2, zd;
};
constexpr int kMlpgChunk = 8;  // frames whose rows a lane of mlpg_kernel asks for ahead of its walk

template <class T>
__global__ __launch_bounds__(64) void mlpg_kernel(const FtUtt *__restrict__ utt, long long block0, int groups, int nd, int n_ap, int orders,
												  const T *__restrict__ mean, const T *__restrict__ var, int var_per_frame,
												  double *__restrict__ park, double *__restrict__ out) {
	const long long b = block0 + blockIdx.x;
	const FtUtt u = utt[b / groups];
	const int n = u.n, S = nd + 1 + n_ap;
	const int c = (int)(b % groups) * 64 + (int)threadIdx.x;
	if (n <= 0 || c > S) return;
	const size_t W = (size_t)orders * S + 1, W1 = (size_t)S + 1;
	const T *M = mean + (size_t)u.f_off * W;
	double *O = out + (size_t)u.f_off * W1;
	if (c == S) {  // vuv: copied through
		for (int t = 0; t < n; ++t) O[(size_t)t * W1 + nd + 1] = (double)M[(size_t)t * W + (size_t)orders * (nd + 1)];
		return;
	}
	int col0, cstep;
	ft_column(c, nd, n_ap, orders, &col0, &cstep);
	const int ocol = c <= nd ? c : c + 1;
	const T *V = var + (var_per_frame ? (size_t)u.f_off * W : 0);
	const size_t vstep = var_per_frame ? W : 0;
	double *P = park + (size_t)u.f_off * 3 * S + c;
	bool bad = false;
	const FtPQ none = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	// A step's arithmetic is short and its rows are a memory latency away, so the rows are asked for a chunk of kMlpgChunk frames
	// ahead of the chunk that is being walked (registers: every index below is a compile-time constant once unrolled).
	auto fetch = [&](int t) {  // the means and variances of frame t; nothing is read beyond the utterance
		FtRaw r = {0.0, 0.0, 0.0, 1.0, 1.0, 1.0};
		if (t < n) {
			const T *m = M + (size_t)t * W + col0, *v = V + (size_t)t * vstep + col0;
			r.m0 = (double)m[0]; r.m1 = (double)m[cstep];
			if (orders == 3) r.m2 = (double)m[2 * cstep];
			if (var_per_frame || t == 0) {  // (one row of variances is read once, at frame 0)
				r.v0 = (double)v[0]; r.v1 = (double)v[cstep];
				if (orders == 3) r.v2 = (double)v[2 * cstep];
			}
		}
		return r;
	};
	// one row of variances for the batch: its precisions are formed once (the same quotients: 1.0 / the same values)
	double g0 = 0.0, g1 = 0.0, g2 = 0.0;
	if (!var_per_frame) {
		const FtRaw w = fetch(0);
		bad = !(w.v0 > 0.0) || !(w.v1 > 0.0) || (orders == 3 && !(w.v2 > 0.0));
		g0 = 1.0 / w.v0;
		g1 = 1.0 / w.v1;
		g2 = orders == 3 ? 1.0 / w.v2 : 0.0;
	}
	auto convert = [&](const FtRaw &w, int t) {  // precisions and weighted means of frame t; zeros outside the utterance
		FtPQ r = none;
		if (t < n) {
			if (var_per_frame) {
				bad = bad || !(w.v0 > 0.0) || !(w.v1 > 0.0) || (orders == 3 && !(w.v2 > 0.0));
				r.p0 = 1.0 / w.v0;
				r.p1 = 1.0 / w.v1;
				if (orders == 3) r.p2 = 1.0 / w.v2;
			} else {
				r.p0 = g0; r.p1 = g1; r.p2 = g2;
			}
			r.q0 = r.p0 == 0.0 ? 0.0 : r.p0 * w.m0;
			r.q1 = r.p1 == 0.0 ? 0.0 : r.p1 * w.m1;
			if (orders == 3) r.q2 = r.p2 == 0.0 ? 0.0 : r.p2 * w.m2;
		}
		return r;
	};
	FtRaw here[kMlpgChunk], ahead[kMlpgChunk];
#pragma unroll
	for (int j = 0; j < kMlpgChunk; ++j) here[j] = fetch(j);
	FtPQ prev = none, cur = convert(here[0], 0), next = none;
	double d1 = 0.0, d2 = 0.0, z1 = 0.0, z2 = 0.0, l1p = 0.0, a1p = 0.0, a2p = 0.0, a2pp = 0.0;
	for (int base = 0; base < n; base += kMlpgChunk) {
#pragma unroll
		for (int j = 0; j < kMlpgChunk; ++j) ahead[j] = fetch(base + kMlpgChunk + j);
#pragma unroll
		for (int j = 0; j < kMlpgChunk; ++j) {
			const int t = base + j;
			if (t >= n) break;
			next = convert(j + 1 < kMlpgChunk ? here[j + 1] : ahead[0], t + 1);
			const double a0 = (cur.p0 + 0.25 * (prev.p1 + next.p1)) + ((prev.p2 + next.p2) + 4.0 * cur.p2);
			const double a1 = t + 1 < n ? -2.0 * (cur.p2 + next.p2) : 0.0;
			const double a2 = t + 2 < n ? next.p2 - 0.25 * next.p1 : 0.0;
			const double r = (cur.q0 + 0.5 * (prev.q1 - next.q1)) + ((prev.q2 + next.q2) - 2.0 * cur.q2);
			double l2 = 0.0, l1 = 0.0, d = a0, z = r;
			if (t >= 2) l2 = a2pp / d2;
			if (t >= 1) {
				double num = a1p;
				if (t >= 2) num = a1p - (l2 * d2) * l1p;
				l1 = num / d1;
			}
			if (t >= 2) d = d - (l2 * l2) * d2;
			if (t >= 1) d = d - (l1 * l1) * d1;
			if (t >= 2) z = z - l2 * z2;
			if (t >= 1) z = z - l1 * z1;
			double *pk = P + (size_t)t * 3 * S;
			pk[0] = l1;
			pk[S] = l2;
			pk[2 * (size_t)S] = z / d;
			d2 = d1; d1 = d; z2 = z1; z1 = z; l1p = l1;
			a2pp = a2p; a2p = a2; a1p = a1;
			prev = cur; cur = next;
		}
#pragma unroll
		for (int j = 0; j < kMlpgChunk; ++j) here[j] = ahead[j];
	}
	// back: the parked l1(t), l2(t) and z(t) / d(t) of frames top, top - 1, ..., asked for a chunk ahead in the same way
	auto parked = [&](int t) {
		FtPark r = {0.0, 0.0, 0.0};
		if (t >= 0) {
			const double *pk = P + (size_t)t * 3 * S;
			r.l1 = pk[0]; r.l2 = pk[S]; r.zd = pk[2 * (size_t)S];
		}
		return r;
	};
	FtPark back[kMlpgChunk], before[kMlpgChunk];
#pragma unroll
	for (int j = 0; j < kMlpgChunk; ++j) back[j] = parked(n - 1 - j);
	double c1 = 0.0, c2 = 0.0, l1n = 0.0, l2n = 0.0, l2nn = 0.0;  // c(t+1), c(t+2), l1(t+1), l2(t+1), l2(t+2)
	const double nan = __longlong_as_double(0x7ff8000000000000ll);
	for (int top = n - 1; top >= 0; top -= kMlpgChunk) {
#pragma unroll
		for (int j = 0; j < kMlpgChunk; ++j) before[j] = parked(top - kMlpgChunk - j);
#pragma unroll
		for (int j = 0; j < kMlpgChunk; ++j) {
			const int t = top - j;
			if (t < 0) break;
			double x = back[j].zd;
			if (t + 1 < n) x = x - l1n * c1;
			if (t + 2 < n) x = x - l2nn * c2;
			O[(size_t)t * W1 + ocol] = bad ? nan : x;
			c2 = c1; c1 = x; l2nn = l2n; l2n = back[j].l2; l1n = back[j].l1;
		}
#pragma unroll
		for (int j = 0; j < kMlpgChunk; ++j) back[j] = before[j];
	}
}

template <class T>
__global__ __launch_bounds__(256) void feat_unpack_kernel(long long n_frames, int nd, int n_ap, int orders, const T *__restrict__ rows,
														  double vuv_threshold, double *__restrict__ f0, double *__restrict__ sp,
														  double *__restrict__ ap) {
	const int S = nd + 1 + n_ap;
	const size_t W = (size_t)orders * S + 1;
	const unsigned long long work = (unsigned long long)n_frames * S;
	for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < work; i += (unsigned long long)gridDim.x * 256) {
		const unsigned long long g = i / S;
		const int c = (int)(i - g * S);
		const T *row = rows + (size_t)g * W;
		if (c < nd) {
			if (sp) sp[(size_t)g * nd + c] = (double)row[c];
		} else if (c == nd) {
			if (f0) {
				const double vuv = (double)row[(size_t)orders * (nd + 1)];
				f0[g] = vuv > vuv_threshold ? exp((double)row[(size_t)orders * nd]) : 0.0;
			}
		} else if (ap) {
			const int bnd = c - nd - 1;
			ap[(size_t)g * n_ap + bnd] = (double)row[(size_t)orders * (nd + 1) + 1 + bnd];
		}
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
std::mutex g_stage_mu;
std::map<std::pair<int, hipStream_t>, Staging *> g_stage;  // the utterance descriptors' way up, per (device, stream)

long long width_of(int nd, int n_ap, int orders) {
	if (nd < 1 || n_ap < 0 || orders < 1 || orders > 3) return -1;
	const long long w = (long long)orders * ((long long)nd + 1 + n_ap) + 1;
	return w > 0x7fffffffll ? -1 : w;
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

namespace wc {

// the shape arguments every call shares; *total: the frames of the batch
int ft_check_shape(const char *who, int n_utt, const int *lengths, int nd, int n_ap, int orders, int orders_min, int format, long long *total) {
	const std::string w(who);
	if (nd < 1 || n_ap < 0) return fail(WC_ERR_INVALID, w + ": nd must be at least 1 and n_ap not negative");
	if (orders < orders_min || orders > 3) return fail(WC_ERR_INVALID, w + ": orders out of range");
	if (width_of(nd, n_ap, orders) < 0) return fail(WC_ERR_INVALID, w + ": the row width leaves 31 bits");
	if (format != WC_FEAT_F64 && format != WC_FEAT_F32) return fail(WC_ERR_INVALID, w + ": the format is 0 (double) or 1 (float)");
	if (n_utt < 0) return fail(WC_ERR_INVALID, w + ": a negative utterance count");
	if (n_utt > 0 && !lengths) return fail(WC_ERR_INVALID, w + ": null length array");
	long long sum = 0;
	for (int u = 0; u < n_utt; ++u) {
		if (lengths[u] < 0) return fail(WC_ERR_INVALID, w + ": a negative length");
		sum += lengths[u];
		if (sum > kMaxFrames) return fail(WC_ERR_INVALID, w + ": more than 2^32 - 1 frames in one call");
	}
	*total = sum;
	return WC_OK;
}

// the descriptors on the device and the scratch reserved, both handed to stream s
int ft_prepare(Device *dev, hipStream_t s, int n_utt, const int *lengths, size_t scratch_bytes, const FtUtt **d_utt) {
	Staging *st;
	{
		std::lock_guard<std::mutex> g(g_stage_mu);
		Staging *&slot = g_stage[{dev->id, s}];
		if (!slot) slot = new Staging();
		st = slot;
	}
	int rc;
	const size_t bytes = sizeof(FtUtt) * (size_t)n_utt;
	if ((rc = st->h.reserve(bytes))) return rc;
	if ((rc = st->d.reserve(bytes))) return rc;
	FtUtt *h = st->h.as<FtUtt>();
	long long off = 0;
	for (int u = 0; u < n_utt; ++u) {
		h[u].f_off = off;
		h[u].n = lengths[u];
		h[u].pad = 0;
		off += lengths[u];
	}
	if (scratch_bytes > dev->features_scratch.cap) {
		dev->quiesce();  // an earlier call's kernels may still use the buffer that is about to go
		if ((rc = dev->features_scratch.reserve(scratch_bytes))) return rc;
	}
	if (!dev->features_done) WC_HIP(hipEventCreateWithFlags(&dev->features_done, hipEventDisableTiming));
	else if (dev->features_last != s) WC_HIP(hipStreamWaitEvent(s, dev->features_done, 0));
	WC_HIP(hipMemcpyAsync(st->d.p, h, bytes, hipMemcpyHostToDevice, s));
	if ((rc = st->h.mark(s))) return rc;
	*d_utt = st->d.as<FtUtt>();
	return WC_OK;
}

int ft_finish(Device *dev, hipStream_t s) {
	WC_HIP(hipEventRecord(dev->features_done, s));
	dev->features_last = s;
	return WC_OK;
}

}  // namespace wc

extern "C" {

int wc_model_feature_width(int nd, int n_ap, int orders) { return (int)width_of(nd, n_ap, orders); }

int wc_pack_model_features_device(int n_utt, const int *lengths, int nd, int n_ap, int orders, const double *d_f0, const double *d_coded_sp,
								  const double *d_coded_ap, double lf0_fill, int out_format, void *d_rows) {
	long long total = 0;
	int rc;
	if ((rc = ft_check_shape("pack model features", n_utt, lengths, nd, n_ap, orders, 1, out_format, &total))) return rc;
	if (lf0_fill != lf0_fill) return fail(WC_ERR_INVALID, "pack model features: lf0_fill is NaN");
	if (total == 0) return WC_OK;
	if ((n_ap == 0) != (d_coded_ap == nullptr)) return fail(WC_ERR_INVALID, "pack model features: d_coded_ap is NULL exactly where n_ap is 0");
	if (!d_f0 || !d_coded_sp || !d_rows) return fail(WC_ERR_INVALID, "pack model features: null array");
	const unsigned long long W = (unsigned long long)width_of(nd, n_ap, orders), esz = out_format == WC_FEAT_F32 ? 4 : 8;
	const unsigned long long out_bytes = (unsigned long long)total * W * esz;
	if (overlap(d_rows, out_bytes, d_f0, 8ull * total) || overlap(d_rows, out_bytes, d_coded_sp, 8ull * total * nd) ||
		overlap(d_rows, out_bytes, d_coded_ap, 8ull * total * n_ap))
		return fail(WC_ERR_INVALID, "pack model features: d_rows overlaps an input");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	const size_t lf0_bytes = round_up((size_t)total * sizeof(double), 16);
	const FtUtt *d_utt = nullptr;
	if ((rc = ft_prepare(dev, s, n_utt, lengths, lf0_bytes + (size_t)total * sizeof(int), &d_utt))) return rc;
	double *lf0 = dev->features_scratch.as<double>();
	int *right = reinterpret_cast<int *>(dev->features_scratch.as<char>() + lf0_bytes);
	if ((rc = dev->time_begin("feat_lf0_kernel", s))) return rc;
	hipLaunchKernelGGL(feat_lf0_kernel, dim3((unsigned)n_utt), dim3(64), 0, s, d_utt, d_f0, lf0_fill, lf0, right);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("feat_lf0_kernel", s))) return rc;
	const unsigned blocks = (unsigned)((total + kPackFrames - 1) / kPackFrames);
	if ((rc = dev->time_begin("feat_pack_kernel", s))) return rc;
	if (out_format == WC_FEAT_F32)
		hipLaunchKernelGGL(feat_pack_kernel<float>, dim3(blocks), dim3(256), 0, s, d_utt, n_utt, total, nd, n_ap, orders, d_f0, d_coded_sp,
						   d_coded_ap, (const double *)lf0, static_cast<float *>(d_rows));
	else
		hipLaunchKernelGGL(feat_pack_kernel<double>, dim3(blocks), dim3(256), 0, s, d_utt, n_utt, total, nd, n_ap, orders, d_f0, d_coded_sp,
						   d_coded_ap, (const double *)lf0, static_cast<double *>(d_rows));
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("feat_pack_kernel", s))) return rc;
	return ft_finish(dev, s);
}

int wc_mlpg_device(int n_utt, const int *lengths, int nd, int n_ap, int orders, int in_format, const void *d_mean, const void *d_var,
				   int var_per_frame, double *d_static) {
	long long total = 0;
	int rc;
	if ((rc = ft_check_shape("mlpg", n_utt, lengths, nd, n_ap, orders, 2, in_format, &total))) return rc;
	if (var_per_frame != 0 && var_per_frame != 1) return fail(WC_ERR_INVALID, "mlpg: var_per_frame is 0 or 1");
	if (total == 0) return WC_OK;
	if (!d_mean || !d_var || !d_static) return fail(WC_ERR_INVALID, "mlpg: null array");
	const unsigned long long W = (unsigned long long)width_of(nd, n_ap, orders), esz = in_format == WC_FEAT_F32 ? 4 : 8;
	const unsigned long long S = (unsigned long long)nd + 1 + n_ap, out_bytes = 8ull * total * (S + 1);
	if (overlap(d_static, out_bytes, d_mean, (unsigned long long)total * W * esz) ||
		overlap(d_static, out_bytes, d_var, (var_per_frame ? (unsigned long long)total : 1ull) * W * esz))
		return fail(WC_ERR_INVALID, "mlpg: d_static overlaps an input");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	const FtUtt *d_utt = nullptr;
	if ((rc = ft_prepare(dev, s, n_utt, lengths, (size_t)total * 3 * S * sizeof(double), &d_utt))) return rc;
	double *park = dev->features_scratch.as<double>();
	const int groups = (int)((S + 1 + 63) / 64);
	const long long blocks = (long long)n_utt * groups, per_launch = 1ll << 30;
	if ((rc = dev->time_begin("mlpg_kernel", s))) return rc;
	for (long long b0 = 0; b0 < blocks; b0 += per_launch) {
		const unsigned nb = (unsigned)(blocks - b0 < per_launch ? blocks - b0 : per_launch);
		if (in_format == WC_FEAT_F32)
			hipLaunchKernelGGL(mlpg_kernel<float>, dim3(nb), dim3(64), 0, s, d_utt, b0, groups, nd, n_ap, orders, static_cast<const float *>(d_mean),
							   static_cast<const float *>(d_var), var_per_frame, park, d_static);
		else
			hipLaunchKernelGGL(mlpg_kernel<double>, dim3(nb), dim3(64), 0, s, d_utt, b0, groups, nd, n_ap, orders, static_cast<const double *>(d_mean),
							   static_cast<const double *>(d_var), var_per_frame, park, d_static);
		WC_HIP(hipGetLastError());
	}
	if ((rc = dev->time_end("mlpg_kernel", s))) return rc;
	return ft_finish(dev, s);
}

int wc_unpack_model_features_device(long long n_frames, int nd, int n_ap, int orders, int in_format, const void *d_rows, double vuv_threshold,
									double *d_f0, double *d_coded_sp, double *d_coded_ap) {
	if (nd < 1 || n_ap < 0) return fail(WC_ERR_INVALID, "unpack model features: nd must be at least 1 and n_ap not negative");
	if (orders < 1 || orders > 3) return fail(WC_ERR_INVALID, "unpack model features: orders out of range");
	if (width_of(nd, n_ap, orders) < 0) return fail(WC_ERR_INVALID, "unpack model features: the row width leaves 31 bits");
	if (in_format != WC_FEAT_F64 && in_format != WC_FEAT_F32) return fail(WC_ERR_INVALID, "unpack model features: the format is 0 (double) or 1 (float)");
	if (n_frames < 0) return fail(WC_ERR_INVALID, "unpack model features: a negative frame count");
	if (n_frames > kMaxFrames) return fail(WC_ERR_INVALID, "unpack model features: more than 2^32 - 1 frames in one call");
	if (vuv_threshold != vuv_threshold) return fail(WC_ERR_INVALID, "unpack model features: vuv_threshold is NaN");
	if (n_ap == 0 && d_coded_ap) return fail(WC_ERR_INVALID, "unpack model features: d_coded_ap is NULL where n_ap is 0");
	if (n_frames == 0 || (!d_f0 && !d_coded_sp && !d_coded_ap)) return WC_OK;
	if (!d_rows) return fail(WC_ERR_INVALID, "unpack model features: null rows");
	const unsigned long long W = (unsigned long long)width_of(nd, n_ap, orders), esz = in_format == WC_FEAT_F32 ? 4 : 8;
	const unsigned long long in_bytes = (unsigned long long)n_frames * W * esz, n = (unsigned long long)n_frames;
	if (overlap(d_rows, in_bytes, d_f0, 8ull * n) || overlap(d_rows, in_bytes, d_coded_sp, 8ull * n * nd) ||
		overlap(d_rows, in_bytes, d_coded_ap, 8ull * n * n_ap))
		return fail(WC_ERR_INVALID, "unpack model features: an output overlaps d_rows");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	const unsigned long long work = n * ((unsigned long long)nd + 1 + n_ap), want = (work + 255) / 256;
	const unsigned blocks = (unsigned)(want < (1ull << 20) ? want : (1ull << 20));
	int rc;
	if ((rc = dev->time_begin("feat_unpack_kernel", s))) return rc;
	if (in_format == WC_FEAT_F32)
		hipLaunchKernelGGL(feat_unpack_kernel<float>, dim3(blocks), dim3(256), 0, s, n_frames, nd, n_ap, orders, static_cast<const float *>(d_rows),
						   vuv_threshold, d_f0, d_coded_sp, d_coded_ap);
	else
		hipLaunchKernelGGL(feat_unpack_kernel<double>, dim3(blocks), dim3(256), 0, s, n_frames, nd, n_ap, orders, static_cast<const double *>(d_rows),
						   vuv_threshold, d_f0, d_coded_sp, d_coded_ap);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("feat_unpack_kernel", s))) return rc;
	return WC_OK;
}

}  // extern "C"
