// Global-variance parameter generation behind MLPG (include/world_class_gv.h).
//
//   gv_system_kernel  the banded system a0, a1, a2, r of the MLPG rule, once per call, [plane][system][frame] in scratch: a block of
//                     256 threads forms a tile of 64 frames x 16 static columns with neighbouring threads on neighbouring columns of a
//                     model row (the reads follow the rows), parks it in LDS and writes it with neighbouring threads on neighbouring
//                     frames (the writes follow the planes).
//   gv_refine_kernel  one wavefront per system (utterance, static column), frame t on lane t mod 64 -- the order THE sum fixes.  The
//                     trajectory c and d (then g) stand in LDS up to kGvLdsFrames frames and in two more scratch planes beyond; the
//                     whole iteration loop runs here; the mask of an LDS-resident utterance is read once, a bit per frame in a
//                     register of its lane.  A switched-off column and N < 2 leave at once.
//   gv_stats_kernel   the stat pass alone, the same device function on the rows as they stand.
// No atomics, no reduction across wavefronts, every loop bounded by n and max_iter.  Every expression follows the header's rule
// operation for operation (the tree is built with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "../../include/world_class_gv.h"
#include "wc_features_batch.hpp"
#include "wc_features_rows.hpp"
#include "wc_internal.hpp"

using namespace wc;

namespace {

constexpr int kGvLdsFrames = 2048;  // the longest utterance whose c and d stand in LDS: 2 x 8 bytes a frame, 32 KiB a wavefront
constexpr int kSysF = 64, kSysC = 16;  // frames and static columns of one tile of gv_system_kernel
constexpr int kMaxIter = 64;

struct GvPQ {
	double p0, p1, p2, q0, q1, q2;
};

template <class T>
__global__ __launch_bounds__(256) void gv_system_kernel(const FtUtt *__restrict__ utt, long long block0, int ctiles, int ftiles, int nd, int n_ap,
														 int orders, const T *__restrict__ mean, const T *__restrict__ var, int var_per_frame,
														 size_t plane, double *__restrict__ sys) {
	__shared__ double tile[4][kSysC][kSysF + 1];
	const long long b = block0 + blockIdx.x;
	const int ft = (int)(b % ftiles);
	const long long rest = b / ftiles;
	const int ct = (int)(rest % ctiles);
	const FtUtt u = utt[rest / ctiles];
	const int n = u.n, S = nd + 1 + n_ap, t0 = ft * kSysF, c0 = ct * kSysC, tid = threadIdx.x;
	if (t0 >= n) return;  // (the whole block)
	const size_t W = (size_t)orders * S + 1;
	const T *M = mean + (size_t)u.f_off * W;
	const T *V = var + (var_per_frame ? (size_t)u.f_off * W : 0);
	const size_t vstep = var_per_frame ? W : 0;
#pragma unroll
	for (int i = 0; i < kSysF * kSysC / 256; ++i) {
		const int idx = tid + 256 * i, cc = idx % kSysC, ff = idx / kSysC;
		const unsigned t = (unsigned)t0 + ff;  // (unsigned: t0 + 63 and t + 2 may pass 2^31 - 1)
		const int c = c0 + cc;
		if (t >= (unsigned)n || c >= S) continue;
		int col0, cstep;
		ft_column(c, nd, n_ap, orders, &col0, &cstep);
		auto pq = [&](long long s) {  // precisions and weighted means of frame s; zeros outside the utterance
			GvPQ w = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
			if (s >= 0 && s < n) {
				const T *m = M + (size_t)s * W + col0, *v = V + (size_t)s * vstep + col0;
				w.p0 = 1.0 / (double)v[0];
				w.p1 = 1.0 / (double)v[cstep];
				w.q0 = w.p0 == 0.0 ? 0.0 : w.p0 * (double)m[0];
				w.q1 = w.p1 == 0.0 ? 0.0 : w.p1 * (double)m[cstep];
				if (orders == 3) {
					w.p2 = 1.0 / (double)v[2 * cstep];
					w.q2 = w.p2 == 0.0 ? 0.0 : w.p2 * (double)m[2 * cstep];
				}
			}
			return w;
		};
		const GvPQ prev = pq((long long)t - 1), cur = pq(t), next = pq((long long)t + 1);
		tile[0][cc][ff] = (cur.p0 + 0.25 * (prev.p1 + next.p1)) + ((prev.p2 + next.p2) + 4.0 * cur.p2);
		tile[1][cc][ff] = t + 1 < (unsigned)n ? -2.0 * (cur.p2 + next.p2) : 0.0;
		tile[2][cc][ff] = t + 2 < (unsigned)n ? next.p2 - 0.25 * next.p1 : 0.0;
		tile[3][cc][ff] = (cur.q0 + 0.5 * (prev.q1 - next.q1)) + ((prev.q2 + next.q2) - 2.0 * cur.q2);
	}
	__syncthreads();
	double *out = sys + (size_t)u.f_off * S;
#pragma unroll 4
	for (int i = 0; i < 4 * kSysF * kSysC / 256; ++i) {
		const int idx = tid + 256 * i, ff = idx % kSysF, row = idx / kSysF;
		const int k = row / kSysC, cc = row % kSysC;
		const unsigned t = (unsigned)t0 + ff;
		const int c = c0 + cc;
		if (t < (unsigned)n && c < S) out[(size_t)k * plane + (size_t)c * n + t] = tile[k][cc][ff];
	}
}

// the butterfly of THE sum over the 64 lane partials: every lane ends with the same bits
__device__ __forceinline__ double gv_sum(double p) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
	return p;
}

// N: the count of masked frames, the same in every lane
__device__ __forceinline__ double gv_count(const unsigned char *mask, int n) {
	if (!mask) return (double)n;
	int k = 0;
	for (unsigned t = threadIdx.x; t < (unsigned)n; t += 64) k += mask[t] != 0;
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) k += __shfl_xor(k, off, 64);
	return (double)k;
}

// whether frame t counts: the mask's bytes as they lie, or -- for an utterance that fits the LDS copy -- one bit per frame of this lane
// (frame t = lane + 64 j stands at bit j), read once instead of in every pass
struct GvMaskBytes {
	const unsigned char *m;
	__device__ __forceinline__ bool operator()(unsigned t) const { return !m || m[t]; }
};
struct GvMaskBits {
	unsigned bits;
	__device__ __forceinline__ bool operator()(unsigned t) const { return (bits >> (t >> 6)) & 1u; }
};
static_assert(kGvLdsFrames <= 64 * 32, "a lane's frames of the LDS copy fit the bits of GvMaskBits");

// stat(c) of the header: c(t) at c[t * cs]; with kStore d(t) goes to d[t]
template <bool kStore, class Mask>
__device__ __forceinline__ void gv_stat(const double *c, size_t cs, const Mask on, int n, double N, double *d, double *mean_out,
										double *v_out) {
	const unsigned lane = threadIdx.x;  // (unsigned frame indices: t + 64 may pass 2^31 - 1)
	double p = 0.0;
	for (unsigned t = lane; t < (unsigned)n; t += 64) p = p + (on(t) ? c[(size_t)t * cs] : 0.0);
	const double mean = gv_sum(p) / N;
	p = 0.0;
	for (unsigned t = lane; t < (unsigned)n; t += 64) {
		const double dt = on(t) ? c[(size_t)t * cs] - mean : 0.0;
		if (kStore) d[t] = dt;
		p = p + dt * dt;
	}
	*mean_out = mean;
	*v_out = gv_sum(p) / N;
}

struct GvParams {
	double w_ml, w_gv, step_init;
	int max_iter, orders;
};

// the start and the iterations of one system; cb, db: n doubles each, in LDS or in scratch (the compiler follows the address space
// into each of the two calls).  O: the system's column of the static rows, W1 doubles from frame to frame.
template <class Mask>
__device__ __forceinline__ void gv_refine(double *cb, double *db, double *O, size_t W1, const Mask on, int n, double N, double gm,
										  double gvv, const double *__restrict__ a0, const double *__restrict__ a1, const double *__restrict__ a2,
										  const double *__restrict__ r, const GvParams P) {
	const int lane = threadIdx.x;
	for (unsigned t = lane; t < (unsigned)n; t += 64) cb[t] = O[(size_t)t * W1];
	double mean, v;
	gv_stat<true>(cb, 1, on, n, N, db, &mean, &v);
	if (!(v > 0.0)) return;
	const double ratio = sqrt(gm / v);
	for (unsigned t = lane; t < (unsigned)n; t += 64)
		if (on(t)) cb[t] = ratio * db[t] + mean;
	const double pv = 1.0 / gvv, omega = P.w_ml / (double)((long long)P.orders * n);
	const double kh = P.w_gv * (2.0 / (N * N)), kg = P.w_gv * (2.0 / N), n1pv = (N - 1.0) * pv, tpv = 2.0 * pv;
	double step = P.step_init, J_prev = 0.0;
	for (int it = 1; it <= P.max_iter; ++it) {
		__syncthreads();  // the c of the step before, written by the lanes of its frames, is read by their neighbours
		gv_stat<true>(cb, 1, on, n, N, db, &mean, &v);
		const double e = v - gm;
		const double he = n1pv * e, ge = kg * (pv * e);
		double p = 0.0;
		for (unsigned t = lane; t < (unsigned)n; t += 64) {
			const double m2 = t >= 2 ? a2[t - 2] * cb[t - 2] : 0.0, m1 = t >= 1 ? a1[t - 1] * cb[t - 1] : 0.0;
			const double p1 = t + 1 < (unsigned)n ? a1[t] * cb[t + 1] : 0.0, p2 = t + 2 < (unsigned)n ? a2[t] * cb[t + 2] : 0.0;
			const double ct = cb[t], dt = db[t], rt = r[t], a0t = a0[t];
			const double Ac = ((m2 + m1) + a0t * ct) + (p1 + p2);
			p = p + ct * (rt - 0.5 * Ac);
			const double h = omega * a0t + kh * (he + tpv * (dt * dt));
			db[t] = (omega * (rt - Ac) - ge * dt) / h;  // g(t) takes d(t)'s place: only this lane reads either
		}
		const double J = omega * gv_sum(p) - (0.5 * P.w_gv) * ((e * e) * pv);
		if (it > 1) {
			if (J < J_prev) step = step * 0.5;
			if (J > J_prev) step = step * 1.2;
		}
		__syncthreads();  // every neighbour has read the c of this step
		for (unsigned t = lane; t < (unsigned)n; t += 64)
			if (on(t)) cb[t] = cb[t] + step * db[t];
		J_prev = J;
	}
	for (unsigned t = lane; t < (unsigned)n; t += 64)
		if (on(t)) O[(size_t)t * W1] = cb[t];
}

__global__ __launch_bounds__(64) void gv_refine_kernel(const FtUtt *__restrict__ utt, long long block0, int nd, int n_ap, const double *__restrict__ gv_mean,
													   const double *__restrict__ gv_var, const unsigned char *__restrict__ d_mask, GvParams P,
													   int lds_frames, size_t plane, double *__restrict__ sys, double *out) {
	extern __shared__ __attribute__((aligned(16))) double gv_lds[];
	const int S = nd + 1 + n_ap;
	const long long b = block0 + blockIdx.x;
	const FtUtt u = utt[b / S];
	const int c = (int)(b % S), n = u.n, lane = threadIdx.x;
	if (n <= 0) return;
	const double gm = gv_mean[c], gvv = gv_var[c];
	if (gvv == INFINITY) return;  // switched off
	const size_t W1 = (size_t)S + 1;
	double *O = out + (size_t)u.f_off * W1 + (c <= nd ? c : c + 1);
	const unsigned char *mask = d_mask ? d_mask + u.f_off : nullptr;
	if (!(gvv > 0.0) || !(gm > 0.0) || gm == INFINITY) {
		const double nan = __longlong_as_double(0x7ff8000000000000ll);
		for (unsigned t = lane; t < (unsigned)n; t += 64)
			if (!mask || mask[t]) O[(size_t)t * W1] = nan;
		return;
	}
	const double N = gv_count(mask, n);
	if (N < 2.0) return;
	const size_t at = (size_t)u.f_off * S + (size_t)c * n;  // this system in a plane
	const double *a0 = sys + at, *a1 = a0 + plane, *a2 = a1 + plane, *r = a2 + plane;
	if (n <= lds_frames) {
		GvMaskBits on = {~0u};
		if (mask) {
			on.bits = 0u;
			for (unsigned t = lane, j = 0; t < (unsigned)n; t += 64, ++j) on.bits |= (unsigned)(mask[t] != 0) << j;
		}
		gv_refine(gv_lds, gv_lds + lds_frames, O, W1, on, n, N, gm, gvv, a0, a1, a2, r, P);
	} else {
		gv_refine(sys + 4 * plane + at, sys + 5 * plane + at, O, W1, GvMaskBytes{mask}, n, N, gm, gvv, a0, a1, a2, r, P);
	}
}

__global__ __launch_bounds__(64) void gv_stats_kernel(const FtUtt *__restrict__ utt, long long block0, int nd, int S, const double *__restrict__ rows,
													  const unsigned char *__restrict__ d_mask, double *__restrict__ mean_out,
													  double *__restrict__ var_out) {
	const long long b = block0 + blockIdx.x;
	const FtUtt u = utt[b / S];
	const int c = (int)(b % S), n = u.n < 0 ? 0 : u.n;
	const size_t W1 = (size_t)S + 1;
	const unsigned char *mask = d_mask ? d_mask + u.f_off : nullptr;
	const double N = gv_count(mask, n);
	double mean, v;
	gv_stat<false>(rows + (size_t)u.f_off * W1 + (c <= nd ? c : c + 1), W1, GvMaskBytes{mask}, n, N, nullptr, &mean, &v);
	if (threadIdx.x == 0) {
		mean_out[b] = mean;
		var_out[b] = v;
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int longest_of(int n_utt, const int *lengths) {
	int most = 0;
	for (int u = 0; u < n_utt; ++u) most = lengths[u] > most ? lengths[u] : most;
	return most;
}

bool weight_ok(double x) { return x >= 0.0 && x <= DBL_MAX; }  // not NaN, not negative, not infinite

}  // namespace

extern "C" {

int wc_gv_stats_device(int n_utt, const int *lengths, int nd, int n_ap, const double *d_static, const unsigned char *d_mask, double *d_mean_out,
					   double *d_var_out) {
	long long total = 0;
	int rc;
	if ((rc = ft_check_shape("gv stats", n_utt, lengths, nd, n_ap, 1, 1, WC_FEAT_F64, &total))) return rc;
	if (n_utt == 0) return WC_OK;
	if (!d_mean_out || !d_var_out || (total > 0 && !d_static)) return fail(WC_ERR_INVALID, "gv stats: null array");
	const unsigned long long S = (unsigned long long)nd + 1 + n_ap, in_bytes = 8ull * total * (S + 1), out_bytes = 8ull * n_utt * S;
	if (overlap(d_mean_out, out_bytes, d_var_out, out_bytes)) return fail(WC_ERR_INVALID, "gv stats: the two outputs overlap");
	if (overlap(d_mean_out, out_bytes, d_static, in_bytes) || overlap(d_var_out, out_bytes, d_static, in_bytes) ||
		overlap(d_mean_out, out_bytes, d_mask, total) || overlap(d_var_out, out_bytes, d_mask, total))
		return fail(WC_ERR_INVALID, "gv stats: an output overlaps an input");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	const FtUtt *d_utt = nullptr;
	if ((rc = ft_prepare(dev, s, n_utt, lengths, 0, &d_utt))) return rc;
	const long long blocks = (long long)n_utt * (long long)S, per_launch = 1ll << 30;
	if ((rc = dev->time_begin("gv_stats_kernel", s))) return rc;
	for (long long b0 = 0; b0 < blocks; b0 += per_launch) {
		const unsigned nb = (unsigned)(blocks - b0 < per_launch ? blocks - b0 : per_launch);
		hipLaunchKernelGGL(gv_stats_kernel, dim3(nb), dim3(64), 0, s, d_utt, b0, nd, (int)S, d_static, d_mask, d_mean_out, d_var_out);
		WC_HIP(hipGetLastError());
	}
	if ((rc = dev->time_end("gv_stats_kernel", s))) return rc;
	return ft_finish(dev, s);
}

int wc_mlpg_gv_device(int n_utt, const int *lengths, int nd, int n_ap, int orders, int in_format, const void *d_mean, const void *d_var,
					  int var_per_frame, const double *d_gv_mean, const double *d_gv_var, const unsigned char *d_mask, double w_ml, double w_gv,
					  double step_init, int max_iter, double *d_static) {
	long long total = 0;
	int rc;
	if ((rc = ft_check_shape("mlpg gv", n_utt, lengths, nd, n_ap, orders, 2, in_format, &total))) return rc;
	if (var_per_frame != 0 && var_per_frame != 1) return fail(WC_ERR_INVALID, "mlpg gv: var_per_frame is 0 or 1");
	if (max_iter < 0 || max_iter > kMaxIter) return fail(WC_ERR_INVALID, "mlpg gv: max_iter is 0 .. 64");
	if (!weight_ok(w_ml) || !weight_ok(w_gv) || !weight_ok(step_init))
		return fail(WC_ERR_INVALID, "mlpg gv: w_ml, w_gv and step_init are finite and not negative");
	if (w_ml == 0.0) return fail(WC_ERR_INVALID, "mlpg gv: w_ml is 0");
	if (total == 0) return WC_OK;
	if (!d_gv_mean || !d_gv_var || !d_static || (max_iter > 0 && (!d_mean || !d_var))) return fail(WC_ERR_INVALID, "mlpg gv: null array");
	const unsigned long long S = (unsigned long long)nd + 1 + n_ap, W = (unsigned long long)orders * S + 1, esz = in_format == WC_FEAT_F32 ? 4 : 8;
	const unsigned long long out_bytes = 8ull * total * (S + 1);
	if (overlap(d_static, out_bytes, d_mean, (unsigned long long)total * W * esz) ||
		overlap(d_static, out_bytes, d_var, (var_per_frame ? (unsigned long long)total : 1ull) * W * esz) ||
		overlap(d_static, out_bytes, d_gv_mean, 8ull * S) || overlap(d_static, out_bytes, d_gv_var, 8ull * S) ||
		overlap(d_static, out_bytes, d_mask, total))
		return fail(WC_ERR_INVALID, "mlpg gv: d_static overlaps an input");
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	const int longest = longest_of(n_utt, lengths);
	const size_t plane = (size_t)total * S;
	const int planes = longest > kGvLdsFrames ? 6 : (max_iter > 0 ? 4 : 0);  // c and d of the long ones; the start alone reads no system
	const FtUtt *d_utt = nullptr;
	if ((rc = ft_prepare(dev, s, n_utt, lengths, (size_t)planes * plane * sizeof(double), &d_utt))) return rc;
	double *sys = dev->features_scratch.as<double>();
	const long long per_launch = 1ll << 30;
	if (max_iter > 0) {
		const int ctiles = (int)((S + kSysC - 1) / kSysC), ftiles = (int)(((long long)longest + kSysF - 1) / kSysF);
		const long long blocks = (long long)n_utt * ctiles * ftiles;
		if ((rc = dev->time_begin("gv_system_kernel", s))) return rc;
		for (long long b0 = 0; b0 < blocks; b0 += per_launch) {
			const unsigned nb = (unsigned)(blocks - b0 < per_launch ? blocks - b0 : per_launch);
			if (in_format == WC_FEAT_F32)
				hipLaunchKernelGGL(gv_system_kernel<float>, dim3(nb), dim3(256), 0, s, d_utt, b0, ctiles, ftiles, nd, n_ap, orders,
								   static_cast<const float *>(d_mean), static_cast<const float *>(d_var), var_per_frame, plane, sys);
			else
				hipLaunchKernelGGL(gv_system_kernel<double>, dim3(nb), dim3(256), 0, s, d_utt, b0, ctiles, ftiles, nd, n_ap, orders,
								   static_cast<const double *>(d_mean), static_cast<const double *>(d_var), var_per_frame, plane, sys);
			WC_HIP(hipGetLastError());
		}
		if ((rc = dev->time_end("gv_system_kernel", s))) return rc;
	}
	const int lds_frames = longest >= kGvLdsFrames ? kGvLdsFrames : (longest + 63) / 64 * 64;
	const GvParams P = {w_ml, w_gv, step_init, max_iter, orders};
	const long long blocks = (long long)n_utt * (long long)S;
	if ((rc = dev->time_begin("gv_refine_kernel", s))) return rc;
	for (long long b0 = 0; b0 < blocks; b0 += per_launch) {
		const unsigned nb = (unsigned)(blocks - b0 < per_launch ? blocks - b0 : per_launch);
		hipLaunchKernelGGL(gv_refine_kernel, dim3(nb), dim3(64), (size_t)lds_frames * 2 * sizeof(double), s, d_utt, b0, nd, n_ap, d_gv_mean,
						   d_gv_var, d_mask, P, lds_frames, plane, sys, d_static);
		WC_HIP(hipGetLastError());
	}
	if ((rc = dev->time_end("gv_refine_kernel", s))) return rc;
	return ft_finish(dev, s);
}

}  // extern "C"
