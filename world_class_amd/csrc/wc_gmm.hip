// Joint-density GMM conversion (include/world_class_gmm.h).
//
//   gmm_ll_kernel    (wc_gmm_ll.hpp, shared with the training) ll(t, m) of THE rule of convert.  A block of eight wavefronts takes a tile of 64 frames: the tile's source vectors
//                    are read along the rows (neighbouring threads on neighbouring columns), widened, and parked in LDS transposed,
//                    65 doubles from column to column, so that both the writes and the reads (lane = frame) miss each other's banks.
//                    Each wavefront then walks mixtures of its own: m = first + wave, + 8, ... inside the block's share of them
//                    (blockIdx.y; the host cuts the mixtures into shares where the tiles alone do not fill the chip).  W_m stands
//                    transposed on the device (column k of W is a row), so that sixteen rows i0 .. i0 + 15 at one k are 128
//                    contiguous bytes behind a wave-uniform address: they, mux_m and c_m arrive through scalar loads, once per
//                    wavefront.  The sixteen partial sums z(i0 .. i0 + 15) stand in registers and take d(k) in ascending k, each its
//                    own sum in the rule's order (the last rows of a mixture go in a block of 16, 8 or 4, whichever holds them);
//                    d(k) = x(k) - mux_m(k) is formed once per block of rows from the LDS tile (a tile of d next to the tile of x
//                    would halve the wavefronts a compute unit holds).  No lane's sum depends on another lane or on the launch shape.
//   gmm_pick_kernel  one wavefront per frame: the least best m over the table in a fixed butterfly (a total order, so every order
//                    of comparison gives the same m), d and z of that mixture again by the same operations (lane = row, the
//                    transposed W read along its rows), then mean(j) and var(j) with lane = j, B transposed as well.
// The table of ll is d_loglik where the caller gave one, else the model features' per-device scratch.  No atomics; every loop is
// bounded by n_mix, dx and dy; lanes past n_frames read and write no global memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/world_class_gmm.h"
#include "wc_features_batch.hpp"
#include "wc_features_rows.hpp"
#include "wc_gmm_ll.hpp"
#include "wc_gmm_plan.hpp"
#include "wc_internal.hpp"

using namespace wc;

struct wc_gmm {
	Device *dev = nullptr;
	GmmPlan plan;
	DevBuf model;  // Wt (+ kRows doubles of 0.0 behind it), Bt, mux, muy, c, cvar
	int cus = 256;
};

namespace {

constexpr size_t kTableBytes = (size_t)256 << 20;  // the most scratch one launch's table of ll takes
constexpr long long kChunkMax = 1ll << 24;         // frames of one launch at the most

template <class T, class O>
__global__ __launch_bounds__(64) void gmm_pick_kernel(GmmDev g, long long t0, const T *__restrict__ rows, int ld_in, int col_in,
													  const double *__restrict__ table, O *__restrict__ mean, O *__restrict__ var, int ld_out,
													  int col_out, int *__restrict__ best_out) {
	__shared__ double d[kGmmMaxDim], z[kGmmMaxDim];
	const int lane = threadIdx.x, dx = g.dx, dy = g.dy;
	const size_t t = (size_t)t0 + blockIdx.x;
	const double *ll = table + (size_t)blockIdx.x * g.n_mix;
	double bv = 0.0;
	int bi = -1;
	for (int m = lane; m < g.n_mix; m += 64) {
		const double v = ll[m];
		if (v == v && (bi < 0 || v > bv)) { bv = v; bi = m; }
	}
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const double ov = __shfl_xor(bv, off, 64);
		const int oi = __shfl_xor(bi, off, 64);
		if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
	}
	bi = __builtin_amdgcn_readfirstlane(bi);
	if (best_out && lane == 0) best_out[t] = bi;
	if (bi < 0) {
		for (int j = lane; j < dy; j += 64) {
			if (mean) mean[t * ld_out + col_out + j] = (O)0.0;
			if (var) var[t * ld_out + col_out + j] = (O)INFINITY;
		}
		return;
	}
	if (var)
		for (int j = lane; j < dy; j += 64) var[t * ld_out + col_out + j] = (O)g.cvar[(size_t)bi * dy + j];
	if (!mean) return;
	for (int k = lane; k < dx; k += 64) d[k] = (double)rows[t * ld_in + col_in + k] - g.mux[(size_t)bi * dx + k];
	__syncthreads();
	const double *Wb = g.Wt + (size_t)bi * dx * dx;
	for (int i0 = 0; i0 < dx; i0 += 64) {
		const int i = i0 + lane, last = i0 + 63 < dx - 1 ? i0 + 63 : dx - 1;  // the last column any row of this group reaches
		if (i < dx) {
			double s = Wb[i] * d[0];
#pragma unroll 4
			for (int k = 1; k <= last; ++k)
				if (k <= i) s = s + Wb[(size_t)k * dx + i] * d[k];
			z[i] = s;
		}
	}
	__syncthreads();
	const double *Bb = g.Bt + (size_t)bi * dx * dy;
	for (int j = lane; j < dy; j += 64) {
		double s = Bb[j] * z[0];
#pragma unroll 4
		for (int k = 1; k < dx; ++k) s = s + Bb[(size_t)k * dy + j] * z[k];
		mean[t * ld_out + col_out + j] = (O)(g.muy[(size_t)bi * dy + j] + s);
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
size_t lds_bytes_of(int dx) { return gmm_lds_bytes_of(dx); }

int refuse(const char *why) { return fail(WC_ERR_INVALID, std::string("gmm convert: ") + why); }

// the bytes from the first to the last element that a call touches in an array of rows
unsigned long long span_of(long long n, int ld, int cols, unsigned long long esz) {
	return n > 0 ? ((unsigned long long)(n - 1) * (unsigned long long)ld + (unsigned long long)cols) * esz : 0ull;
}

template <class T, class O>
void launch_pick(const GmmDev &dv, hipStream_t s, long long t0, unsigned n, const void *rows, int ld_in, int col_in, const double *table, void *mean,
				 void *var, int ld_out, int col_out, int *best) {
	hipLaunchKernelGGL((gmm_pick_kernel<T, O>), dim3(n), dim3(64), 0, s, dv, t0, static_cast<const T *>(rows), ld_in, col_in, table,
					   static_cast<O *>(mean), static_cast<O *>(var), ld_out, col_out, best);
}

}  // namespace

extern "C" {

wc_gmm *wc_gmm_create(int n_mix, int dx, int dy, const double *h_weight, const double *h_mean, const double *h_cov) {
	const auto no = [](const std::string &why) { set_error("gmm create: " + why); return (wc_gmm *)nullptr; };
	wc_gmm *g = new wc_gmm();
	std::string why;
	if (!gmm_prepare(n_mix, dx, dy, h_weight, h_mean, h_cov, &g->plan, &why)) {
		delete g;
		return no(why);
	}
	Device *dev = current_device();
	if (!dev) {
		delete g;
		return nullptr;
	}
	DeviceLock lock(dev);
	g->dev = dev;
	const GmmPlan &p = g->plan;
	const size_t X = (size_t)dx, Y = (size_t)dy, M = (size_t)n_mix;
	const size_t nW = M * X * X + kRows, nB = M * X * Y;
	std::vector<double> up(nW + nB + M * X + M * Y + M + M * Y, 0.0);
	double *Wt = up.data(), *Bt = Wt + nW, *mux = Bt + nB, *muy = mux + M * X, *c = muy + M * Y, *cvar = c + M;
	for (size_t m = 0; m < M; ++m) {
		for (size_t i = 0; i < X; ++i)
			for (size_t k = 0; k <= i; ++k) Wt[(m * X + k) * X + i] = p.W[(m * X + i) * X + k];
		for (size_t j = 0; j < Y; ++j)
			for (size_t k = 0; k < X; ++k) Bt[(m * X + k) * Y + j] = p.B[(m * Y + j) * X + k];
	}
	std::copy(p.mux.begin(), p.mux.end(), mux);
	std::copy(p.muy.begin(), p.muy.end(), muy);
	std::copy(p.c.begin(), p.c.end(), c);
	std::copy(p.cvar.begin(), p.cvar.end(), cvar);
	bool ok = g->model.reserve(up.size() * sizeof(double)) == 0 &&
			  hipMemcpy(g->model.p, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
	int cus = 0;
	if (ok && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev->id) == hipSuccess && cus > 0) g->cus = cus;
	// a tile above the 64 KB every kernel may take has to be asked for (gfx950 has 160 KB a compute unit; the widest tile takes 99 840)
	const size_t lds = lds_bytes_of(dx);
	if (ok && lds > 65536)
		ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&gmm_ll_kernel<double>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
			 hipFuncSetAttribute(reinterpret_cast<const void *>(&gmm_ll_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
	if (!ok) {
		(void)hipGetLastError();
		g->model.release();
		delete g;
		set_error("gmm create: the model could not be placed on the device");
		return nullptr;
	}
	return g;
}

void wc_gmm_destroy(wc_gmm *g) {
	if (!g) return;
	g->dev->quiesce();
	g->model.release();
	delete g;
}

int wc_gmm_prepared_host(const wc_gmm *g, double *h_c, double *h_W, double *h_B, double *h_cvar) {
	if (!g) return fail(WC_ERR_INVALID, "gmm prepared: null handle");
	const GmmPlan &p = g->plan;
	if (h_c) std::copy(p.c.begin(), p.c.end(), h_c);
	if (h_W) std::copy(p.W.begin(), p.W.end(), h_W);
	if (h_B) std::copy(p.B.begin(), p.B.end(), h_B);
	if (h_cvar) std::copy(p.cvar.begin(), p.cvar.end(), h_cvar);
	return WC_OK;
}

int wc_gmm_convert_device(const wc_gmm *g, long long n_frames, int in_format, const void *d_rows_in, int ld_in, int col_in, int out_format,
						  void *d_mean, void *d_var, int ld_out, int col_out, int *d_best, double *d_loglik) {
	if (!g) return refuse("null handle");
	if (n_frames < 0 || n_frames > 0xffffffffll) return refuse("n_frames outside 0 .. 2^32 - 1");
	if ((in_format != WC_FEAT_F64 && in_format != WC_FEAT_F32) || (out_format != WC_FEAT_F64 && out_format != WC_FEAT_F32))
		return refuse("a format is 0 (double) or 1 (float)");
	if (col_in < 0 || col_out < 0) return refuse("a negative column");
	const int n_mix = g->plan.n_mix, dx = g->plan.dx, dy = g->plan.dy;
	if ((long long)ld_in < (long long)col_in + dx) return refuse("ld_in < col_in + dx");
	if ((long long)ld_out < (long long)col_out + dy) return refuse("ld_out < col_out + dy");
	if (n_frames == 0) return WC_OK;
	if (!d_rows_in) return refuse("null d_rows_in");
	if (!d_mean && !d_var && !d_best && !d_loglik) return refuse("all four outputs are NULL");
	const unsigned long long ein = in_format == WC_FEAT_F32 ? 4 : 8, eout = out_format == WC_FEAT_F32 ? 4 : 8;
	const char *in0 = static_cast<const char *>(d_rows_in) + (size_t)col_in * ein;
	const unsigned long long in_bytes = span_of(n_frames, ld_in, dx, ein), out_bytes = span_of(n_frames, ld_out, dy, eout);
	const void *outs[4] = {d_mean ? static_cast<char *>(d_mean) + (size_t)col_out * eout : nullptr,
						   d_var ? static_cast<char *>(d_var) + (size_t)col_out * eout : nullptr, d_best, d_loglik};
	const unsigned long long bytes[4] = {out_bytes, out_bytes, 4ull * n_frames, 8ull * n_frames * n_mix};
	for (int a = 0; a < 4; ++a) {
		if (overlap(outs[a], bytes[a], in0, in_bytes)) return refuse("an output overlaps the input");
		for (int b = a + 1; b < 4; ++b)
			if (overlap(outs[a], bytes[a], outs[b], bytes[b])) return refuse("two outputs overlap");
	}
	Device *dev = g->dev;
	DeviceLock lock(dev);
	OnDeviceOf here(dev);
	hipStream_t s = dev->active();
	long long chunk = (long long)(kTableBytes / (sizeof(double) * (size_t)n_mix)) / kTile * kTile;
	chunk = chunk > kChunkMax ? kChunkMax : chunk;
	if (chunk > n_frames) chunk = n_frames;
	const bool pick = d_mean || d_var || d_best;
	int rc;
	const int one = (int)chunk;
	const FtUtt *d_utt = nullptr;  // (not read: the frames of this call are no utterances; the call takes the scratch and its hand-over)
	if ((rc = ft_prepare(dev, s, 1, &one, d_loglik ? 0 : (size_t)chunk * n_mix * sizeof(double), &d_utt))) return rc;
	const double *base = g->model.as<double>();
	const size_t X = (size_t)dx, Y = (size_t)dy, M = (size_t)n_mix;
	GmmDev dv;
	dv.Wt = base;
	dv.Bt = dv.Wt + M * X * X + kRows;
	dv.mux = dv.Bt + M * X * Y;
	dv.muy = dv.mux + M * X;
	dv.c = dv.muy + M * Y;
	dv.cvar = dv.c + M;
	dv.n_mix = n_mix; dv.dx = dx; dv.dy = dy;
	for (long long t0 = 0; t0 < n_frames; t0 += chunk) {
		const long long nc = n_frames - t0 < chunk ? n_frames - t0 : chunk;
		double *table = d_loglik ? d_loglik + (size_t)t0 * n_mix : dev->features_scratch.as<double>();
		if ((rc = dev->time_begin("gmm_ll_kernel", s))) return rc;
		if (in_format == WC_FEAT_F32) gmm_ll_launch(dv, g->cus, s, t0, nc, n_frames, static_cast<const float *>(d_rows_in), ld_in, col_in, table);
		else gmm_ll_launch(dv, g->cus, s, t0, nc, n_frames, static_cast<const double *>(d_rows_in), ld_in, col_in, table);
		WC_HIP(hipGetLastError());
		if ((rc = dev->time_end("gmm_ll_kernel", s))) return rc;
		if (!pick) continue;
		if ((rc = dev->time_begin("gmm_pick_kernel", s))) return rc;
		const unsigned n = (unsigned)nc;
		if (in_format == WC_FEAT_F32 && out_format == WC_FEAT_F32)
			launch_pick<float, float>(dv, s, t0, n, d_rows_in, ld_in, col_in, table, d_mean, d_var, ld_out, col_out, d_best);
		else if (in_format == WC_FEAT_F32)
			launch_pick<float, double>(dv, s, t0, n, d_rows_in, ld_in, col_in, table, d_mean, d_var, ld_out, col_out, d_best);
		else if (out_format == WC_FEAT_F32)
			launch_pick<double, float>(dv, s, t0, n, d_rows_in, ld_in, col_in, table, d_mean, d_var, ld_out, col_out, d_best);
		else
			launch_pick<double, double>(dv, s, t0, n, d_rows_in, ld_in, col_in, table, d_mean, d_var, ld_out, col_out, d_best);
		WC_HIP(hipGetLastError());
		if ((rc = dev->time_end("gmm_pick_kernel", s))) return rc;
	}
	return ft_finish(dev, s);
}

}  // extern "C"
