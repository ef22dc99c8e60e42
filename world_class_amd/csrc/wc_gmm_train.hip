// Expectation-maximisation for the joint-density GMM (include/world_class_gmm_train.h).
//
//   gmm_ll_kernel     (wc_gmm_ll.hpp) ll(t, m) on the joint row: the conversion's kernel on a GmmDev of width D.
//   gmm_post_kernel   lane = frame, a wavefront per 64 frames, four to a block.  The table of ll is walked three times in tiles of 16
//                     mixtures that each wavefront transposes through LDS of its own (read along the rows, 65 doubles from mixture to
//                     mixture): top, then s, then gamma = e / s, which goes back through the tile so that the table of gamma is
//                     written along its rows too.  e(m) is formed twice by the same operations instead of being kept.
//   gmm_seg_kernel    a wavefront per segment brings frame_ll and the frames' states into LDS; lane 0 sums the live ones ascending
//                     and counts the live and the dropped.
//   gmm_stats_kernel  the hot path.  A block of 256 owns one (segment, mixture) and 256 of the 4 x 4 tiles of S2's lower triangle, a tile
//                     to a thread (blockIdx.z where the triangle has more; a block sized to its share of tiles was measured: no gain).  Wavefront 0 compacts the segment's live frames into a list in LDS.
//                     The block then walks that list ascending in sub-tiles of 16 frames: d = z - mean of the 16 frames and their
//                     gamma are parked in LDS (rows padded to whole fours with 0.0), and every thread takes g = gamma * d(i) for its
//                     four rows and adds g * d(j) for its four columns, frame after frame, each its own sum.  The tiles on the
//                     diagonal carry S1 of their four rows, tile 0 carries N.  The sums start at -0.0, the one start from which
//                     `sum = sum + term` gives the term itself, bit for bit, for every first term (0.0 + -0.0 would lose the sign).
//   gmm_fold_kernel   a thread per total: total = total + partial over the launch's segments ascending; two more threads for LL and
//                     the counts.
// No atomics and no matrix instructions; every loop is bounded by n_mix, D and the segment; threads past the data read and write no
// global memory.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/world_class_gmm_train.h"
#include "wc_features_batch.hpp"
#include "wc_features_rows.hpp"
#include "wc_gmm_ll.hpp"
#include "wc_gmm_train_plan.hpp"
#include "wc_internal.hpp"

using namespace wc;

struct wc_gmm_trainer {
	Device *dev = nullptr;
	int n_mix = 0, dx = 0, dy = 0, D = 0;
	GmmTrainModel mdl;
	DevBuf model;   // Wt (+ kRows doubles of 0.0 behind it), mean, c
	DevBuf totals;  // n_mix * width doubles, LL, then two long long: n_live, n_dropped
	int cus = 256, segments = 0;
};

namespace {

constexpr int kPostM = 16, kPostWaves = 4, kStatF = 16, kStatThreads = 256, kBlock = 4;
enum : unsigned char { kMasked = 0, kLive = 1, kDropped = 2 };

__global__ __launch_bounds__(64 * kPostWaves) void gmm_post_kernel(int n_mix, long long t0, unsigned nc, const unsigned char *__restrict__ mask,
																   const double *__restrict__ table, double *__restrict__ post,
																   double *__restrict__ fll, unsigned char *__restrict__ state) {
	__shared__ double tiles[kPostWaves][kPostM * kPitch];
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	const unsigned f0 = (blockIdx.x * kPostWaves + wave) * 64u, f = f0 + lane;
	double *tile = tiles[wave];
	const auto load = [&](int m0, int mc) {
		for (int idx = lane; idx < 64 * mc; idx += 64) {
			const int ff = idx / mc, mm = idx - ff * mc;
			tile[mm * kPitch + ff] = f0 + ff < nc ? table[(size_t)(f0 + ff) * n_mix + m0 + mm] : 0.0;
		}
	};
	bool any = false;
	double top = 0.0;
	for (int m0 = 0; m0 < n_mix; m0 += kPostM) {
		const int mc = n_mix - m0 < kPostM ? n_mix - m0 : kPostM;
		load(m0, mc);
		__syncthreads();
		for (int mm = 0; mm < mc; ++mm) {
			const double v = tile[mm * kPitch + lane];
			if (v == v && (!any || v > top)) { top = v; any = true; }
		}
		__syncthreads();
	}
	const bool in = f < nc;
	const bool counted = in && (!mask || mask[(size_t)t0 + f] != 0);
	const bool live = counted && any && fabs(top) <= DBL_MAX;
	double s = 0.0;
	for (int m0 = 0; m0 < n_mix; m0 += kPostM) {
		const int mc = n_mix - m0 < kPostM ? n_mix - m0 : kPostM;
		load(m0, mc);
		__syncthreads();
		if (live)
			for (int mm = 0; mm < mc; ++mm) {
				const double v = tile[mm * kPitch + lane];
				const double e = v == v ? exp(v - top) : 0.0;
				s = m0 + mm == 0 ? e : s + e;
			}
		__syncthreads();
	}
	if (in) {
		fll[f] = live ? top + log(s) : 0.0;
		state[f] = !counted ? kMasked : (live ? kLive : kDropped);
	}
	if (!post) return;  // (the same for every thread of the launch)
	for (int m0 = 0; m0 < n_mix; m0 += kPostM) {
		const int mc = n_mix - m0 < kPostM ? n_mix - m0 : kPostM;
		load(m0, mc);
		__syncthreads();
		for (int mm = 0; mm < mc; ++mm) {
			const double v = tile[mm * kPitch + lane];
			double gamma = 0.0;
			if (live) gamma = (v == v ? exp(v - top) : 0.0) / s;
			tile[mm * kPitch + lane] = gamma;
		}
		__syncthreads();
		for (int idx = lane; idx < 64 * mc; idx += 64) {
			const int ff = idx / mc, mm = idx - ff * mc;
			if (f0 + ff < nc) post[(size_t)(f0 + ff) * n_mix + m0 + mm] = tile[mm * kPitch + ff];
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(64) void gmm_seg_kernel(unsigned nc, const double *__restrict__ fll, const unsigned char *__restrict__ state,
													 double *__restrict__ seg_ll, long long *__restrict__ seg_cnt) {
	__shared__ double v[kGmmSegment];
	__shared__ unsigned char st[kGmmSegment];
	const unsigned base = blockIdx.x * (unsigned)kGmmSegment;
	const int n = nc - base < (unsigned)kGmmSegment ? (int)(nc - base) : kGmmSegment;
	for (int i = threadIdx.x; i < n; i += 64) {
		v[i] = fll[base + i];
		st[i] = state[base + i];
	}
	__syncthreads();
	if (threadIdx.x != 0) return;
	double acc = -0.0;
	long long n_live = 0, n_dropped = 0;
	for (int i = 0; i < n; ++i) {
		if (st[i] == kLive) { acc = acc + v[i]; ++n_live; }
		else if (st[i] == kDropped) ++n_dropped;
	}
	seg_ll[blockIdx.x] = n_live ? acc : 0.0;
	seg_cnt[2 * blockIdx.x] = n_live;
	seg_cnt[2 * blockIdx.x + 1] = n_dropped;
}

// partials: [segment][mixture][N, S1, packed S2] of this launch; post, state: of the launch's first frame; rows: of the call's first
template <class T>
__global__ __launch_bounds__(kStatThreads) void gmm_stats_kernel(int n_mix, int D, int n_tiles, long long t0, unsigned nc, const T *__restrict__ rows, int ld,
																 int col, const double *__restrict__ mean, const double *__restrict__ post,
																 const unsigned char *__restrict__ state, double *__restrict__ partials) {
	__shared__ __attribute__((aligned(16))) double d[kStatF * kGmmMaxDim];
	__shared__ double gam[kStatF];
	__shared__ unsigned short list[kGmmSegment];
	__shared__ int n_list;
	const int tid = threadIdx.x, m = blockIdx.y, pitch = (D + kBlock - 1) / kBlock * kBlock;
	const unsigned base = blockIdx.x * (unsigned)kGmmSegment;
	const int seg_n = nc - base < (unsigned)kGmmSegment ? (int)(nc - base) : kGmmSegment;
	if (tid < 64) {
		int count = 0;
		for (int it = 0; it < kGmmSegment / 64; ++it) {
			const int f = it * 64 + tid;
			const bool live = f < seg_n && state[base + f] == kLive;
			const unsigned long long votes = __ballot(live);
			if (live) list[count + __popcll(votes & ((1ull << tid) - 1ull))] = (unsigned short)f;
			count += __popcll(votes);
		}
		if (tid == 0) n_list = count;
	}
	__syncthreads();
	const int n = n_list;
	// this thread's tile of the lower triangle: rows i0 .. i0 + 3, columns j0 .. j0 + 3, j0 <= i0
	const int tile = blockIdx.z * kStatThreads + tid;
	const bool active = tile < n_tiles;
	int bi = 0;
	if (active) {
		bi = (int)((sqrtf(8.0f * (float)tile + 1.0f) - 1.0f) * 0.5f);
		while (bi * (bi + 1) / 2 > tile) --bi;
		while ((bi + 1) * (bi + 2) / 2 <= tile) ++bi;
	}
	const int bj = tile - bi * (bi + 1) / 2, i0 = bi * kBlock, j0 = bj * kBlock;
	const bool diag = active && bi == bj, first = tile == 0;
	double acc[kBlock][kBlock], s1[kBlock], occ = -0.0;
#pragma unroll
	for (int r = 0; r < kBlock; ++r) {
		s1[r] = -0.0;
#pragma unroll
		for (int c = 0; c < kBlock; ++c) acc[r][c] = -0.0;
	}
	const double *mu = mean + (size_t)m * D;
	for (int at = 0; at < n; at += kStatF) {
		const int cnt = n - at < kStatF ? n - at : kStatF;
		for (int idx = tid; idx < cnt * pitch; idx += kStatThreads) {
			const int ff = idx / pitch, i = idx - ff * pitch;
			const size_t t = (size_t)t0 + base + list[at + ff];
			d[idx] = i < D ? (double)rows[t * ld + col + i] - mu[i] : 0.0;
		}
		if (tid < cnt) gam[tid] = post[((size_t)base + list[at + tid]) * n_mix + m];
		__syncthreads();
		if (active) {
			for (int ff = 0; ff < cnt; ++ff) {
				const double gamma = gam[ff];
				const double *row = d + ff * pitch;
				double g[kBlock], dj[kBlock];
#pragma unroll
				for (int r = 0; r < kBlock; ++r) {
					g[r] = gamma * row[i0 + r];
					dj[r] = row[j0 + r];
				}
#pragma unroll
				for (int r = 0; r < kBlock; ++r)
#pragma unroll
					for (int c = 0; c < kBlock; ++c) acc[r][c] = acc[r][c] + g[r] * dj[c];
				if (diag) {
#pragma unroll
					for (int r = 0; r < kBlock; ++r) s1[r] = s1[r] + g[r];
				}
				if (first) occ = occ + gamma;
			}
		}
		__syncthreads();
	}
	if (!active) return;
	double *out = partials + ((size_t)blockIdx.x * n_mix + m) * (1 + (size_t)D + (size_t)D * (D + 1) / 2);
	const bool none = n == 0;  // an empty sum is +0.0
	if (first) out[0] = none ? 0.0 : occ;
#pragma unroll
	for (int r = 0; r < kBlock; ++r) {
		const int i = i0 + r;
		if (i >= D) continue;
		if (diag) out[1 + i] = none ? 0.0 : s1[r];
		double *tri = out + 1 + D + (size_t)i * (i + 1) / 2;
#pragma unroll
		for (int c = 0; c < kBlock; ++c)
			if (j0 + c <= i) tri[j0 + c] = none ? 0.0 : acc[r][c];
	}
}

__global__ __launch_bounds__(256) void gmm_fold_kernel(unsigned long long n_el, int segments, const double *__restrict__ partials,
													   const double *__restrict__ seg_ll, const long long *__restrict__ seg_cnt,
													   double *__restrict__ totals, long long *__restrict__ counts) {
	const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (e < n_el) {
		double acc = totals[e];
		for (int s = 0; s < segments; ++s) acc = acc + partials[(size_t)s * n_el + e];
		totals[e] = acc;
	} else if (e == n_el) {
		double acc = totals[n_el];
		for (int s = 0; s < segments; ++s) acc = acc + seg_ll[s];
		totals[n_el] = acc;
	} else if (e == n_el + 1) {
		long long n_live = counts[0], n_dropped = counts[1];
		for (int s = 0; s < segments; ++s) {
			n_live += seg_cnt[2 * s];
			n_dropped += seg_cnt[2 * s + 1];
		}
		counts[0] = n_live;
		counts[1] = n_dropped;
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int refuse(const char *who, const std::string &why) { return fail(WC_ERR_INVALID, std::string("gmm trainer ") + who + ": " + why); }

unsigned long long span_of(long long n, int ld, int cols, unsigned long long esz) {
	return n > 0 ? ((unsigned long long)(n - 1) * (unsigned long long)ld + (unsigned long long)cols) * esz : 0ull;
}

size_t totals_doubles(const wc_gmm_trainer *t) { return (size_t)t->n_mix * gmm_train_width(t->D) + 1; }
size_t totals_bytes(const wc_gmm_trainer *t) { return totals_doubles(t) * sizeof(double) + 2 * sizeof(long long); }

// the model in force on the device, behind everything that may still read the one before
int upload_model(wc_gmm_trainer *t) {
	const size_t N = (size_t)t->D, M = (size_t)t->n_mix;
	std::vector<double> up(M * N * N + kRows + M * N + M, 0.0);
	double *Wt = up.data(), *mean = Wt + M * N * N + kRows, *c = mean + M * N;
	for (size_t m = 0; m < M; ++m)
		for (size_t i = 0; i < N; ++i)
			for (size_t k = 0; k <= i; ++k) Wt[(m * N + k) * N + i] = t->mdl.W[(m * N + i) * N + k];
	std::copy(t->mdl.mean.begin(), t->mdl.mean.end(), mean);
	std::copy(t->mdl.c.begin(), t->mdl.c.end(), c);
	t->dev->quiesce();
	WC_HIP(hipMemcpy(t->model.p, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice));
	return WC_OK;
}

// the totals on the host, behind every accumulate: n_mix rows of N, S1, packed S2, then LL; the two counts
int fetch_totals(wc_gmm_trainer *t, std::vector<double> *tot, long long counts[2]) {
	Device *dev = t->dev;
	hipStream_t s = dev->active();
	if (dev->features_done && dev->features_last != s) WC_HIP(hipStreamWaitEvent(s, dev->features_done, 0));
	const size_t n = totals_doubles(t);
	tot->resize(n + 2);
	WC_HIP(hipMemcpyAsync(tot->data(), t->totals.p, totals_bytes(t), hipMemcpyDeviceToHost, s));
	WC_HIP(hipStreamSynchronize(s));
	std::memcpy(counts, tot->data() + n, 2 * sizeof(long long));
	return WC_OK;
}

int clear_totals(wc_gmm_trainer *t) {
	Device *dev = t->dev;
	hipStream_t s = dev->active();
	if (!dev->features_done) WC_HIP(hipEventCreateWithFlags(&dev->features_done, hipEventDisableTiming));
	else if (dev->features_last != s) WC_HIP(hipStreamWaitEvent(s, dev->features_done, 0));
	WC_HIP(hipMemsetAsync(t->totals.p, 0, totals_bytes(t), s));
	return ft_finish(dev, s);  // an accumulate on another stream waits for the clearing
}

// the checks posterior and accumulate share
int check_rows(const char *who, const wc_gmm_trainer *t, long long n_frames, int format, const void *d_rows, int ld, int col) {
	if (!t) return refuse(who, "null handle");
	if (!t->mdl.set) return refuse(who, "no model is set");
	if (n_frames < 0 || n_frames > 0xffffffffll) return refuse(who, "n_frames outside 0 .. 2^32 - 1");
	if (format != WC_FEAT_F64 && format != WC_FEAT_F32) return refuse(who, "a format is 0 (double) or 1 (float)");
	if (col < 0) return refuse(who, "a negative column");
	if ((long long)ld < (long long)col + t->D) return refuse(who, "ld < col + D");
	if (n_frames > 0 && !d_rows) return refuse(who, "null d_rows");
	return WC_OK;
}

// the E-step of every launch and, where stats, the statistics behind it
int run(wc_gmm_trainer *t, bool stats, long long n_frames, int format, const void *d_rows, int ld, int col, const unsigned char *d_mask, double *d_post,
		double *d_frame_ll) {
	Device *dev = t->dev;
	DeviceLock lock(dev);
	OnDeviceOf here(dev);
	hipStream_t s = dev->active();
	const int n_mix = t->n_mix, D = t->D;
	const size_t M = (size_t)n_mix, N = (size_t)D, P = gmm_train_width(D);
	long long g = gmm_train_segments(n_mix, D, t->segments);
	const long long all = (n_frames + kGmmSegment - 1) / kGmmSegment;
	g = g > all ? all : g;
	const size_t cap = (size_t)g * kGmmSegment;  // frames of a launch at the most
	// the scratch of a launch
	const size_t off_post = cap * M, off_fll = off_post + cap * M, off_segll = off_fll + cap, off_cnt = off_segll + (size_t)g,
				 off_part = off_cnt + 2 * (size_t)g, off_state = off_part + (stats ? (size_t)g * M * P : 0);
	int rc;
	const int one = (int)(cap > 0x7fffffffull ? 0x7fffffff : cap);
	const FtUtt *d_utt = nullptr;  // (not read: the call takes the scratch and its hand-over from stream to stream)
	if ((rc = ft_prepare(dev, s, 1, &one, off_state * sizeof(double) + cap, &d_utt))) return rc;
	double *scratch = dev->features_scratch.as<double>();
	double *table = scratch, *seg_ll = scratch + off_segll, *partials = scratch + off_part;
	long long *seg_cnt = reinterpret_cast<long long *>(scratch + off_cnt);
	unsigned char *state = reinterpret_cast<unsigned char *>(scratch + off_state);
	const double *base = t->model.as<double>();
	GmmDev dv;
	dv.Wt = base;
	dv.mux = base + M * N * N + kRows;
	dv.c = dv.mux + M * N;
	dv.Bt = dv.muy = dv.cvar = nullptr;
	dv.n_mix = n_mix; dv.dx = D; dv.dy = 0;
	const int nb = (D + kBlock - 1) / kBlock, n_tiles = nb * (nb + 1) / 2;
	double *totals = t->totals.as<double>();
	long long *counts = reinterpret_cast<long long *>(totals + totals_doubles(t));
	for (long long t0 = 0; t0 < n_frames; t0 += (long long)cap) {
		const long long nc = n_frames - t0 < (long long)cap ? n_frames - t0 : (long long)cap;
		const int segs = (int)((nc + kGmmSegment - 1) / kGmmSegment);
		if ((rc = dev->time_begin("gmm_ll_kernel", s))) return rc;
		if (format == WC_FEAT_F32) gmm_ll_launch(dv, t->cus, s, t0, nc, n_frames, static_cast<const float *>(d_rows), ld, col, table);
		else gmm_ll_launch(dv, t->cus, s, t0, nc, n_frames, static_cast<const double *>(d_rows), ld, col, table);
		WC_HIP(hipGetLastError());
		if ((rc = dev->time_end("gmm_ll_kernel", s))) return rc;
		double *post = stats ? scratch + off_post : (d_post ? d_post + (size_t)t0 * M : nullptr);
		double *fll = stats || !d_frame_ll ? scratch + off_fll : d_frame_ll + t0;
		if ((rc = dev->time_begin("gmm_post_kernel", s))) return rc;
		hipLaunchKernelGGL(gmm_post_kernel, dim3((unsigned)((nc + 64 * kPostWaves - 1) / (64 * kPostWaves))), dim3(64 * kPostWaves), 0, s, n_mix, t0,
						   (unsigned)nc, d_mask, table, post, fll, state);
		WC_HIP(hipGetLastError());
		if ((rc = dev->time_end("gmm_post_kernel", s))) return rc;
		if (!stats) continue;
		hipLaunchKernelGGL(gmm_seg_kernel, dim3(segs), dim3(64), 0, s, (unsigned)nc, fll, state, seg_ll, seg_cnt);
		WC_HIP(hipGetLastError());
		const dim3 grid((unsigned)segs, (unsigned)n_mix, (unsigned)((n_tiles + kStatThreads - 1) / kStatThreads));
		if ((rc = dev->time_begin("gmm_stats_kernel", s))) return rc;
		if (format == WC_FEAT_F32)
			hipLaunchKernelGGL(gmm_stats_kernel<float>, grid, dim3(kStatThreads), 0, s, n_mix, D, n_tiles, t0, (unsigned)nc, static_cast<const float *>(d_rows),
							   ld, col, dv.mux, post, state, partials);
		else
			hipLaunchKernelGGL(gmm_stats_kernel<double>, grid, dim3(kStatThreads), 0, s, n_mix, D, n_tiles, t0, (unsigned)nc,
							   static_cast<const double *>(d_rows), ld, col, dv.mux, post, state, partials);
		WC_HIP(hipGetLastError());
		if ((rc = dev->time_end("gmm_stats_kernel", s))) return rc;
		const unsigned long long n_el = (unsigned long long)(M * P);
		hipLaunchKernelGGL(gmm_fold_kernel, dim3((unsigned)((n_el + 2 + 255) / 256)), dim3(256), 0, s, n_el, segs, partials, seg_ll, seg_cnt, totals, counts);
		WC_HIP(hipGetLastError());
	}
	return ft_finish(dev, s);
}

}  // namespace

extern "C" {

wc_gmm_trainer *wc_gmm_trainer_create(int n_mix, int dx, int dy) {
	const auto no = [](const std::string &why) { set_error("gmm trainer create: " + why); return (wc_gmm_trainer *)nullptr; };
	if (n_mix < 1 || n_mix > kGmmMaxMix) return no("n_mix outside 1 .. 1024");
	if (dx < 1 || dy < 1 || (long long)dx + dy > kGmmMaxDim) return no("dx and dy are at least 1 and D = dx + dy lies in 2 .. 192");
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	wc_gmm_trainer *t = new wc_gmm_trainer();
	t->dev = dev;
	t->n_mix = n_mix; t->dx = dx; t->dy = dy; t->D = dx + dy;
	const size_t N = (size_t)t->D, M = (size_t)n_mix;
	bool ok = t->model.reserve((M * N * N + kRows + M * N + M) * sizeof(double)) == 0 && t->totals.reserve(totals_bytes(t)) == 0 &&
			  hipMemset(t->totals.p, 0, totals_bytes(t)) == hipSuccess;
	int cus = 0;
	if (ok && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev->id) == hipSuccess && cus > 0) t->cus = cus;
	const size_t lds = gmm_lds_bytes_of(t->D);  // a tile above the 64 KB every kernel may take has to be asked for
	if (ok && lds > 65536)
		ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&gmm_ll_kernel<double>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
			 hipFuncSetAttribute(reinterpret_cast<const void *>(&gmm_ll_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
	if (!ok) {
		(void)hipGetLastError();
		t->model.release();
		t->totals.release();
		delete t;
		return no("the handle could not be placed on the device");
	}
	return t;
}

void wc_gmm_trainer_destroy(wc_gmm_trainer *t) {
	if (!t) return;
	t->dev->quiesce();
	t->model.release();
	t->totals.release();
	delete t;
}

int wc_gmm_trainer_set_model(wc_gmm_trainer *t, const double *h_weight, const double *h_mean, const double *h_cov) {
	if (!t) return refuse("set model", "null handle");
	GmmTrainModel next;
	std::string why;
	if (!gmm_train_set_model(t->n_mix, t->D, h_weight, h_mean, h_cov, &next, &why)) return refuse("set model", why);
	DeviceLock lock(t->dev);
	OnDeviceOf here(t->dev);
	t->mdl = std::move(next);
	return upload_model(t);
}

int wc_gmm_trainer_model_host(const wc_gmm_trainer *t, double *h_weight, double *h_mean, double *h_cov) {
	if (!t) return refuse("model", "null handle");
	if (!t->mdl.set) return refuse("model", "no model is set");
	if (h_weight) std::copy(t->mdl.weight.begin(), t->mdl.weight.end(), h_weight);
	if (h_mean) std::copy(t->mdl.mean.begin(), t->mdl.mean.end(), h_mean);
	if (h_cov) std::copy(t->mdl.cov.begin(), t->mdl.cov.end(), h_cov);
	return WC_OK;
}

int wc_gmm_trainer_posterior_device(wc_gmm_trainer *t, long long n_frames, int format, const void *d_rows, int ld, int col, const unsigned char *d_mask,
									double *d_post, double *d_frame_ll) {
	const char *who = "posterior";
	if (int rc = check_rows(who, t, n_frames, format, d_rows, ld, col)) return rc;
	if (n_frames == 0) return WC_OK;
	if (!d_post && !d_frame_ll) return refuse(who, "both outputs are NULL");
	const unsigned long long esz = format == WC_FEAT_F32 ? 4 : 8;
	const char *in0 = static_cast<const char *>(d_rows) + (size_t)col * esz;
	const unsigned long long in_bytes = span_of(n_frames, ld, t->D, esz), post_bytes = 8ull * n_frames * t->n_mix, fll_bytes = 8ull * n_frames;
	if (overlap(d_post, post_bytes, d_frame_ll, fll_bytes)) return refuse(who, "the two outputs overlap");
	if (overlap(d_post, post_bytes, in0, in_bytes) || overlap(d_frame_ll, fll_bytes, in0, in_bytes)) return refuse(who, "an output overlaps the rows");
	if (overlap(d_post, post_bytes, d_mask, n_frames) || overlap(d_frame_ll, fll_bytes, d_mask, n_frames)) return refuse(who, "an output overlaps the mask");
	return run(t, false, n_frames, format, d_rows, ld, col, d_mask, d_post, d_frame_ll);
}

int wc_gmm_trainer_accumulate_device(wc_gmm_trainer *t, long long n_frames, int format, const void *d_rows, int ld, int col, const unsigned char *d_mask) {
	if (int rc = check_rows("accumulate", t, n_frames, format, d_rows, ld, col)) return rc;
	if (n_frames == 0) return WC_OK;
	return run(t, true, n_frames, format, d_rows, ld, col, d_mask, nullptr, nullptr);
}

int wc_gmm_trainer_stats_host(wc_gmm_trainer *t, double *h_N, double *h_S1, double *h_S2, wc_gmm_train_info *info) {
	if (!t) return refuse("stats", "null handle");
	DeviceLock lock(t->dev);
	OnDeviceOf here(t->dev);
	std::vector<double> tot;
	long long counts[2];
	if (int rc = fetch_totals(t, &tot, counts)) return rc;
	const size_t N = (size_t)t->D, P = gmm_train_width(t->D), T = N * (N + 1) / 2;
	for (size_t m = 0; m < (size_t)t->n_mix; ++m) {
		const double *st = tot.data() + m * P;
		if (h_N) h_N[m] = st[0];
		if (h_S1) std::copy(st + 1, st + 1 + N, h_S1 + m * N);
		if (h_S2) std::copy(st + 1 + N, st + P, h_S2 + m * T);
	}
	if (info) {
		info->loglik = tot[(size_t)t->n_mix * P];
		info->n_live = counts[0];
		info->n_dropped = counts[1];
		info->n_starved = info->n_kept = 0;
	}
	return WC_OK;
}

int wc_gmm_trainer_update(wc_gmm_trainer *t, double min_occupancy, const double *h_var_floor, wc_gmm_train_info *info) {
	const char *who = "update";
	if (!t) return refuse(who, "null handle");
	if (!t->mdl.set) return refuse(who, "no model is set");
	if (!gmm_finite(min_occupancy) || min_occupancy < 1.0) return refuse(who, "min_occupancy is not finite or < 1");
	if (h_var_floor)
		for (int i = 0; i < t->D; ++i)
			if (!gmm_finite(h_var_floor[i]) || h_var_floor[i] < 0.0) return refuse(who, "a floor that is negative or not finite");
	DeviceLock lock(t->dev);
	OnDeviceOf here(t->dev);
	std::vector<double> tot;
	long long counts[2];
	if (int rc = fetch_totals(t, &tot, counts)) return rc;
	if (counts[0] == 0) return refuse(who, "n_live == 0: there is nothing to estimate from");
	int n_starved = 0, n_kept = 0;
	gmm_train_update(&t->mdl, tot.data(), counts[0], min_occupancy, h_var_floor, &n_starved, &n_kept);
	if (int rc = upload_model(t)) return rc;
	if (int rc = clear_totals(t)) return rc;
	if (info) {
		info->loglik = tot[(size_t)t->n_mix * gmm_train_width(t->D)];
		info->n_live = counts[0];
		info->n_dropped = counts[1];
		info->n_starved = n_starved;
		info->n_kept = n_kept;
	}
	return WC_OK;
}

int wc_gmm_trainer_reset_stats(wc_gmm_trainer *t) {
	if (!t) return refuse("reset stats", "null handle");
	DeviceLock lock(t->dev);
	OnDeviceOf here(t->dev);
	return clear_totals(t);
}

int wc_gmm_trainer_set_segments_per_launch(wc_gmm_trainer *t, int g) {
	if (!t) return refuse("set segments per launch", "null handle");
	if (g < 0) return refuse("set segments per launch", "g < 0");
	t->segments = g;
	return WC_OK;
}

}  // extern "C"
