// Feature streams (include/world_class_feature_stream.h): packed model rows from a live voice, a lag behind.
//
//   feat_stream_scan_kernel  one wavefront per stream with rows in the push (or wanted by the flush).  It takes the pushed rows into
//                            the stream's ring, the log of a voiced F0 taken once and parked in the F0 column (a NaN marks an unvoiced
//                            row), then does the two bounded shuffle scans of feat_lf0_kernel over the ring window of this call, in
//                            chunks of 64 rows: backwards the suffix min-scan of the voiced indices, forwards the prefix max-scan,
//                            whose initial carry is the stream's carried record.  A lane holds one row i of the window and writes the
//                            continuous log-F0 of i as the rows of frames i + 1, i and i - 1 need it, each with the right neighbour
//                            capped at that frame's own j = min(t + L, newest row); the lane on the last row below the next call's
//                            window advances the carried record.
//   feat_stream_pack_kernel  feat_pack_kernel's pattern: a thread per (emitted frame, static column), neighbouring threads on
//                            neighbouring columns; it reads the ring and the triples.
// No lane searches for a voiced frame: every loop is bounded by a count the host put into the descriptors.  Every expression follows
// the rule of world_class_features.h operation for operation (the tree is built with -ffp-contract=off); tests/feature_stream_rule.py
// is the same recursion in numpy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/world_class_feature_stream.h"
#include "wc_features_rows.hpp"
#include "wc_internal.hpp"
#include "wc_lag_stream.hpp"

using namespace wc;

namespace {

struct FsDesc {          // a stream with rows in this push, or with frames in this flush
	long long lo;        // the first row of the scanned window: the row before the first emitted frame, or row 0
	long long e0;        // the first frame this call emits
	long long last;      // the newest row of the stream behind this call
	long long in_off;    // its first pushed row in d_f0, d_coded_sp and d_coded_ap
	long long out_off;   // its first emitted row in d_rows and in the triples
	double fill;         // lf0_fill
	int stream, k;       // k rows are taken
	int n_out, w;        // frames emitted; rows of the window lo .. last (0 where nothing is emitted: nothing is scanned)
	int lag, slot_lo;    // the ring slot of row lo
	int slot0, adv;      // the ring slot of the first pushed row; rows by which the next call's window starts above lo
};
struct FsCarry {         // the last voiced row below the window the next call scans
	long long idx;       // -1: none
	double lg;
};

constexpr int kPackFrames = 8;  // frames of one block of feat_stream_pack_kernel
constexpr int kNone = 0x7fffffff;

__device__ __forceinline__ double fs_unvoiced() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(64) void feat_stream_scan_kernel(const FsDesc *__restrict__ desc, int nd, int n_ap, int cap,
															  const double *__restrict__ f0, const double *__restrict__ sp,
															  const double *__restrict__ ap, double *__restrict__ ring,
															  FsCarry *__restrict__ carried, int *__restrict__ right,
															  double *__restrict__ triples) {
	const FsDesc d = desc[blockIdx.x];
	const int lane = threadIdx.x, S = nd + 1 + n_ap;
	double *R = ring + (size_t)d.stream * cap * S;
	// take: the pushed rows into the ring, neighbouring lanes on neighbouring columns
	const int items = d.k * S;
	for (int idx = lane; idx < items; idx += 64) {
		const int r = idx / S, c = idx - r * S;
		const size_t g = (size_t)d.in_off + r;
		double v;
		if (c < nd) {
			v = sp[g * nd + c];
		} else if (c == nd) {
			const double f = f0[g];
			v = ft_voiced(f) ? log(f) : fs_unvoiced();
		} else {
			v = ap[g * n_ap + (c - nd - 1)];
		}
		int slot = d.slot0 + r;
		if (slot >= cap) slot -= cap;
		R[(size_t)slot * S + c] = v;
	}
	const int w = d.w;
	if (w <= 0) return;
	__syncthreads();  // (one wavefront: the parked logs are read below by other lanes than wrote them)
	auto parked = [&](int rel) {  // the F0 column of window row rel < cap
		int slot = d.slot_lo + rel;
		if (slot >= cap) slot -= cap;
		return R[(size_t)slot * S + nd];
	};
	int *Rt = right + (size_t)d.stream * cap;
	const int chunks = (w + 63) / 64;
	int carry = kNone;  // kNone: no voiced row at or behind, up to the newest
	for (int c = chunks - 1; c >= 0; --c) {
		const int i = c * 64 + lane;
		const double l = i < w ? parked(i) : fs_unvoiced();
		int m = l == l ? i : kNone;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const int t = __shfl_down(m, o, 64);
			if (lane + o < 64) m = min(m, t);
		}
		m = min(m, carry);
		if (i < w) Rt[i] = m;
		carry = __shfl(m, 0, 64);
	}
	// -1: the carried record, a voiced row below the window; -2: no voiced row at or before
	FsCarry rec = {-1, 0.0};
	if (d.lo > 0) rec = carried[d.stream];
	carry = rec.idx >= 0 ? -1 : -2;
	const long long first = d.e0 - d.lo;  // the first emitted frame as a row of the window: 0 or 1
	double *T3 = triples + (size_t)d.out_off * 3;
	for (int c = 0; c < chunks; ++c) {
		const int i = c * 64 + lane;
		const double l = i < w ? parked(i) : fs_unvoiced();
		int m = l == l ? i : -2;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const int t = __shfl_up(m, o, 64);
			if (lane >= o) m = max(m, t);
		}
		m = max(m, carry);
		carry = __shfl(m, 63, 64);
		if (i >= w) continue;
		const int L = m, Rr = Rt[i];  // (written by this lane in the first walk)
		const double lo_log = L >= 0 ? parked(L) : rec.lg, hi_log = Rr != kNone ? parked(Rr) : 0.0;
		double mid = 0.0;
		if (L != i && L > -2 && Rr != kNone) {
			const long long left = L >= 0 ? d.lo + L : rec.idx, at = d.lo + i;
			const double a = (double)(at - left) / (double)(d.lo + Rr - left);
			mid = (1.0 - a) * lo_log + a * hi_log;
		}
		// row i as its own frame's row needs it and as the rows of its two neighbours need it: frame t = e0 + f sees the rows up to
		// j = min(t + lag, last), a voiced row beyond j is not there yet
		for (int n = -1; n <= 1; ++n) {  // the frame is row i - n: this row is its neighbour on side n
			const long long f = (long long)i - n - first;
			if (f < 0 || f >= d.n_out) continue;
			const long long t = d.e0 + f, j = t + d.lag < d.last ? t + d.lag : d.last;
			if (d.lo + i > j) continue;  // beyond the frame's prefix: the pack kernel counts it as 0.0
			const bool has_r = Rr != kNone && d.lo + Rr <= j;
			double v;
			if (L == -2 && !has_r) v = d.fill;
			else if (L == i) v = l;
			else if (L == -2) v = hi_log;
			else if (!has_r) v = lo_log;
			else v = mid;
			T3[(size_t)f * 3 + (n + 1)] = v;
		}
		if (i + 1 == d.adv) {  // the last row below the next call's window
			FsCarry next = rec;
			if (L >= 0) { next.idx = d.lo + L; next.lg = lo_log; }
			else if (L == -2) next.idx = -1;
			carried[d.stream] = next;
		}
	}
}

template <class T>
__global__ __launch_bounds__(256) void feat_stream_pack_kernel(const FsDesc *__restrict__ desc, int n_desc, long long total, int nd, int n_ap,
															   int orders, int cap, const double *__restrict__ ring,
															   const double *__restrict__ triples, T *__restrict__ rows) {
	__shared__ int s_d[kPackFrames];
	const int tid = threadIdx.x;
	const long long g0 = (long long)blockIdx.x * kPackFrames;
	if (tid < kPackFrames && g0 + tid < total) {
		const long long g = g0 + tid;
		int lo = 0, hi = n_desc - 1;  // the greatest u with out_off <= g: the stream that emits row g
		while (lo < hi) {
			const int mid = lo + (hi - lo + 1) / 2;
			if (desc[mid].out_off <= g) lo = mid;
			else hi = mid - 1;
		}
		s_d[tid] = lo;
	}
	__syncthreads();
	const int S = nd + 1 + n_ap;
	const size_t W = (size_t)orders * S + 1;
	for (int idx = tid; idx < kPackFrames * (S + 1); idx += 256) {
		const int fr = idx / (S + 1), c = idx - fr * (S + 1);
		const long long g = g0 + fr;
		if (g >= total) break;
		const FsDesc &d = desc[s_d[fr]];
		const long long t = d.e0 + (g - d.out_off), j = t + d.lag < d.last ? t + d.lag : d.last;
		int slot = d.slot_lo + (int)(t - d.lo);  // of frame t; t - lo <= the emitted frames < cap
		if (slot >= cap) slot -= cap;
		const double *here = ring + ((size_t)d.stream * cap + slot) * S;
		T *row = rows + (size_t)g * W;
		if (c == S) {
			const double l = here[nd];
			row[(size_t)orders * (nd + 1)] = (T)(l == l ? 1.0 : 0.0);
			continue;
		}
		int col0, cstep;
		ft_column(c, nd, n_ap, orders, &col0, &cstep);
		const bool lf0 = c == nd;
		const double *tr = triples + (size_t)g * 3;
		const double x0 = lf0 ? tr[1] : here[c];
		row[col0] = (T)x0;
		if (orders >= 2) {
			double xm = 0.0, xp = 0.0;
			if (t > 0) xm = lf0 ? tr[0] : ring[((size_t)d.stream * cap + (slot == 0 ? cap - 1 : slot - 1)) * S + c];
			if (t < j) xp = lf0 ? tr[2] : ring[((size_t)d.stream * cap + (slot + 1 == cap ? 0 : slot + 1)) * S + c];
			row[col0 + cstep] = (T)(0.5 * (xp - xm));
			if (orders == 3) row[col0 + 2 * cstep] = (T)((xm + xp) - 2.0 * x0);
		}
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct FsState : LagState {
	double fill = 0.0;
};

constexpr char kName[] = "feature stream";
int refuse(const std::string &what) { return fail(WC_ERR_INVALID, std::string(kName) + what); }

}  // namespace

struct wc_feature_stream : LagLedger<FsState> {
	Device *dev = nullptr;
	int nd = 0, n_ap = 0, orders = 0;
	// Ring slots are the absolute row index modulo cap = max_lag + max_rows_per_push + 1.  A push from T0 to T1 rows at lag L scans
	// rows T0 - L - 1 .. T1 - 1, the row before its first emitted frame up to its newest: at most max_lag + max_rows_per_push + 1 of
	// them, none of which shares a slot with the rows T0 .. T1 - 1 it writes.  A flush scans rows n - L - 1 .. n - 1.
	DevBuf ring;     // n_streams x cap x S doubles: the coded envelope, the parked log of F0 (NaN: unvoiced), the coded aperiodicity
	DevBuf carried;  // n_streams records
	DevBuf right;    // n_streams x cap ints: the suffix min-scan of a call, read back by the lane that wrote it
	DevBuf triples;  // n_streams x max(max_rows_per_push, max_lag) x 3 doubles: the continuous log-F0 of an emitted frame and its neighbours
	RecPair rec;     // the descriptors of a call
	void release_all() { ring.release(); carried.release(); right.release(); triples.release(); rec.release(); }
};

namespace {

// what both calls fill of a descriptor: the window and the frames of a stream that stands at `rows` rows behind this call
void window(const wc_feature_stream *h, const FsState &s, long long rows, int n_out, FsDesc *d) {
	d->e0 = s.emitted;
	d->last = rows - 1;
	d->lo = s.emitted > 0 ? s.emitted - 1 : 0;
	d->fill = s.fill;
	d->n_out = n_out;
	d->w = n_out > 0 ? (int)(rows - d->lo) : 0;
	d->lag = s.lag;
	d->slot_lo = (int)(d->lo % h->cap);
}

// the descriptors up in one copy, then the two kernels
int enqueue(wc_feature_stream *h, size_t n_desc, long long total_out, const double *d_f0, const double *d_sp, const double *d_ap,
			int out_format, void *d_rows) {
	Device *dev = h->dev;
	WC_HIP(hipSetDevice(dev->id));
	hipStream_t s = dev->active();
	const FsDesc *d_desc;
	int rc;
	if ((rc = h->rec.upload(s, sizeof(FsDesc) * n_desc, &d_desc))) return rc;
	if ((rc = dev->time_begin("feat_stream_scan_kernel", s))) return rc;
	hipLaunchKernelGGL(feat_stream_scan_kernel, dim3((unsigned)n_desc), dim3(64), 0, s, d_desc, h->nd, h->n_ap, h->cap, d_f0, d_sp, d_ap,
					   h->ring.as<double>(), h->carried.as<FsCarry>(), h->right.as<int>(), h->triples.as<double>());
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("feat_stream_scan_kernel", s))) return rc;
	if (total_out > 0) {
		const unsigned blocks = (unsigned)((total_out + kPackFrames - 1) / kPackFrames);
		if ((rc = dev->time_begin("feat_stream_pack_kernel", s))) return rc;
		if (out_format == WC_FEAT_F32)
			hipLaunchKernelGGL(feat_stream_pack_kernel<float>, dim3(blocks), dim3(256), 0, s, d_desc, (int)n_desc, total_out, h->nd, h->n_ap, h->orders,
							   h->cap, (const double *)h->ring.as<double>(), (const double *)h->triples.as<double>(), static_cast<float *>(d_rows));
		else
			hipLaunchKernelGGL(feat_stream_pack_kernel<double>, dim3(blocks), dim3(256), 0, s, d_desc, (int)n_desc, total_out, h->nd, h->n_ap, h->orders,
							   h->cap, (const double *)h->ring.as<double>(), (const double *)h->triples.as<double>(), static_cast<double *>(d_rows));
		WC_HIP(hipGetLastError());
		if ((rc = dev->time_end("feat_stream_pack_kernel", s))) return rc;
	}
	return WC_OK;
}

}  // namespace

extern "C" {

long long wc_feature_stream_emitted(long long rows, int lag) { return emitted_of(rows, lag); }

wc_feature_stream *wc_feature_stream_create(int n_streams, int nd, int n_ap, int orders, int max_rows_per_push, int max_lag) {
	const auto no = [](const char *why) { set_error(std::string(kName) + why); return (wc_feature_stream *)nullptr; };
	const unsigned long long S = (unsigned long long)nd + 1 + n_ap;  // doubles of a ring row
	if (const char *why = lag_check_dims(nd, n_ap)) return no(why);
	if (orders < 1 || orders > 3) return no(": orders is 1, 2 or 3");
	// (under the ring's bound the items of a take (max_rows_per_push x S), the triples and the block counts stay far below 2^31)
	if (const char *why = lag_check_create(wc_model_feature_width(nd, n_ap, orders), n_streams, max_rows_per_push, max_lag, S)) return no(why);
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	wc_feature_stream *h = new wc_feature_stream();
	h->dev = dev;
	h->init(n_streams, max_rows_per_push, max_lag);
	h->nd = nd; h->n_ap = n_ap; h->orders = orders;
	const size_t cap = (size_t)h->cap, ring_bytes = sizeof(double) * (size_t)S * cap;  // of one stream
	const size_t rec = sizeof(FsDesc) * (size_t)n_streams, most = (size_t)std::max(max_rows_per_push, max_lag);
	if (h->ring.reserve((size_t)ring_bytes * (size_t)n_streams) || h->carried.reserve(sizeof(FsCarry) * (size_t)n_streams) ||
		h->right.reserve(sizeof(int) * (size_t)cap * (size_t)n_streams) || h->triples.reserve(sizeof(double) * 3 * most * (size_t)n_streams) ||
		h->rec.reserve(rec)) {
		h->release_all();
		delete h;
		return nullptr;
	}
	// every byte 0xff: NaN in the ring and the triples, "none" in the records -- a row read before it was taken would show
	hipStream_t s = dev->active();
	const size_t n_bytes[4] = {(size_t)ring_bytes * (size_t)n_streams, sizeof(FsCarry) * (size_t)n_streams,
							   sizeof(int) * (size_t)cap * (size_t)n_streams, sizeof(double) * 3 * most * (size_t)n_streams};
	void *const bufs[4] = {h->ring.p, h->carried.p, h->right.p, h->triples.p};
	hipError_t e = hipSuccess;
	for (int i = 0; i < 4 && e == hipSuccess; ++i)
		if (n_bytes[i]) e = hipMemsetAsync(bufs[i], 0xff, n_bytes[i], s);
	if (e == hipSuccess) e = hipStreamSynchronize(s);
	if (e != hipSuccess) {
		set_error(std::string(kName) + ": " + hipGetErrorString(e));
		h->release_all();
		delete h;
		return nullptr;
	}
	return h;
}

void wc_feature_stream_destroy(wc_feature_stream *h) {
	if (!h) return;
	h->dev->quiesce();
	h->release_all();
	delete h;
}

int wc_feature_stream_reset(wc_feature_stream *h, int stream, int lag, double lf0_fill) {
	if (const char *why = lag_check_reset(h, stream, lag)) return refuse(why);
	if (lf0_fill != lf0_fill) return refuse(" reset: lf0_fill is NaN");
	DeviceLock lock(h->dev);
	FsState &s = h->st[stream];
	s = FsState();  // (neither the ring nor the carried record is cleared: no window reaches below row 0, where the record is not read)
	s.lag = lag;
	s.fill = lf0_fill;
	return WC_OK;
}

int wc_feature_stream_push_device(wc_feature_stream *h, const int *n_rows, const double *d_f0, const double *d_coded_sp, const double *d_coded_ap,
								  int out_format, void *d_rows, int *frames_out) {
	if (!h || !n_rows || !frames_out) return refuse(" push: null argument");
	if (out_format != WC_FEAT_F64 && out_format != WC_FEAT_F32) return refuse(" push: the format is 0 (double) or 1 (float)");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	long long total_rows, total_out;
	if (const char *why = h->scan_push(n_rows, &total_rows, &total_out)) return refuse(why);
	if (total_rows > 0 && (h->n_ap == 0) != (d_coded_ap == nullptr)) return refuse(" push: d_coded_ap is NULL exactly where n_ap is 0");
	if (total_rows > 0 && (!d_f0 || !d_coded_sp)) return refuse(" push: null array");
	if (total_out > 0 && !d_rows) return refuse(" push: null array");
	const unsigned long long W = (unsigned long long)wc_model_feature_width(h->nd, h->n_ap, h->orders), esz = out_format == WC_FEAT_F32 ? 4 : 8;
	const unsigned long long out_bytes = (unsigned long long)total_out * W * esz, rows_in = (unsigned long long)total_rows;
	if (overlap(d_rows, out_bytes, d_f0, 8ull * rows_in) || overlap(d_rows, out_bytes, d_coded_sp, 8ull * rows_in * h->nd) ||
		overlap(d_rows, out_bytes, d_coded_ap, 8ull * rows_in * h->n_ap))
		return refuse(" push: d_rows overlaps an input");
	// ---- no refusal is left: the descriptors ----
	FsDesc *desc = total_rows > 0 ? h->rec.begin<FsDesc>() : nullptr;  // (an empty call waits for nothing)
	if (total_rows > 0 && !desc) return WC_ERR_DEVICE;
	size_t n_desc = 0;
	long long in_off = 0, out_off = 0;
	for (int u = 0; u < n; ++u) {
		const FsState &s = h->st[u];
		const int k = n_rows[u];
		frames_out[u] = h->push_frames(u, k);
		if (k == 0) continue;
		const long long rows = s.rows + k;
		FsDesc &d = desc[n_desc++];
		window(h, s, rows, frames_out[u], &d);
		d.in_off = in_off; d.out_off = out_off;
		d.stream = u; d.k = k;
		d.slot0 = (int)(s.rows % h->cap);
		const long long e1 = s.emitted + frames_out[u];
		d.adv = (int)((e1 > 0 ? e1 - 1 : 0) - d.lo);  // (0 where nothing is emitted)
		in_off += k;
		out_off += frames_out[u];
	}
	if (n_desc == 0) return WC_OK;
	int rc;
	if ((rc = enqueue(h, n_desc, total_out, d_f0, d_coded_sp, d_coded_ap, out_format, d_rows))) return rc;
	h->commit_push(n_rows, frames_out);
	return WC_OK;
}

int wc_feature_stream_flush_device(wc_feature_stream *h, const int *want, int out_format, void *d_rows, int *frames_out) {
	if (!h || !want || !frames_out) return refuse(" flush: null argument");
	if (out_format != WC_FEAT_F64 && out_format != WC_FEAT_F32) return refuse(" flush: the format is 0 (double) or 1 (float)");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	long long total_out;
	if (const char *why = h->scan_flush(want, &total_out)) return refuse(why);
	if (total_out > 0 && !d_rows) return refuse(" flush: null array");
	// ---- no refusal is left: the same two kernels, nothing taken, every frame's prefix ending at the last row ----
	FsDesc *desc = total_out > 0 ? h->rec.begin<FsDesc>() : nullptr;
	if (total_out > 0 && !desc) return WC_ERR_DEVICE;
	size_t n_desc = 0;
	long long out_off = 0;
	for (int u = 0; u < n; ++u) {
		const FsState &s = h->st[u];
		frames_out[u] = h->flush_frames(u, want[u]);
		if (frames_out[u] == 0) continue;
		FsDesc &d = desc[n_desc++];
		window(h, s, s.rows, frames_out[u], &d);
		d.in_off = 0; d.out_off = out_off;
		d.stream = u; d.k = 0;
		d.slot0 = 0; d.adv = 0;
		out_off += frames_out[u];
	}
	if (n_desc) {
		int rc;
		if ((rc = enqueue(h, n_desc, total_out, nullptr, nullptr, nullptr, out_format, d_rows))) return rc;
	}
	h->commit_flush(want, frames_out);
	return WC_OK;
}

int wc_feature_stream_max_frames_per_push(const wc_feature_stream *h) { return lag_max_frames_per_push(h, WC_ERR_INVALID); }
int wc_feature_stream_max_frames_per_flush(const wc_feature_stream *h) { return lag_max_frames_per_flush(h, WC_ERR_INVALID); }

long long wc_feature_stream_rows_received(const wc_feature_stream *h, int stream) { return lag_rows_received(h, stream); }
long long wc_feature_stream_frames_emitted(const wc_feature_stream *h, int stream) { return lag_frames_emitted(h, stream); }
int wc_feature_stream_get_lag(const wc_feature_stream *h, int stream) { return lag_get_lag(h, stream); }

}  // extern "C"
