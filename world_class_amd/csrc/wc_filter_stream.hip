// Filter streams (include/world_class_filter_stream.h): frame filtering push by push, the whole call's bits.
//
// The host half -- counts, acceptance, refusals -- is wc_filter_stream_plan.hpp.  The response rows of a push are the batch's: the
// segment kernels of wc_filter.hip, reached through filter_segments_launch with one record per touched stream whose t0 is the stream's
// first segment of the push and whose offsets count from the window's first sample and row.  New here:
//   filter_stream_window_kernel       every touched stream's new windows into the other half of the pair: what is still pending of the
//                    old window, then what was pushed, samples and rows (slot 0 of the rows: the last row a done segment used).
//   filter_stream_overlap_add_kernel<N>  the outputs k in [C_before, a_{T_after-1} + N): each starts from the old tail's partial sum (0.0
//                    past the tail's end), adds the new rows' samples in segment order, and goes to y where k < C_after and to the new
//                    tail where k >= C_after; at a flush y[C .. n) and no tail.  One workgroup per tile of outputs; the segments that
//                    reach a tile follow from the c_t formula as in filter_overlap_add_kernel.  No atomics.
// Both kernels take a flat grid of (touched streams) x (tiles a stream can need at the handle's capacities), so that a push makes the
// same launches whatever the number of streams.  Every load and store is bounded by the stream's own counts of the push.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/world_class_filter_stream.h"
#include "wc_features_rows.hpp"
#include "wc_filter_stream_plan.hpp"
#include "wc_internal.hpp"
#include "wc_options.hpp"
#include "wc_stages.hpp"

namespace wc {

struct FsRec {  // one per touched stream
	long long x_old, x_new, x_push;     // doubles: the first pending sample of the old window, the new window, the stream's pushed samples
	long long r_old, r_new, r_push;     // rows: the old slot that becomes the new slot 0, the new slot 0, the stream's pushed rows
	long long tail_old, tail_new;       // doubles
	long long y_off, seg_off;           // the stream's outputs in d_y, its rows among the push's response rows
	long long C0, T0, T1;               // outputs committed and segments done in front of the push, segments done behind it
	int keep_s, ns;                     // samples: still pending of the old window, pushed
	int keep_r, nr;                     // rows: slots kept (slot 0 included; it holds nothing at T0 == 0), pushed
	int out, span;                      // outputs committed by the push; outputs handled (out + N, at a flush out)
	int tail_n, flush;
};

struct FsArgs {
	const FsRec *recs;
	const double *x_push, *r_push;  // the push's samples and rows
	double *xw, *rw, *tails;        // the handle's windows and tails
	const double *rows;             // the push's response rows
	double *y;
	double fp_ms;
	int fs, width, tiles_win, tiles_ola;  // width: doubles of a row
};

constexpr int FS_T = 256, FS_K = kFspTile / FS_T;

__global__ __launch_bounds__(FS_T) void filter_stream_window_kernel(FsArgs a) {
	const FsRec r = a.recs[blockIdx.x / a.tiles_win];
	const long long n_s = (long long)r.keep_s + r.ns, n_r = ((long long)r.keep_r + r.nr) * a.width;
	const long long e0 = (long long)(blockIdx.x % a.tiles_win) * kFspTile + threadIdx.x;
#pragma unroll
	for (int m = 0; m < FS_K; ++m) {
		const long long e = e0 + m * FS_T;
		if (e < n_s) {
			a.xw[r.x_new + e] = e < r.keep_s ? a.xw[r.x_old + e] : a.x_push[r.x_push + (e - r.keep_s)];
		} else if (e - n_s < n_r) {
			const long long q = e - n_s, slot = q / a.width, i = q - slot * a.width;
			if (slot == 0 && r.T0 == 0) continue;  // no segment is done: there is no row in front of the window
			a.rw[r.r_new * a.width + q] = slot < r.keep_r ? a.rw[(r.r_old + slot) * a.width + i] : a.r_push[(r.r_push + (slot - r.keep_r)) * a.width + i];
		}
	}
}

template <int N>
__global__ __launch_bounds__(FS_T) void filter_stream_overlap_add_kernel(FsArgs a) {
	const FsRec r = a.recs[blockIdx.x / a.tiles_ola];
	const long long e0 = (long long)(blockIdx.x % a.tiles_ola) * kFspTile;  // outputs count from C0
	if (e0 >= r.span) return;
	const long long k0 = r.C0 + e0, last = k0 + kFspTile - 1;
	const double h = a.fp_ms * (double)a.fs / 1000.0;
	// as filter_overlap_add_kernel: the estimate lies at or in front of the first segment that reaches the tile, the walk ends on it;
	// the segments in front of T0 have reached the tile through the tail
	const double est = floor((double)(k0 - N) / h) - 1.0;
	long long t = est > (double)r.T0 ? (long long)est : r.T0;
	auto start = [&](long long tt) { return tt ? ff_centre(tt - 1, a.fp_ms, a.fs) + 1 : 0ll; };
	while (t < r.T1 && start(t) + N <= k0) ++t;
	double acc[FS_K];
	const long long o0 = e0 + threadIdx.x;
#pragma unroll
	for (int m = 0; m < FS_K; ++m) {
		const long long e = o0 + m * FS_T;
		acc[m] = e < r.tail_n ? a.tails[r.tail_old + e] : 0.0;
	}
	const double *__restrict__ rows = a.rows + r.seg_off * N;
	constexpr int PB = 4;  // segments per trip: their loads are requested together, the additions stay in segment order
	for (; t < r.T1; t += PB) {
		if (start(t) > last) break;
		double v[PB][FS_K];
#pragma unroll
		for (int b = 0; b < PB; ++b) {
			const long long tt = min(t + b, r.T1 - 1);
			const long long st = start(tt);
			const bool on = t + b < r.T1 && st <= last;
#pragma unroll
			for (int m = 0; m < FS_K; ++m) {
				const long long j = r.C0 + o0 + m * FS_T - st;
				v[b][m] = (on && j >= 0 && j < N) ? rows[(tt - r.T0) * N + j] : 0.0;
			}
		}
#pragma unroll
		for (int b = 0; b < PB; ++b)
#pragma unroll
			for (int m = 0; m < FS_K; ++m) acc[m] += v[b][m];
	}
#pragma unroll
	for (int m = 0; m < FS_K; ++m) {
		const long long e = o0 + m * FS_T;
		if (e >= r.span) continue;
		if (e < r.out) a.y[r.y_off + e] = acc[m];
		else a.tails[r.tail_new + (e - r.out)] = acc[m];  // (span == out at a flush: no tail)
	}
}

}  // namespace wc

using namespace wc;

struct wc_filter_stream {
	FspPlan plan;
	int kind = 0;
	Device *dev = nullptr;
	bool block = false;  // WC_FILTER_KERNEL=block, as the batch
	RecPair rec;         // the push's records: FfUtt x (touched + 1), then FsRec x touched
	DevBuf xw, rw, tails;       // the pairs: 2 x n_streams x (max_pending_samples | (max_pending_rows + 1) rows | fft_size) doubles
	DevBuf rows, diff, dec;     // scratch of a push
	std::vector<FspStep> steps;
	hipEvent_t done = nullptr;  // behind the last call's kernels: a call on another stream waits for it on the device
	hipStream_t last = nullptr;
};

namespace {

int refuse(const char *why) { return fail(WC_ERR_INVALID, std::string("filter stream: ") + why); }

int take(wc_filter_stream *f, hipStream_t s) {
	if (f->done && f->last != s) WC_HIP(hipStreamWaitEvent(s, f->done, 0));
	return WC_OK;
}
int hand(wc_filter_stream *f, hipStream_t s) {
	if (!f->done) WC_HIP(hipEventCreateWithFlags(&f->done, hipEventDisableTiming));
	WC_HIP(hipEventRecord(f->done, s));
	f->last = s;
	return WC_OK;
}

struct Totals {
	long long s = 0, r = 0, out = 0, seg = 0;
	int active = 0;
};

// what both pushes refuse, in front of the first allocation; the steps are planned
int check(wc_filter_stream *f, const int *n_samples, const double *d_x, const int *n_rows, const int *flush, const double *d_y,
		  const int *samples_out, Totals *tot) {
	if (!f) return refuse("null handle");
	if (!n_samples || !n_rows || !samples_out) return refuse("null n_samples, n_rows or samples_out");
	if (const char *why = f->plan.plan_push(n_samples, n_rows, flush, f->steps, &tot->s, &tot->r, &tot->out, &tot->seg, &tot->active)) return refuse(why);
	if (tot->s > 0 && !d_x) return refuse("null d_x");
	if (tot->out > 0 && !d_y) return refuse("null d_y");
	if (overlap(d_y, 8ull * tot->out, d_x, 8ull * tot->s)) return refuse("d_y overlaps d_x");
	return WC_OK;
}

template <int N>
void launch_ola(const FsArgs &a, unsigned grid, hipStream_t s) {
	hipLaunchKernelGGL(filter_stream_overlap_add_kernel<N>, dim3(grid), dim3(FS_T), 0, s, a);
}

// the push behind its checks: d_rows are the pushed rows of the handle's kind
int enqueue(wc_filter_stream *f, hipStream_t s, const double *d_x, const double *d_rows, double *d_y, const Totals &tot) {
	const FspPlan &pl = f->plan;
	Device *dev = f->dev;
	const int N = pl.N, width = N / 2 + 1, nu = pl.n_streams, na = tot.active;
	const size_t bytes = sizeof(FfUtt) * ((size_t)na + 1) + sizeof(FsRec) * (size_t)na;
	char *h = f->rec.begin<char>(bytes);
	if (!h) return WC_ERR_DEVICE;
	int rc;
	if ((rc = f->rows.reserve(sizeof(double) * (size_t)tot.seg * N))) return rc;
	FfUtt *utts = reinterpret_cast<FfUtt *>(h);
	FsRec *recs = reinterpret_cast<FsRec *>(h + sizeof(FfUtt) * ((size_t)na + 1));
	long long xo = 0, ro = 0, so = 0, yo = 0;
	int i = 0;
	for (int u = 0; u < nu; ++u) {
		const FspStep &p = f->steps[(size_t)u];
		const FspState &st = pl.st[(size_t)u];
		if (p.active) {
			const long long xb_old = ((long long)st.cur * nu + u) * pl.max_s, xb_new = ((long long)(1 - st.cur) * nu + u) * pl.max_s;
			const long long rb_old = ((long long)st.cur * nu + u) * (pl.max_r + 1ll), rb_new = ((long long)(1 - st.cur) * nu + u) * (pl.max_r + 1ll);
			FsRec r;
			r.x_old = xb_old + (p.C0 - st.wb); r.x_new = xb_new; r.x_push = xo;
			r.r_old = rb_old + (p.T0 - st.rb); r.r_new = rb_new; r.r_push = ro;
			r.tail_old = ((long long)st.cur * nu + u) * N; r.tail_new = ((long long)(1 - st.cur) * nu + u) * N;
			r.y_off = yo; r.seg_off = so;
			r.C0 = p.C0; r.T0 = p.T0; r.T1 = p.T1;
			r.keep_s = (int)(p.n0 - p.C0); r.ns = p.ns;
			r.keep_r = (int)(p.F0 - p.T0) + 1; r.nr = p.nr;
			r.out = p.out; r.span = p.flush ? p.out : p.out + N;
			r.tail_n = p.tail_n; r.flush = p.flush ? 1 : 0;
			recs[i] = r;
			// the segments count from the new window: its first sample is a_T0, its slot 1 holds row T0
			utts[i] = FfUtt{xb_new, rb_new + 1, so, (int)(p.n1 - p.C0), (int)(p.F1 - p.T0), p.segs, (int)p.T0};
			++i;
		}
		xo += p.ns; ro += p.nr; so += p.segs; yo += p.out;
	}
	utts[na] = FfUtt{0, 0, so, 0, 0, 0, 0};
	const char *d_recs = nullptr;
	if ((rc = f->rec.upload(s, bytes, &d_recs))) return rc;
	FsArgs w;
	w.recs = reinterpret_cast<const FsRec *>(d_recs + sizeof(FfUtt) * ((size_t)na + 1));
	w.x_push = d_x; w.r_push = d_rows;
	w.xw = f->xw.as<double>(); w.rw = f->rw.as<double>(); w.tails = f->tails.as<double>();
	w.rows = f->rows.as<double>(); w.y = d_y;
	w.fp_ms = pl.fp_ms; w.fs = pl.fs; w.width = width;
	w.tiles_win = (int)(((long long)pl.max_s + (pl.max_r + 1ll) * width + kFspTile - 1) / kFspTile);
	w.tiles_ola = (int)(((long long)pl.max_s + N + kFspTile - 1) / kFspTile);
	if ((rc = dev->time_begin("filter_stream_window_kernel", s))) return rc;
	hipLaunchKernelGGL(filter_stream_window_kernel, dim3((unsigned)na * (unsigned)w.tiles_win), dim3(FS_T), 0, s, w);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("filter_stream_window_kernel", s))) return rc;
	if (tot.seg > 0) {
		FfArgs a;
		a.x = w.xw; a.gain = w.rw; a.rows = f->rows.as<double>(); a.y = nullptr;
		a.utts = reinterpret_cast<const FfUtt *>(d_recs); a.tw = dev->twiddle;
		a.total_seg = tot.seg; a.fp_ms = pl.fp_ms; a.n_utt = na; a.fs = pl.fs; a.kind = f->kind;
		if ((rc = filter_segments_launch(dev, s, N, f->block, a))) return rc;
	}
	if ((rc = dev->time_begin("filter_stream_overlap_add_kernel", s))) return rc;
	const unsigned grid = (unsigned)na * (unsigned)w.tiles_ola;
	if (N == 512) launch_ola<512>(w, grid, s);
	else if (N == 1024) launch_ola<1024>(w, grid, s);
	else if (N == 2048) launch_ola<2048>(w, grid, s);
	else launch_ola<4096>(w, grid, s);
	WC_HIP(hipGetLastError());
	return dev->time_end("filter_stream_overlap_add_kernel", s);
}

void finish(wc_filter_stream *f, int *samples_out) {
	for (int u = 0; u < f->plan.n_streams; ++u) samples_out[u] = f->steps[(size_t)u].out;
	f->plan.commit(f->steps);
}

bool setting_ok(int fs, double frame_period_ms) {
	const double h = ff_hop(frame_period_ms, fs);
	return fs > 0 && h >= 1.0 && h <= DBL_MAX;
}

}  // namespace

extern "C" {

long long wc_filter_stream_segments_done(int fs, double frame_period_ms, long long n, long long rows) {
	if (!setting_ok(fs, frame_period_ms) || n < 0 || rows < 0) return -1;
	return fsp_segments_done(frame_period_ms, fs, n, rows);
}

long long wc_filter_stream_committed(int fs, double frame_period_ms, long long segments_done) {
	if (!setting_ok(fs, frame_period_ms) || segments_done < 0) return -1;
	return fsp_committed(frame_period_ms, fs, segments_done);
}

wc_filter_stream *wc_filter_stream_create(int fs, int fft_size, double frame_period_ms, int kind, int n_streams, int max_pending_samples,
										  int max_pending_rows) {
	const auto no = [](const char *why) { set_error(std::string("filter stream create: ") + why); return (wc_filter_stream *)nullptr; };
	if (const char *why = ff_check_setting(fs, fft_size_supported(fft_size), fft_size, frame_period_ms)) return no(why);
	if (const char *why = FspPlan::check_create(fs, fft_size, frame_period_ms, kind, n_streams, max_pending_samples, max_pending_rows)) return no(why);
	Device *dev = current_device();
	if (!dev) return nullptr;
	wc_filter_stream *f = new wc_filter_stream();
	f->plan.init(fs, fft_size, frame_period_ms, n_streams, max_pending_samples, max_pending_rows);
	f->kind = kind;
	f->dev = dev;
	f->block = opt_is("WC_FILTER_KERNEL", "block");
	const size_t pairs = 2 * (size_t)n_streams;
	if (f->xw.reserve(sizeof(double) * pairs * (size_t)max_pending_samples) ||
		f->rw.reserve(sizeof(double) * pairs * ((size_t)max_pending_rows + 1) * (size_t)(fft_size / 2 + 1)) ||
		f->tails.reserve(sizeof(double) * pairs * (size_t)fft_size)) {
		wc_filter_stream_destroy(f);
		return nullptr;
	}
	return f;
}

void wc_filter_stream_destroy(wc_filter_stream *f) {
	if (!f) return;
	f->dev->quiesce();
	if (f->done) (void)hipEventDestroy(f->done);
	f->rec.release(); f->xw.release(); f->rw.release(); f->tails.release(); f->rows.release(); f->diff.release(); f->dec.release();
	delete f;
}

int wc_filter_stream_reset(wc_filter_stream *f, int stream) {
	if (!f) return refuse("null handle");
	if (!f->plan.ok(stream)) return refuse("reset: bad stream index");
	DeviceLock lock(f->dev);
	f->plan.reset(stream);
	return WC_OK;
}

int wc_filter_stream_push_device(wc_filter_stream *f, const int *n_samples, const double *d_x, const int *n_rows, const double *d_rows,
								 const int *flush, double *d_y, int *samples_out) {
	if (!f) return refuse("null handle");
	DeviceLock lock(f->dev);
	Totals tot;
	if (int rc = check(f, n_samples, d_x, n_rows, flush, d_y, samples_out, &tot)) return rc;
	if (tot.r > 0 && !d_rows) return refuse("null d_rows");
	if (overlap(d_y, 8ull * tot.out, d_rows, 8ull * tot.r * (f->plan.N / 2 + 1))) return refuse("d_y overlaps d_rows");
	if (tot.active == 0) { finish(f, samples_out); return WC_OK; }
	OnDeviceOf here(f->dev);
	hipStream_t s = f->dev->active();
	int rc;
	if ((rc = take(f, s))) return rc;
	if ((rc = enqueue(f, s, d_x, d_rows, d_y, tot))) return rc;
	if ((rc = hand(f, s))) return rc;
	finish(f, samples_out);
	return WC_OK;
}

int wc_filter_stream_push_coded_device(wc_filter_stream *f, const int *n_samples, const double *d_x, const int *n_rows,
									   const double *d_coded_to, const double *d_coded_from, int number_of_dimensions, int skip_energy,
									   const int *flush, double *d_y, int *samples_out) {
	if (!f) return refuse("null handle");
	DeviceLock lock(f->dev);
	Totals tot;
	if (int rc = check(f, n_samples, d_x, n_rows, flush, d_y, samples_out, &tot)) return rc;
	const int nd = number_of_dimensions, N = f->plan.N;
	if (f->kind != WC_FILTER_POWER) return refuse("a coded push needs a handle of kind WC_FILTER_POWER");
	if (nd < 1 || nd > N / 2) return refuse("number_of_dimensions outside 1 .. fft_size/2");
	if (tot.r > 0 && !d_coded_to) return refuse("null d_coded_to");
	const unsigned long long cb = 8ull * tot.r * nd;
	if (overlap(d_y, 8ull * tot.out, d_coded_to, cb) || overlap(d_y, 8ull * tot.out, d_coded_from, cb)) return refuse("d_y overlaps the coded rows");
	if (tot.active == 0) { finish(f, samples_out); return WC_OK; }
	Device *dev = f->dev;
	OnDeviceOf here(dev);
	hipStream_t s = dev->active();
	int rc;
	if (tot.r > 0) {
		const CodecPlan *pl;
		if ((rc = codec_plan(dev, f->plan.fs, N, false, &pl))) return rc;
		if ((rc = f->diff.reserve(sizeof(double) * (size_t)tot.r * nd))) return rc;
		if ((rc = f->dec.reserve(sizeof(double) * (size_t)tot.r * (N / 2 + 1)))) return rc;
		if ((rc = take(f, s))) return rc;
		if ((rc = filter_difference_launch(s, d_coded_to, d_coded_from, f->diff.as<double>(), tot.r * nd, nd, skip_energy))) return rc;
		if ((rc = codec_decode_sp_launch(dev, s, N, tot.r, nd, f->diff.as<double>(), f->dec.as<double>(), *pl))) return rc;
	} else if ((rc = take(f, s))) {
		return rc;
	}
	if ((rc = enqueue(f, s, d_x, f->dec.as<double>(), d_y, tot))) return rc;
	if ((rc = hand(f, s))) return rc;
	finish(f, samples_out);
	return WC_OK;
}

long long wc_filter_stream_samples_received(const wc_filter_stream *f, int stream) { return f && f->plan.ok(stream) ? f->plan.st[(size_t)stream].n : -1; }
long long wc_filter_stream_rows_received(const wc_filter_stream *f, int stream) { return f && f->plan.ok(stream) ? f->plan.st[(size_t)stream].F : -1; }
long long wc_filter_stream_segments_done_of(const wc_filter_stream *f, int stream) { return f && f->plan.ok(stream) ? f->plan.st[(size_t)stream].T : -1; }
long long wc_filter_stream_samples_committed(const wc_filter_stream *f, int stream) { return f && f->plan.ok(stream) ? f->plan.st[(size_t)stream].C : -1; }
int wc_filter_stream_pending_samples(const wc_filter_stream *f, int stream) { return f && f->plan.ok(stream) ? f->plan.pending_samples(stream) : -1; }
int wc_filter_stream_pending_rows(const wc_filter_stream *f, int stream) { return f && f->plan.ok(stream) ? f->plan.pending_rows(stream) : -1; }

}  // extern "C"
