// Alignment streams (include/world_class_align_stream.h: wc_align_stream): a live voice is followed row by row through a known
// track.  The streaming form of wc_align_features_ex_device (wc_align.hip) at step pattern 0, band 0 and an open end: row i of D
// needs row i - 1 of D and row i of d only, so a stream carries one row of D from push to push and every pushed row gets the
// open-end scan of its own row of D -- the position in the track and the cost so far.  Two launches per push, both bounded by
// counts the host wrote into the descriptors:
//
//   align_cost_kernel   (wc_align_cost.hpp, the whole call's kernel and so its rounding)  one AlPair per stream that has rows: the
//     pushed rows against the stream's track, W = m, no band, into the stream's part of the handle's d buffer.
//   align_stream_rows_kernel   one 64-lane wavefront per stream that has rows, no barrier, no LDS.  The rows are taken in passes of
//     up to 64: in a pass lane l owns pushed row i0 + l and does cell j = s - l at step s.  Lane l - 1 finished D(i - 1, j) one step
//     earlier and D(i - 1, j - 1) two steps earlier: the first arrives by one cross-lane move per step, the second is that move's
//     value of the step before; Dl is the lane's own last result.  Lane 0 takes Du / Dd from the stream's state row (D of the last
//     row before the pass; +inf in front of row 0), the lane of the pass's last row writes the new state row.  A stream has TWO
//     state rows and a pass reads one and writes the other, so within a pass no lane reads from memory a D that another lane wrote
//     (the principle of wc_align.hip); where a push takes more than one pass, a fence stands between a pass's last store and the
//     next pass's first load of that row.  Which row is current is host state, so a push that fails leaves the last good row.
//     Eight steps form a round: the eight local costs of the lane's row and (lane 0) eight cells of the state row are loaded
//     together, then the chain of three comparisons and one sum per cell runs on registers.  Each lane keeps its row's running
//     (best, j*) under the strict < of the open-end scan and writes d_position / d_cost when its row has ended.
//
//   A push is host arithmetic (every refusal), one asynchronous copy of the descriptors out of page-locked staging and the two
//   launches; set_track is one asynchronous device-to-device copy.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/world_class_io.h"
#include "../../include/world_class_stream.h"
#include "wc_align_cost.hpp"
#include "wc_stages.hpp"

using namespace wc;

namespace {

constexpr long long kAlignStreamMaxCells = 1ll << 28;  // n_streams x max_rows_per_push x max_track_frames: the whole call's cap

struct AsWork {
	long long out_off;  // first pushed row of the stream in the packed outputs
	long long d_off;    // the stream's local costs: n rows of m
	long long st_off;   // the stream's two state rows
	long long first;    // rows the stream had received before this push
	int n, m;           // rows pushed / rows of the track
	int parity;         // the state row that holds D of the last row before this push
	int flags;
};

struct AsArgs {
	const AsWork *work;
	const double *d;
	double *state;
	long long max_m;  // doubles per state row
	double *position, *cost;
};

__global__ __launch_bounds__(64) void align_stream_rows_kernel(AsArgs A) {
	const AsWork w = A.work[blockIdx.x];
	const int lane = threadIdx.x;
	const double inf = __builtin_inf();
	const int m = w.m;
	const bool open_begin = (w.flags & WC_ALIGN_OPEN_BEGIN) != 0;
	int par = w.parity;
	for (int i0 = 0; i0 < w.n; i0 += 64) {  // (the trip counts of this loop and of the two below are the wavefront's)
		const int R = min(64, w.n - i0);    // rows of this pass
		const bool mine = lane < R, last = lane == R - 1;
		const bool has_prev = w.first + i0 > 0;      // a row of D lies above the pass
		const bool row0 = w.first + i0 + lane == 0;  // this lane's row is row 0 of the stream
		const double *__restrict__ src = A.state + w.st_off + (long long)par * A.max_m;
		double *__restrict__ dst = A.state + w.st_off + (long long)(par ^ 1) * A.max_m;
		const double *__restrict__ drow = A.d + w.d_off + (long long)(mine ? i0 + lane : i0) * m;
		double cur = inf;   // this lane's last result: D(i, j - 1), and what lane + 1 takes as D(i, j) one step later
		double diag = inf;  // what came from above one step ago: D(i - 1, j - 1)
		double best = inf;
		int bj = -1;
		const int steps = m + R - 1;
		for (int s0 = 0; s0 < steps; s0 += AL_CHUNK) {
			double dv[AL_CHUNK], sv[AL_CHUNK];
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				const int j = s0 + k - lane;
				const bool in = mine && j >= 0 && j < m;
				dv[k] = in ? drow[j] : 0.0;
				sv[k] = in && lane == 0 && has_prev ? src[j] : inf;
			}
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				double up = __shfl_up(cur, 1);  // D(i - 1, j): lane - 1 did column j one step ago (every lane is here at every step)
				if (lane == 0) up = sv[k];
				const int j = s0 + k - lane;
				if (mine && j >= 0 && j < m) {
					const double Dd = diag, Du = up, Dl = cur;
					double b;
					if (Dd <= Du && Dd <= Dl) b = Dd;
					else if (Du <= Dl) b = Du;
					else b = Dl;
					const double D = (row0 && (open_begin || j == 0)) ? dv[k] : dv[k] + b;
					if (D < best) { best = D; bj = j; }
					if (last) dst[j] = D;
					cur = D;
				}
				diag = up;
			}
		}
		if (mine) {  // the open-end scan of row i: the lowest column of the least D, or no winner (NaN or +inf throughout)
			const long long o = w.out_off + i0 + lane;
			A.cost[o] = bj >= 0 ? best : cur;  // (cur: D(i, m - 1))
			A.position[o] = bj >= 0 ? (double)bj : __builtin_nan("");
		}
		par ^= 1;
		if (i0 + 64 < w.n) __threadfence();  // the new state row, before lane 0 of the next pass reads it
	}
}

}  // namespace

struct wc_align_stream {
	int dims, dim_begin, dim_end, n_streams, n_tracks, max_m, max_rows;
	Device *dev;
	struct Stream {
		int track = -1;      // -1: never reset
		int flags = 0;
		int parity = 0;      // the state row that holds D of the newest row
		long long rows = 0;  // rows received since the reset
	};
	std::vector<Stream> st;
	std::vector<int> track_m;  // rows per slot, 0: empty
	DevBuf tracks;             // n_tracks x max_m rows of dims
	DevBuf d;                  // n_streams x max_rows x max_m local costs
	DevBuf state;              // n_streams x 2 x max_m
	DevBuf drec;               // the descriptors of a push: AlPair per stream with rows | AsWork per stream with rows
	HostBuf h_rec[2];          // their page-locked staging: a pair, so that a push waits for the copy of the push before the last only
	int parity = 0;
};

namespace {

bool as_stream_ok(const wc_align_stream *h, int u) { return h && u >= 0 && u < h->n_streams; }
bool as_track_ok(const wc_align_stream *h, int t) { return h && t >= 0 && t < h->n_tracks; }

}  // namespace

extern "C" {

wc_align_stream *wc_align_stream_create(int dims, int dim_begin, int dim_end, int n_streams, int n_tracks, int max_track_frames,
										int max_rows_per_push) {
	if (dims < 1) { set_error("align stream: dims must be at least 1"); return nullptr; }
	if (dim_begin < 0 || dim_end > dims || dim_begin >= dim_end) { set_error("align stream: need 0 <= dim_begin < dim_end <= dims"); return nullptr; }
	if (n_streams < 1 || n_tracks < 1 || max_track_frames < 1 || max_rows_per_push < 1) {
		set_error("align stream: n_streams, n_tracks, max_track_frames and max_rows_per_push must be at least 1");
		return nullptr;
	}
	// (each factor is below 2^31 and the product of the first two is checked before the third comes in)
	const long long sr = (long long)n_streams * max_rows_per_push;
	if (sr > kAlignStreamMaxCells || sr * max_track_frames > kAlignStreamMaxCells) {
		set_error("align stream: n_streams x max_rows_per_push x max_track_frames above 2^28 cells");
		return nullptr;
	}
	const long long track_rows = (long long)n_tracks * max_track_frames;
	if (track_rows > kAlignStreamMaxCells || track_rows * dims > (1ll << 34)) {
		set_error("align stream: n_tracks x max_track_frames x dims too large");
		return nullptr;
	}
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	wc_align_stream *h = new wc_align_stream();
	h->dims = dims; h->dim_begin = dim_begin; h->dim_end = dim_end;
	h->n_streams = n_streams; h->n_tracks = n_tracks; h->max_m = max_track_frames; h->max_rows = max_rows_per_push;
	h->dev = dev;
	h->st.assign(n_streams, wc_align_stream::Stream());
	h->track_m.assign(n_tracks, 0);
	const size_t rec = (sizeof(AlPair) + sizeof(AsWork)) * (size_t)n_streams;
	if (h->tracks.reserve(sizeof(double) * (size_t)track_rows * dims) || h->d.reserve(sizeof(double) * (size_t)sr * max_track_frames) ||
		h->state.reserve(sizeof(double) * (size_t)2 * n_streams * max_track_frames) || h->drec.reserve(rec) || h->h_rec[0].reserve(rec) ||
		h->h_rec[1].reserve(rec)) {
		wc_align_stream_destroy(h);
		return nullptr;
	}
	return h;
}

void wc_align_stream_destroy(wc_align_stream *h) {
	if (!h) return;
	h->dev->quiesce();
	h->tracks.release(); h->d.release(); h->state.release(); h->drec.release(); h->h_rec[0].release(); h->h_rec[1].release();
	delete h;
}

int wc_align_stream_set_track_device(wc_align_stream *h, int track, int m, const double *d_feat_b) {
	if (!as_track_ok(h, track)) return fail(WC_ERR_INVALID, "align stream: bad track index");
	if (m < 1 || m > h->max_m) return fail(WC_ERR_INVALID, "align stream set_track: need 1 <= m <= max_track_frames");
	if (!d_feat_b) return fail(WC_ERR_INVALID, "align stream set_track: null rows");
	DeviceLock lock(h->dev);
	for (const auto &s : h->st)
		if (s.track == track && s.rows > 0)
			return fail(WC_ERR_INVALID, "align stream set_track: a stream that has received rows follows this track (reset it first)");
	WC_HIP(hipSetDevice(h->dev->id));
	double *to = h->tracks.as<double>() + (size_t)track * h->max_m * h->dims;
	WC_HIP(hipMemcpyAsync(to, d_feat_b, sizeof(double) * (size_t)m * h->dims, hipMemcpyDeviceToDevice, h->dev->active()));
	h->track_m[track] = m;
	return WC_OK;
}

int wc_align_stream_reset(wc_align_stream *h, int stream, int track, int flags) {
	if (!as_stream_ok(h, stream)) return fail(WC_ERR_INVALID, "align stream: bad stream index");
	if (!as_track_ok(h, track)) return fail(WC_ERR_INVALID, "align stream: bad track index");
	if (flags != 0 && flags != WC_ALIGN_OPEN_BEGIN) return fail(WC_ERR_INVALID, "align stream reset: flags must be 0 or WC_ALIGN_OPEN_BEGIN");
	DeviceLock lock(h->dev);
	if (h->track_m[track] == 0) return fail(WC_ERR_INVALID, "align stream reset: the track has not been set");
	wc_align_stream::Stream &s = h->st[stream];
	s.track = track; s.flags = flags; s.rows = 0;  // (the parity stays: row 0 reads no state row)
	return WC_OK;
}

int wc_align_stream_push_device(wc_align_stream *h, const int *n_rows, const double *d_feat_a, double *d_position, double *d_cost) {
	if (!h || !n_rows) return fail(WC_ERR_INVALID, "align stream push: null argument");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	long long total = 0;
	int active = 0;
	for (int u = 0; u < n; ++u) {
		if (n_rows[u] < 0) return fail(WC_ERR_INVALID, "align stream push: negative row count");
		if (n_rows[u] > h->max_rows) return fail(WC_ERR_INVALID, "align stream push: more than max_rows_per_push rows for one stream");
		if (n_rows[u] > 0 && h->st[u].track < 0) return fail(WC_ERR_INVALID, "align stream push: rows for a stream that was never reset onto a track");
		total += n_rows[u];
		active += n_rows[u] > 0;
	}
	if (total == 0) return WC_OK;
	if (!d_feat_a || !d_position || !d_cost) return fail(WC_ERR_INVALID, "align stream push: null array");
	// ---- the descriptors (no refusal is left) ----
	if (h->h_rec[h->parity].reserve(0)) return WC_ERR_DEVICE;  // (the copy of the push before the last has read this staging)
	AlPair *pairs = h->h_rec[h->parity].as<AlPair>();
	AsWork *work = reinterpret_cast<AsWork *>(pairs + active);
	long long off = 0, tiles = 0;
	int k = 0;
	for (int u = 0; u < n; ++u) {
		const int c = n_rows[u];
		if (c == 0) continue;
		const wc_align_stream::Stream &s = h->st[u];
		const int m = h->track_m[s.track];
		AlPair &q = pairs[k];
		q.a_off = off; q.b_off = (long long)s.track * h->max_m;
		q.cell_off = (long long)u * h->max_rows * h->max_m;
		q.path_off = 0; q.tile_off = tiles; q.B = -1;
		q.n = c; q.m = m; q.W = m;
		q.tiles_j = (m + AL_TILE - 1) / AL_TILE;
		tiles += (long long)((c + AL_TILE - 1) / AL_TILE) * q.tiles_j;
		AsWork &w = work[k];
		w.out_off = off; w.d_off = q.cell_off; w.st_off = (long long)u * 2 * h->max_m; w.first = s.rows;
		w.n = c; w.m = m; w.parity = s.parity; w.flags = s.flags;
		off += c;
		++k;
	}
	// (tiles <= cells / 1024 + rows + columns: far below 2^31)
	WC_HIP(hipSetDevice(h->dev->id));
	hipStream_t hs = h->dev->active();
	int rc;
	const size_t bytes = (sizeof(AlPair) + sizeof(AsWork)) * (size_t)active;
	WC_HIP(hipMemcpyAsync(h->drec.p, pairs, bytes, hipMemcpyHostToDevice, hs));
	if ((rc = h->h_rec[h->parity].mark(hs))) return rc;
	AlArgs a = {};
	a.pairs = h->drec.as<AlPair>();
	a.n_pairs = active; a.dims = h->dims; a.dim_begin = h->dim_begin; a.dim_end = h->dim_end;
	a.fa = d_feat_a; a.fb = h->tracks.as<double>();
	a.cells = h->d.as<double>();
	AsArgs x;
	x.work = reinterpret_cast<const AsWork *>(a.pairs + active);
	x.d = h->d.as<double>(); x.state = h->state.as<double>(); x.max_m = h->max_m;
	x.position = d_position; x.cost = d_cost;
	if ((rc = h->dev->time_begin("align_stream_cost_kernel", hs))) return rc;
	hipLaunchKernelGGL(align_cost_kernel, dim3((unsigned)tiles), dim3(256), 0, hs, a);
	WC_HIP(hipGetLastError());
	if ((rc = h->dev->time_end("align_stream_cost_kernel", hs))) return rc;
	if ((rc = h->dev->time_begin("align_stream_rows_kernel", hs))) return rc;
	hipLaunchKernelGGL(align_stream_rows_kernel, dim3((unsigned)active), dim3(64), 0, hs, x);
	WC_HIP(hipGetLastError());
	if ((rc = h->dev->time_end("align_stream_rows_kernel", hs))) return rc;
	for (int u = 0; u < n; ++u) {
		wc_align_stream::Stream &s = h->st[u];
		s.rows += n_rows[u];
		s.parity ^= ((n_rows[u] + 63) / 64) & 1;  // one flip per pass
	}
	h->parity = 1 - h->parity;
	return WC_OK;
}

long long wc_align_stream_rows_received(const wc_align_stream *h, int stream) {
	if (!as_stream_ok(h, stream)) return -1;
	return h->st[stream].rows;
}

int wc_align_stream_track_length(const wc_align_stream *h, int track) {
	if (!as_track_ok(h, track)) return -1;
	return h->track_m[track];
}

}  // extern "C"
