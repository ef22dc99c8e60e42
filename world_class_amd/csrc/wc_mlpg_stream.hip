// MLPG streams (include/world_class_mlpg_stream.h): settled statics from a lagged back-substitution.
//
//   mlpg_stream_forward_kernel  a lane per (stream with rows in the push, static column), the lanes of a wavefront on neighbouring
//                               static columns of one stream: it takes the carried state, and for every pushed row finishes the row
//                               before it now that its successor is known (final z / d into the ring) and parks the row's own l1,
//                               l2 and end quotient z_end / d_end.  It reads one half of the stream's state pair and writes the
//                               other.  The lane behind the static columns stores the rows' vuv.
//   mlpg_stream_back_kernel     a wavefront per (walk, group of 64 static columns): from a row's end quotient lag + 1 steps down the
//                               ring; a push has one walk per pushed row that emits and writes the frame the walk ends at, a flush
//                               one walk per stream and writes every frame it passes.
// Both loops are bounded by counts in the descriptors (<= max_rows_per_push, <= max_lag + 1); both ask for their rows a chunk ahead,
// as mlpg_kernel does.  Every expression follows the rule of world_class_features.h operation for operation (the tree is built with
// -ffp-contract=off); tests/mlpg_stream_rule.py is the same recursion in numpy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/world_class_mlpg_stream.h"
#include "wc_features_rows.hpp"
#include "wc_internal.hpp"
#include "wc_lag_stream.hpp"

using namespace wc;

namespace {

struct MsFwd {          // a stream with rows in this push
	long long row0;     // rows it had received before
	long long in_off;   // its first row in d_mean (and in d_var, per frame)
	int stream, k;      // k rows
	int slot0, from;    // ring slot of row row0; the half of its state pair the push reads (it writes the other)
};
struct MsBack {         // a walk of the back-substitution
	long long out_off;  // output row of the frame the walk ends at
	int stream, slot_top;  // ring slot of the row whose end quotient it starts at
	int steps, every;   // frames it passes; every: each of them is written (the flush), else the last one only
};
struct MsPQ {
	double p0, p1, p2, q0, q1, q2;
};
struct MsRaw {
	double m0, m1, m2, v0, v1, v2;
};
struct MsPark {
	double l1, l2, zd;
};
constexpr int kChunk = 8;    // rows asked for ahead of the walk
constexpr int kFields = 18;  // doubles of a lane's carried state
// the carried state of a lane, before its newest row t is finished
enum { kP1m, kP2m, kQ1m, kQ2m,           // p1, p2, q1, q2 of row t - 1
	   kP0, kP1, kP2, kQ0, kQ1, kQ2,     // p and q of row t
	   kD1, kD2, kZ1, kZ2,               // d and z of rows t - 1 and t - 2
	   kL1, kL2, kA2m, kBad };           // l1(t), l2(t), a2(t - 1); 1.0 once a variance was NaN or <= 0

template <class T>
__global__ __launch_bounds__(64) void mlpg_stream_forward_kernel(const MsFwd *__restrict__ fw, int groups, int nd, int n_ap, int orders, int cap,
																 const T *__restrict__ mean, const T *__restrict__ var, int var_per_frame,
																 double *__restrict__ state, double *__restrict__ ring) {
	const MsFwd f = fw[blockIdx.x / groups];
	const int S = nd + 1 + n_ap, k = f.k;
	const int c = (int)(blockIdx.x % groups) * 64 + (int)threadIdx.x;
	if (c > S) return;
	const size_t W = (size_t)orders * S + 1, RW = 4 * (size_t)S + 1;
	const T *M = mean + (size_t)f.in_off * W;
	double *R = ring + (size_t)f.stream * cap * RW;
	if (c == S) {  // vuv: parked with its row
		int slot = f.slot0;
		for (int j = 0; j < k; ++j) {
			R[(size_t)slot * RW + 4 * (size_t)S] = (double)M[(size_t)j * W + (size_t)orders * (nd + 1)];
			slot = slot + 1 == cap ? 0 : slot + 1;
		}
		return;
	}
	int col0, cstep;
	ft_column(c, nd, n_ap, orders, &col0, &cstep);
	const T *V = var + (var_per_frame ? (size_t)f.in_off * W : 0);
	const size_t vstep = var_per_frame ? W : 0;
	const double *sin = state + ((size_t)f.stream * 2 + f.from) * kFields * S + c;
	double *sout = state + ((size_t)f.stream * 2 + (1 - f.from)) * kFields * S + c;
	auto fetch = [&](int j) {  // the means and variances of pushed row j; nothing is read beyond the push
		MsRaw r = {0.0, 0.0, 0.0, 1.0, 1.0, 1.0};
		if (j < k) {
			const T *m = M + (size_t)j * W + col0, *v = V + (size_t)j * vstep + col0;
			r.m0 = (double)m[0]; r.m1 = (double)m[cstep];
			if (orders == 3) r.m2 = (double)m[2 * cstep];
			if (var_per_frame || j == 0) {  // (one row of variances is read once, at row 0)
				r.v0 = (double)v[0]; r.v1 = (double)v[cstep];
				if (orders == 3) r.v2 = (double)v[2 * cstep];
			}
		}
		return r;
	};
	MsRaw here[kChunk], ahead[kChunk];
#pragma unroll
	for (int j = 0; j < kChunk; ++j) here[j] = fetch(j);
	MsPQ cur = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	double p1m = 0.0, p2m = 0.0, q1m = 0.0, q2m = 0.0, d1 = 0.0, d2 = 0.0, z1 = 0.0, z2 = 0.0, l1c = 0.0, l2c = 0.0, a2m = 0.0;
	bool bad = false;
	if (f.row0 > 0) {
		p1m = sin[kP1m * (size_t)S]; p2m = sin[kP2m * (size_t)S]; q1m = sin[kQ1m * (size_t)S]; q2m = sin[kQ2m * (size_t)S];
		cur.p0 = sin[kP0 * (size_t)S]; cur.p1 = sin[kP1 * (size_t)S]; cur.p2 = sin[kP2 * (size_t)S];
		cur.q0 = sin[kQ0 * (size_t)S]; cur.q1 = sin[kQ1 * (size_t)S]; cur.q2 = sin[kQ2 * (size_t)S];
		d1 = sin[kD1 * (size_t)S]; d2 = sin[kD2 * (size_t)S]; z1 = sin[kZ1 * (size_t)S]; z2 = sin[kZ2 * (size_t)S];
		l1c = sin[kL1 * (size_t)S]; l2c = sin[kL2 * (size_t)S]; a2m = sin[kA2m * (size_t)S];
		bad = sin[kBad * (size_t)S] != 0.0;
	}
	// one row of variances for the push: its precisions are formed once (the same quotients: 1.0 / the same values)
	double g0 = 0.0, g1 = 0.0, g2 = 0.0;
	if (!var_per_frame) {
		const MsRaw &w = here[0];
		bad = bad || !(w.v0 > 0.0) || !(w.v1 > 0.0) || (orders == 3 && !(w.v2 > 0.0));
		g0 = 1.0 / w.v0;
		g1 = 1.0 / w.v1;
		g2 = orders == 3 ? 1.0 / w.v2 : 0.0;
	}
	auto convert = [&](const MsRaw &w) {  // precisions and weighted means of a pushed row
		MsPQ r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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
		return r;
	};
	const double nan = __longlong_as_double(0x7ff8000000000000ll);
	int slot = f.slot0, slot_m = f.slot0 == 0 ? cap - 1 : f.slot0 - 1;  // of row i and of row i - 1
	for (int base = 0; base < k; base += kChunk) {
#pragma unroll
		for (int j = 0; j < kChunk; ++j) ahead[j] = fetch(base + kChunk + j);
#pragma unroll
		for (int j = 0; j < kChunk; ++j) {
			if (base + j >= k) break;
			const long long i = f.row0 + base + j;
			const MsPQ next = convert(here[j]);
			if (i >= 1) {  // row t = i - 1 is finished: its successor is known
				const double a0 = (cur.p0 + 0.25 * (p1m + next.p1)) + ((p2m + next.p2) + 4.0 * cur.p2);
				const double a1 = -2.0 * (cur.p2 + next.p2);
				const double a2 = next.p2 - 0.25 * next.p1;
				const double r = (cur.q0 + 0.5 * (q1m - next.q1)) + ((q2m + next.q2) - 2.0 * cur.q2);
				double d = a0, z = r;
				if (i >= 3) d = d - (l2c * l2c) * d2;
				if (i >= 2) d = d - (l1c * l1c) * d1;
				if (i >= 3) z = z - l2c * z2;
				if (i >= 2) z = z - l1c * z1;
				R[(size_t)slot_m * RW + 2 * (size_t)S + c] = z / d;
				double l2n = 0.0, l1n;  // l2(i), l1(i)
				if (i >= 2) {
					l2n = a2m / d1;
					l1n = (a1 - (l2n * d1) * l1c) / d;
				} else {
					l1n = a1 / d;
				}
				d2 = d1; d1 = d; z2 = z1; z1 = z;
				l1c = l1n; l2c = l2n; a2m = a2;
				p1m = cur.p1; p2m = cur.p2; q1m = cur.q1; q2m = cur.q2;
			}
			cur = next;
			// row i as the last row of its prefix: the same expressions, the successor's p and q literal zeros
			const double a0e = (cur.p0 + 0.25 * (p1m + 0.0)) + ((p2m + 0.0) + 4.0 * cur.p2);
			const double re = (cur.q0 + 0.5 * (q1m - 0.0)) + ((q2m + 0.0) - 2.0 * cur.q2);
			double de = a0e, ze = re;
			if (i >= 2) de = de - (l2c * l2c) * d2;
			if (i >= 1) de = de - (l1c * l1c) * d1;
			if (i >= 2) ze = ze - l2c * z2;
			if (i >= 1) ze = ze - l1c * z1;
			double *pk = R + (size_t)slot * RW + c;
			pk[0] = l1c;
			pk[S] = l2c;
			pk[3 * (size_t)S] = bad ? nan : ze / de;
			slot_m = slot;
			slot = slot + 1 == cap ? 0 : slot + 1;
		}
#pragma unroll
		for (int j = 0; j < kChunk; ++j) here[j] = ahead[j];
	}
	sout[kP1m * (size_t)S] = p1m; sout[kP2m * (size_t)S] = p2m; sout[kQ1m * (size_t)S] = q1m; sout[kQ2m * (size_t)S] = q2m;
	sout[kP0 * (size_t)S] = cur.p0; sout[kP1 * (size_t)S] = cur.p1; sout[kP2 * (size_t)S] = cur.p2;
	sout[kQ0 * (size_t)S] = cur.q0; sout[kQ1 * (size_t)S] = cur.q1; sout[kQ2 * (size_t)S] = cur.q2;
	sout[kD1 * (size_t)S] = d1; sout[kD2 * (size_t)S] = d2; sout[kZ1 * (size_t)S] = z1; sout[kZ2 * (size_t)S] = z2;
	sout[kL1 * (size_t)S] = l1c; sout[kL2 * (size_t)S] = l2c; sout[kA2m * (size_t)S] = a2m;
	sout[kBad * (size_t)S] = bad ? 1.0 : 0.0;
}

__global__ __launch_bounds__(64) void mlpg_stream_back_kernel(const MsBack *__restrict__ bk, int groups, int nd, int n_ap, int cap,
															  const double *__restrict__ ring, double *__restrict__ out) {
	const MsBack b = bk[blockIdx.x / groups];
	const int S = nd + 1 + n_ap, steps = b.steps;
	const int c = (int)(blockIdx.x % groups) * 64 + (int)threadIdx.x;
	if (c > S) return;
	const size_t RW = 4 * (size_t)S + 1, W1 = (size_t)S + 1;
	const double *R = ring + (size_t)b.stream * cap * RW;
	double *O = out + (size_t)b.out_off * W1;  // the frame of step s stands steps - 1 - s rows behind it
	auto slot_of = [&](int s) {  // s <= max_lag < cap steps below the top
		const int v = b.slot_top - s;
		return v < 0 ? v + cap : v;
	};
	if (c == S) {  // vuv
		for (int s = b.every ? 0 : steps - 1; s < steps; ++s) O[(size_t)(steps - 1 - s) * W1 + nd + 1] = R[(size_t)slot_of(s) * RW + 4 * (size_t)S];
		return;
	}
	const int ocol = c <= nd ? c : c + 1;
	auto parked = [&](int s) {  // l1, l2 and the quotient of the row s steps below the top: the top's is its end quotient
		MsPark r = {0.0, 0.0, 0.0};
		if (s < steps) {
			const double *pk = R + (size_t)slot_of(s) * RW + c;
			r.l1 = pk[0]; r.l2 = pk[S]; r.zd = s == 0 ? pk[3 * (size_t)S] : pk[2 * (size_t)S];
		}
		return r;
	};
	MsPark back[kChunk], before[kChunk];
#pragma unroll
	for (int j = 0; j < kChunk; ++j) back[j] = parked(j);
	double c1 = 0.0, c2 = 0.0, l1n = 0.0, l2n = 0.0, l2nn = 0.0;  // c(t+1), c(t+2), l1(t+1), l2(t+1), l2(t+2)
	for (int base = 0; base < steps; base += kChunk) {
#pragma unroll
		for (int j = 0; j < kChunk; ++j) before[j] = parked(base + kChunk + j);
#pragma unroll
		for (int j = 0; j < kChunk; ++j) {
			const int s = base + j;
			if (s >= steps) break;
			double x = back[j].zd;
			if (s >= 1) x = x - l1n * c1;
			if (s >= 2) x = x - l2nn * c2;
			if (b.every || s == steps - 1) O[(size_t)(steps - 1 - s) * W1 + ocol] = x;
			c2 = c1; c1 = x; l2nn = l2n; l2n = back[j].l2; l1n = back[j].l1;
		}
#pragma unroll
		for (int j = 0; j < kChunk; ++j) back[j] = before[j];
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct MsState : LagState {
	int half = 0;  // where of its pair the carried state stands
};

constexpr char kName[] = "mlpg stream";
int refuse(const std::string &what) { return fail(WC_ERR_INVALID, std::string(kName) + what); }

}  // namespace

struct wc_mlpg_stream : LagLedger<MsState> {
	Device *dev = nullptr;
	int nd = 0, n_ap = 0, orders = 0;
	// Ring slots are the absolute row index modulo cap = max_lag + max_rows_per_push + 1.  A push from T0 to T1 rows at lag L reads
	// rows T0 - L .. T1 - 1 in its walks, at most max_lag + max_rows_per_push of them, and its forward kernel writes the final z / d of
	// the carried row T0 - 1, which lies below that range when L is 0: the one slot of margin keeps row T0 - 1 apart from row T1 - 1
	// then.  A flush reads rows n - L .. n - 1.
	DevBuf state;  // n_streams x 2 halves x kFields x S doubles
	DevBuf ring;   // n_streams x cap x (4 S + 1) doubles: l1, l2, z / d, z_end / d_end of every static column, vuv
	RecPair rec;   // the forward descriptors of a push, then its walks
	void release_all() { state.release(); ring.release(); rec.release(); }
};

namespace {

// the descriptors up in one copy, then the kernels: the forward kernel where rows were pushed, the back kernel where frames come out
int enqueue(wc_mlpg_stream *h, size_t n_fwd, size_t n_back, int in_format, const void *d_mean, const void *d_var, int var_per_frame,
			double *d_static) {
	Device *dev = h->dev;
	WC_HIP(hipSetDevice(dev->id));
	hipStream_t s = dev->active();
	const size_t bytes = sizeof(MsFwd) * n_fwd + sizeof(MsBack) * n_back;
	const MsFwd *d_fwd;
	int rc;
	if ((rc = h->rec.upload(s, bytes, &d_fwd))) return rc;
	const int S = h->nd + 1 + h->n_ap, groups = (S + 1 + 63) / 64;
	const MsBack *d_back = reinterpret_cast<const MsBack *>(d_fwd + n_fwd);
	if (n_fwd) {
		if ((rc = dev->time_begin("mlpg_stream_forward_kernel", s))) return rc;
		if (in_format == WC_FEAT_F32)
			hipLaunchKernelGGL(mlpg_stream_forward_kernel<float>, dim3((unsigned)(n_fwd * groups)), dim3(64), 0, s, d_fwd, groups, h->nd, h->n_ap, h->orders,
							   h->cap, static_cast<const float *>(d_mean), static_cast<const float *>(d_var), var_per_frame, h->state.as<double>(),
							   h->ring.as<double>());
		else
			hipLaunchKernelGGL(mlpg_stream_forward_kernel<double>, dim3((unsigned)(n_fwd * groups)), dim3(64), 0, s, d_fwd, groups, h->nd, h->n_ap, h->orders,
							   h->cap, static_cast<const double *>(d_mean), static_cast<const double *>(d_var), var_per_frame, h->state.as<double>(),
							   h->ring.as<double>());
		WC_HIP(hipGetLastError());
		if ((rc = dev->time_end("mlpg_stream_forward_kernel", s))) return rc;
	}
	if (n_back) {
		if ((rc = dev->time_begin("mlpg_stream_back_kernel", s))) return rc;
		hipLaunchKernelGGL(mlpg_stream_back_kernel, dim3((unsigned)(n_back * groups)), dim3(64), 0, s, d_back, groups, h->nd, h->n_ap, h->cap,
						   (const double *)h->ring.as<double>(), d_static);
		WC_HIP(hipGetLastError());
		if ((rc = dev->time_end("mlpg_stream_back_kernel", s))) return rc;
	}
	return WC_OK;
}

}  // namespace

extern "C" {

long long wc_mlpg_stream_emitted(long long rows, int lag) { return emitted_of(rows, lag); }

wc_mlpg_stream *wc_mlpg_stream_create(int n_streams, int nd, int n_ap, int orders, int max_rows_per_push, int max_lag) {
	const auto no = [](const char *why) { set_error(std::string(kName) + why); return (wc_mlpg_stream *)nullptr; };
	const unsigned long long S = (unsigned long long)nd + 1 + n_ap, row = 4 * S + 1;  // doubles of a ring row
	if (const char *why = lag_check_dims(nd, n_ap)) return no(why);
	if (orders < 2 || orders > 3) return no(": orders is 2 or 3");
	// (under the ring's bound a push's n_streams x max_rows_per_push walks, each over (S + 1 + 63) / 64 blocks, stay far below 2^31)
	if (const char *why = lag_check_create(wc_model_feature_width(nd, n_ap, orders), n_streams, max_rows_per_push, max_lag, row)) return no(why);
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	wc_mlpg_stream *h = new wc_mlpg_stream();
	h->dev = dev;
	h->init(n_streams, max_rows_per_push, max_lag);
	h->nd = nd; h->n_ap = n_ap; h->orders = orders;
	const size_t rec = (size_t)n_streams * (sizeof(MsFwd) + sizeof(MsBack) * (size_t)max_rows_per_push);
	if (h->state.reserve(sizeof(double) * 2 * kFields * (size_t)S * (size_t)n_streams) || h->ring.reserve(sizeof(double) * (size_t)row * (size_t)h->cap * (size_t)n_streams) ||
		h->rec.reserve(rec)) {
		h->release_all();
		delete h;
		return nullptr;
	}
	return h;
}

void wc_mlpg_stream_destroy(wc_mlpg_stream *h) {
	if (!h) return;
	h->dev->quiesce();
	h->release_all();
	delete h;
}

int wc_mlpg_stream_reset(wc_mlpg_stream *h, int stream, int lag) {
	if (const char *why = lag_check_reset(h, stream, lag)) return refuse(why);
	DeviceLock lock(h->dev);
	MsState &s = h->st[stream];
	const int half = s.half;  // (neither the state nor the ring is cleared: a stream with no rows reads neither, and no walk goes below row 0)
	s = MsState();
	s.half = half;
	s.lag = lag;
	return WC_OK;
}

int wc_mlpg_stream_push_device(wc_mlpg_stream *h, const int *n_rows, int in_format, const void *d_mean, const void *d_var, int var_per_frame,
							   double *d_static, int *frames_out) {
	if (!h || !n_rows || !frames_out) return refuse(" push: null argument");
	if (in_format != WC_FEAT_F64 && in_format != WC_FEAT_F32) return refuse(" push: the format is 0 (double) or 1 (float)");
	if (var_per_frame != 0 && var_per_frame != 1) return refuse(" push: var_per_frame is 0 or 1");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	long long total_rows, total_out;
	if (const char *why = h->scan_push(n_rows, &total_rows, &total_out)) return refuse(why);
	if (total_rows > 0 && (!d_mean || !d_var)) return refuse(" push: null array");
	if (total_out > 0 && !d_static) return refuse(" push: null array");
	const unsigned long long W = (unsigned long long)wc_model_feature_width(h->nd, h->n_ap, h->orders), esz = in_format == WC_FEAT_F32 ? 4 : 8;
	const unsigned long long S = (unsigned long long)h->nd + 1 + h->n_ap, out_bytes = 8ull * total_out * (S + 1);
	if (overlap(d_static, out_bytes, d_mean, (unsigned long long)total_rows * W * esz) ||
		overlap(d_static, out_bytes, d_var, (var_per_frame ? (unsigned long long)total_rows : (total_rows ? 1ull : 0ull)) * W * esz))
		return refuse(" push: d_static overlaps an input");
	// ---- no refusal is left: the descriptors ----
	MsFwd *fwd = total_rows > 0 ? h->rec.begin<MsFwd>() : nullptr;  // (an empty call waits for nothing)
	if (total_rows > 0 && !fwd) return WC_ERR_DEVICE;
	std::vector<MsBack> walks;
	size_t n_fwd = 0;
	long long in_off = 0, out_off = 0;
	for (int u = 0; u < n; ++u) {
		const MsState &s = h->st[u];
		const int k = n_rows[u];
		frames_out[u] = 0;
		if (k == 0) continue;
		MsFwd &f = fwd[n_fwd++];
		f.row0 = s.rows; f.in_off = in_off;
		f.stream = u; f.k = k;
		f.slot0 = (int)(s.rows % h->cap); f.from = s.half;
		for (int j = 0; j < k; ++j) {
			const long long i = s.rows + j;
			if (i < s.lag) continue;
			MsBack b;
			b.out_off = out_off + frames_out[u];
			b.stream = u; b.slot_top = (int)(i % h->cap);
			b.steps = s.lag + 1; b.every = 0;
			walks.push_back(b);
			++frames_out[u];
		}
		in_off += k;
		out_off += frames_out[u];
	}
	if (n_fwd == 0) return WC_OK;
	std::copy(walks.begin(), walks.end(), reinterpret_cast<MsBack *>(fwd + n_fwd));
	int rc;
	if ((rc = enqueue(h, n_fwd, walks.size(), in_format, d_mean, d_var, var_per_frame, d_static))) return rc;
	h->commit_push(n_rows, frames_out);
	for (int u = 0; u < n; ++u)
		if (n_rows[u] > 0) h->st[u].half = 1 - h->st[u].half;
	return WC_OK;
}

int wc_mlpg_stream_flush_device(wc_mlpg_stream *h, const int *want, double *d_static, int *frames_out) {
	if (!h || !want || !frames_out) return refuse(" flush: null argument");
	DeviceLock lock(h->dev);
	const int n = h->n_streams;
	long long total_out;
	if (const char *why = h->scan_flush(want, &total_out)) return refuse(why);
	if (total_out > 0 && !d_static) return refuse(" flush: null array");
	// ---- no refusal is left: a walk per stream with rows that wait ----
	MsBack *walks = total_out > 0 ? h->rec.begin<MsBack>() : nullptr;
	if (total_out > 0 && !walks) return WC_ERR_DEVICE;
	size_t n_back = 0;
	long long out_off = 0;
	for (int u = 0; u < n; ++u) {
		const MsState &s = h->st[u];
		frames_out[u] = h->flush_frames(u, want[u]);
		if (frames_out[u] == 0) continue;
		MsBack &b = walks[n_back++];
		b.out_off = out_off;
		b.stream = u; b.slot_top = (int)((s.rows - 1) % h->cap);
		b.steps = frames_out[u]; b.every = 1;
		out_off += frames_out[u];
	}
	if (n_back) {
		int rc;
		if ((rc = enqueue(h, 0, n_back, WC_FEAT_F64, nullptr, nullptr, 0, d_static))) return rc;
	}
	h->commit_flush(want, frames_out);
	return WC_OK;
}

int wc_mlpg_stream_max_frames_per_push(const wc_mlpg_stream *h) { return lag_max_frames_per_push(h, WC_ERR_INVALID); }
int wc_mlpg_stream_max_frames_per_flush(const wc_mlpg_stream *h) { return lag_max_frames_per_flush(h, WC_ERR_INVALID); }

long long wc_mlpg_stream_rows_received(const wc_mlpg_stream *h, int stream) { return lag_rows_received(h, stream); }
long long wc_mlpg_stream_frames_emitted(const wc_mlpg_stream *h, int stream) { return lag_frames_emitted(h, stream); }
int wc_mlpg_stream_get_lag(const wc_mlpg_stream *h, int stream) { return lag_get_lag(h, stream); }

}  // extern "C"
