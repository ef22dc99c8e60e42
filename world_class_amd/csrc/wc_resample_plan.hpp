// The host half of the two sample-rate converters, stated once: wc_resample.hip (rational ratios) and wc_vresample.hip (any ratio as
// a 32.32 step).  A converter keeps what only it knows -- the plan of a ratio, its tiling, its launch record's position fields, its
// two kernels and their one output function -- and takes from here everything around them: the filter's parameters and prototype,
// the table on the device with the local memory its tiled kernel asks for, the split of a launch's records into tiled and plain
// ones, the batch call and the stream handle.  `name` ("resample" / "vresample") leads every message.
//
//   A launch.  Its records stand in one array, those of the tiled mapping first (rs_sort_records: a record of at least tiled_min
//   outputs, where the handle has a tiled mapping), block0 counted per mapping; at most two kernels follow (rs_launch_pair).
//
//   A stream.  The last 2K samples as doubles at the head of one of a pair of buffers of cap = 2K + max_samples_per_push doubles; a
//   push widens the new samples behind them and writes the new last 2K to the head of the other buffer (resample_widen_kernel), then
//   the converter's kernels run on the buffer of this push, and the stream's parity flips.  The buffer's double b is the stream's
//   sample received - 2K + b.
//
//   A call plans on the host with every refusal in front of the first enqueue, so a refused call moves nothing; its records go up
//   with one asynchronous copy through the handle's record pair (RecPair, wc_internal.hpp); then the kernels are enqueued and the
//   plan becomes the state.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "wc_internal.hpp"
#include "wc_resample_dev.hpp"

namespace wc {
namespace {

// ---- the filter -----------------------------------------------------------------------------------------------------------------
constexpr long long kMaxTable = 1ll << 21;  // doubles

// the Kaiser-windowed sinc g(d) = s sinc(s d) w(d s / zeros), d in input samples
struct RsFilter {
	int zeros;
	double s, beta;
};

// the arguments both plans check alike: the refusal's text, or empty
std::string rs_filter_check(const char *name, int zeros, double rolloff, double beta) {
	const std::string p = std::string(name) + ": ";
	if (zeros < 0) return p + "zeros must be at least 1 (0: the default, 64)";
	if (!(rolloff >= 0.0 && rolloff <= 1.0)) return p + "rolloff must lie in (0, 1] (0.0: the default)";
	if (!std::isfinite(beta) || beta < 0.0) return p + "beta must be finite and not negative (0.0: the default)";
	if (beta > 700.0) return p + "beta above 700 (I0 overflows)";
	return std::string();
}

// checked arguments with their defaults; ratio: output rate over input rate at the handle's lowest
RsFilter rs_filter_of(int zeros, double rolloff, double beta, double ratio) {
	RsFilter f;
	f.zeros = zeros == 0 ? 64 : zeros;
	const double ro = rolloff == 0.0 ? 0.9475937167399596 : rolloff;
	f.beta = beta == 0.0 ? 14.769656459379492 : beta;
	f.s = ro * std::min(1.0, ratio);
	return f;
}

// K = ceil(zeros / s) for a table of per_tap doubles per tap row (L, or P (D+1)); 0 where the table would pass kMaxTable
int rs_half_width(const RsFilter &f, long long per_tap) {
	const double kd = std::ceil(f.zeros / f.s);
	if (!(kd <= (double)kMaxTable) || per_tap * (2 * (long long)kd + 1) > kMaxTable) return 0;
	return (int)kd;
}
std::string rs_table_refusal(const char *name) { return std::string(name) + ": a table of more than 2^21 doubles"; }

// the modified Bessel function of the first kind and order 0 by its power series: every term is positive, so the sum is good to a
// few ulp wherever it does not overflow
double bessel_i0(double x) {
	const double h = 0.25 * x * x;
	double term = 1.0, sum = 1.0;
	for (int k = 1; k < 4000; ++k) {
		term = term * h / ((double)k * k);
		sum += term;
		if (term < 1e-18 * sum) break;
	}
	return sum;
}

// g(d), with i0b = bessel_i0(f.beta)
double rs_prototype(const RsFilter &f, double i0b, double d) {
	const double pi = 3.14159265358979323846;
	const double u = d * f.s / f.zeros;
	const double w = std::fabs(u) < 1.0 ? bessel_i0(f.beta * std::sqrt(1.0 - u * u)) / i0b : 0.0;
	const double v = f.s * d;
	return f.s * (v == 0.0 ? 1.0 : std::sin(pi * v) / (pi * v)) * w;
}

// ---- the core: what a converter's batch handle and its stream handle share ---------------------------------------------------------
// the part of a converter's tiling that the split of a launch reads
struct RsTiles {
	int tile_out;         // outputs of a tile of the tiled mapping; 0: the plan has none
	int lds_bytes;        // local memory of its block
	int threads;          // of its block
	long long tiled_min;  // the tiled mapping from so many outputs of a record on
};

// Plan: K and what the converter's kernels read; Tiling: derives from RsTiles
template <class Plan, class Tiling> struct RsCore {
	Plan p;
	Tiling t;
	bool tiled = false;  // the tiled mapping is available
	Device *dev = nullptr;
	DevBuf table;
};

template <class Core> void rs_core_destroy(Core *c) {
	if (!c) return;
	c->table.release();
	delete c;
}

// The table of a checked plan built (build(double *), n_table doubles) and uploaded, and more than 64 KB of local memory asked for
// on the N variants of the tiled kernels; nullptr + error on failure.  tile_name: "the input tile" / "the tile".
template <class Core, class Plan, class Tiling, class Build, size_t N>
Core *rs_core_create(const char *name, const char *tile_name, const Plan &p, const Tiling &t, bool tiled, size_t n_table, Build build,
					 const void *const (&tiled_kernels)[N]) {
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	Core *c = new Core();
	c->p = p;
	c->t = t;
	c->tiled = tiled;
	c->dev = dev;
	std::vector<double> table(n_table);
	build(table.data());
	if (c->table.reserve(n_table * sizeof(double)) || hipMemcpy(c->table.p, table.data(), n_table * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
		set_error(std::string(name) + ": the table could not be uploaded");
		rs_core_destroy(c);
		return nullptr;
	}
	// a tile above the 64 KB every kernel may take has to be asked for.  The library is built for gfx950 alone, whose compute units
	// have the 160 KB that the tilings count on: a device that grants less is an error, not a reason to change the mapping quietly
	const size_t bytes = (size_t)t.lds_bytes;
	if (tiled && bytes > 65536) {
		int limit = 0;
		bool ok = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev->id) == hipSuccess && (size_t)limit >= bytes;
		for (size_t k = 0; k < N && ok; ++k)
			ok = hipFuncSetAttribute(tiled_kernels[k], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
		if (!ok) {
			(void)hipGetLastError();
			set_error(std::string(name) + ": the device grants " + std::to_string(limit) + " bytes of local memory per workgroup, " + tile_name + " needs " +
					  std::to_string(bytes));
			rs_core_destroy(c);
			return nullptr;
		}
	}
	return c;
}

// ---- the split of a launch ----------------------------------------------------------------------------------------------------------
template <class Core> bool rs_tiled(const Core &c, long long n_out) { return c.tiled && n_out >= c.t.tiled_min; }
template <class Core> int rs_rec_blocks(const Core &c, long long n_out) {
	return rs_tiled(c, n_out) ? (int)((n_out + c.t.tile_out - 1) / c.t.tile_out) : (int)((n_out + kPlainBlock - 1) / kPlainBlock);
}

// the host's records sorted into the staging (tiled records first, block0 assigned per launch)
struct RsSorted {
	int n_tiled = 0, n_plain = 0, blocks_tiled = 0, blocks_plain = 0;
};
template <class Core, class Rec> RsSorted rs_sort_records(const Core &c, const std::vector<Rec> &recs, Rec *to) {
	RsSorted s;
	for (const Rec &r : recs) s.n_tiled += rs_tiled(c, r.n_out) ? 1 : 0;
	int kt = 0, kq = s.n_tiled;
	for (const Rec &r : recs) {
		const bool tl = rs_tiled(c, r.n_out);
		Rec &d = to[tl ? kt++ : kq++];
		d = r;
		d.block0 = tl ? s.blocks_tiled : s.blocks_plain;
		(tl ? s.blocks_tiled : s.blocks_plain) += rs_rec_blocks(c, r.n_out);
	}
	s.n_plain = (int)recs.size() - s.n_tiled;
	return s;
}

// the sorted records are on the device: the tiled launch, then the plain launch (records without outputs take no block)
template <class Core, class Args, class Rec>
void rs_launch_pair(const Core &c, hipStream_t hs, Args a, const Rec *d_rec, const RsSorted &s, void (*tiled_kernel)(Args, const double *),
					void (*plain_kernel)(Args, const double *)) {
	if (s.blocks_tiled > 0) {
		a.rec = d_rec; a.n_rec = s.n_tiled;
		hipLaunchKernelGGL(tiled_kernel, dim3((unsigned)s.blocks_tiled), dim3(c.t.threads), (size_t)c.t.lds_bytes, hs, a, c.table.template as<double>());
	}
	if (s.blocks_plain > 0) {
		a.rec = d_rec + s.n_tiled; a.n_rec = s.n_plain;
		hipLaunchKernelGGL(plain_kernel, dim3((unsigned)s.blocks_plain), dim3(kPlainBlock), 0, hs, a, c.table.template as<double>());
	}
}

// a launch under the converter's timing label: launch() enqueues its pair
template <class Core, class Launch> int rs_timed(const Core &c, const char *label, hipStream_t hs, Launch launch) {
	int rc;
	if ((rc = c.dev->time_begin(label, hs))) return rc;
	launch();
	WC_HIP(hipGetLastError());
	return c.dev->time_end(label, hs);
}

// f(format) with the input format as a compile-time constant: decltype(format)::value
template <int N> using RsConst = std::integral_constant<int, N>;
template <class F> void rs_with_format(int fmt, F &&f) {
	if (fmt == 0) f(RsConst<0>());
	else if (fmt == 1) f(RsConst<1>());
	else f(RsConst<2>());
}

bool rs_format_ok(int in_format, int out_format) { return in_format >= 0 && in_format <= 2 && (out_format == 0 || out_format == 1); }
int rs_refuse(const char *name, const char *what) { return fail(WC_ERR_INVALID, std::string(name) + what); }

// ---- the batch handle -----------------------------------------------------------------------------------------------------------------
template <class Core> struct RsBatch {
	Core *c = nullptr;
	RecPair rec;  // grown to the call's records by every call
};

template <class H, class Core> H *rs_batch_create(Core *c) {
	if (!c) return nullptr;
	H *r = new H();
	r->c = c;
	return r;
}

template <class H> void rs_batch_destroy(H *r) {
	if (!r) return;
	r->c->dev->quiesce();
	r->rec.release();
	rs_core_destroy(r->c);
	delete r;
}

// The whole of a batch call: n_utt packed signals become n_utt records, which are sorted, uploaded and handed to the converter's
// launch.  arrays_ok: the converter's arrays are all there.  form(u, rec, &n_out) gives utterance u's output length (negative where
// it leaves 63 bits) and the record's position fields, or a refusal's text; enqueue(hs, d_rec, sorted) launches.
template <class Rec, class H, class Form, class Enqueue>
int rs_batch_run(const char *name, H *r, bool arrays_ok, int n_utt, int in_format, int out_format, const int *x_length, Form form, Enqueue enqueue) {
	if (!r || !arrays_ok) return rs_refuse(name, ": null argument");
	if (n_utt < 1) return rs_refuse(name, ": n_utt must be at least 1");
	if (!rs_format_ok(in_format, out_format)) return rs_refuse(name, ": in_format is 0, 1 or 2 and out_format 0 or 1");
	const auto &c = *r->c;
	DeviceLock lock(c.dev);
	std::vector<Rec> recs((size_t)n_utt);
	long long x_off = 0, y_off = 0;
	for (int u = 0; u < n_utt; ++u) {
		if (x_length[u] < 1) return rs_refuse(name, ": every length must be at least 1");
		Rec &q = recs[u];
		q = Rec();
		long long n_out = -1;
		if (const char *why = form(u, q, &n_out)) return rs_refuse(name, why);
		if (n_out < 0 || y_off + n_out > INT_MAX) return rs_refuse(name, ": the packed output exceeds 2^31 - 1 samples");
		q.x_off = x_off; q.y_off = y_off;
		q.lo = 0; q.hi = x_length[u];
		q.n_out = (int)n_out;
		x_off += x_length[u];
		y_off += n_out;
	}
	// ---- no refusal is left ----
	const size_t bytes = sizeof(Rec) * (size_t)n_utt;
	WC_HIP(hipSetDevice(c.dev->id));
	hipStream_t hs = c.dev->active();
	Rec *staged = r->rec.template begin<Rec>(bytes);
	if (!staged) return WC_ERR_DEVICE;
	const RsSorted s = rs_sort_records(c, recs, staged);
	const Rec *d_rec;
	if (int rc = r->rec.upload(hs, bytes, &d_rec)) return rc;
	return enqueue(hs, d_rec, s);
}

// ---- the stream handle ----------------------------------------------------------------------------------------------------------------
// what every stream has; a converter's State derives from it and adds its position, if it keeps one
struct RsStreamState {
	long long received = 0, committed = 0;
	int parity = 0;  // the buffer whose head holds the history
	bool flushed = false;
	// (the history is not cleared: the records say how much of it exists)
	void rewind() { received = 0; committed = 0; flushed = false; }
};

template <class Core, class State> struct RsStreams {
	Core *c = nullptr;
	int n_streams = 0, max_new = 0, max_out = 0;
	long long cap = 0;  // doubles per buffer: 2K + max_new
	std::vector<State> st;
	DevBuf buf;   // n_streams x 2 x cap
	RecPair rec;  // RsPush per stream with samples, then the converter's record per stream with outputs
};

bool rs_stream_counts_ok(const char *name, int n_streams, int max_samples_per_push) {
	if (n_streams >= 1 && max_samples_per_push >= 1) return true;
	set_error(std::string(name) + " stream: n_streams and max_samples_per_push must be at least 1");
	return false;
}

template <class H> void rs_stream_destroy(H *h) {
	if (!h) return;
	h->c->dev->quiesce();
	h->buf.release(); h->rec.release();
	rs_core_destroy(h->c);
	delete h;
}

// the handle around a core (nullptr: its create failed), with every array a push needs
template <class H, class Rec, class Core> H *rs_stream_create(Core *c, int n_streams, int max_samples_per_push, int max_out) {
	if (!c) return nullptr;
	DeviceLock lock(c->dev);
	H *h = new H();
	h->c = c;
	h->n_streams = n_streams; h->max_new = max_samples_per_push; h->max_out = max_out;
	h->cap = 2ll * c->p.K + max_samples_per_push;
	h->st.resize((size_t)n_streams);
	const size_t rec = (sizeof(RsPush) + sizeof(Rec)) * (size_t)n_streams;
	if (h->buf.reserve(sizeof(double) * (size_t)n_streams * 2 * (size_t)h->cap) || h->rec.reserve(rec)) {
		rs_stream_destroy(h);
		return nullptr;
	}
	return h;
}

template <class H> bool rs_stream_ok(const H *h, int stream) { return h && stream >= 0 && stream < h->n_streams; }
template <class H> int rs_stream_max_out(const H *h) { return h ? h->max_out : WC_ERR_INVALID; }
template <class H> long long rs_stream_received(const H *h, int stream) { return rs_stream_ok(h, stream) ? h->st[stream].received : -1; }
template <class H> long long rs_stream_committed(const H *h, int stream) { return rs_stream_ok(h, stream) ? h->st[stream].committed : -1; }

template <class H> int rs_stream_reset(const char *name, H *h, int stream) {
	if (!rs_stream_ok(h, stream)) return rs_refuse(name, " stream: bad stream index");
	DeviceLock lock(h->c->dev);
	h->st[stream].rewind();
	return WC_OK;
}

// The whole of a push.  The converter states three things: count(s, T, flushed) is the number of outputs stream s commits once it
// has T samples (negative: refused with count_refusal); first(s, rec) sets the position fields of its first output in the buffer
// of this push; advance(s, count) moves its position on.  enqueue(hs, d_rec, sorted, x) launches the converter's kernels on the
// buffers x, which hold doubles.
template <class Rec, class H, class Count, class First, class Advance, class Enqueue>
int rs_stream_push(const char *name, const char *count_refusal, H *h, const void *d_chunk, int in_format, const int *n_new, const int *flush, void *d_y,
				   int out_format, int *samples_out, Count count_of, First first, Advance advance, Enqueue enqueue) {
	if (!h || !n_new || !samples_out) return rs_refuse(name, " stream push: null argument");
	if (!rs_format_ok(in_format, out_format)) return rs_refuse(name, " stream push: in_format is 0, 1 or 2 and out_format 0 or 1");
	const auto &c = *h->c;
	DeviceLock lock(c.dev);
	const int n = h->n_streams, hist = 2 * c.p.K;
	std::vector<long long> count((size_t)n);
	long long total_in = 0, total_out = 0;
	int n_push = 0;
	for (int u = 0; u < n; ++u) {
		const auto &s = h->st[u];
		if (n_new[u] < 0 || n_new[u] > h->max_new) return rs_refuse(name, " stream push: a count outside 0 .. max_samples_per_push");
		if (s.flushed && n_new[u] > 0) return rs_refuse(name, " stream push: samples for a flushed stream (reset it first)");
		count[u] = count_of(s, s.received + n_new[u], s.flushed || (flush && flush[u]));
		if (count[u] < 0) return rs_refuse(name, count_refusal);
		total_in += n_new[u];
		total_out += count[u];
		n_push += n_new[u] > 0 ? 1 : 0;
	}
	if ((total_in > 0 && !d_chunk) || (total_out > 0 && !d_y)) return rs_refuse(name, " stream push: null array");
	// ---- no refusal is left: the records ----
	RsPush *push = h->rec.template begin<RsPush>();
	if (!push) return WC_ERR_DEVICE;
	std::vector<Rec> recs;
	long long c_off = 0, y_off = 0;
	int kp = 0, widen_blocks = 0;
	for (int u = 0; u < n; ++u) {
		const auto &s = h->st[u];
		const long long cur = ((long long)u * 2 + s.parity) * h->cap, other = ((long long)u * 2 + (1 - s.parity)) * h->cap;
		if (n_new[u] > 0) {
			RsPush &w = push[kp++];
			w.c_off = c_off; w.cur_off = cur; w.other_off = other;
			w.n_new = n_new[u]; w.block0 = widen_blocks;
			widen_blocks += (n_new[u] + hist + kPlainBlock - 1) / kPlainBlock;
		}
		samples_out[u] = (int)count[u];  // (<= max_out)
		if (count[u] > 0) {
			Rec q = Rec();
			first(s, q);
			q.x_off = cur; q.y_off = y_off;
			q.lo = s.received >= hist ? 0 : (int)(hist - s.received);
			q.hi = hist + n_new[u];
			q.n_out = (int)count[u];
			recs.push_back(q);
		}
		c_off += n_new[u];
		y_off += count[u];
	}
	WC_HIP(hipSetDevice(c.dev->id));
	hipStream_t hs = c.dev->active();
	if (n_push > 0 || !recs.empty()) {
		const RsSorted so = rs_sort_records(c, recs, reinterpret_cast<Rec *>(push + n_push));
		const size_t bytes = sizeof(RsPush) * (size_t)n_push + sizeof(Rec) * recs.size();
		const RsPush *d_push;
		int rc;
		if ((rc = h->rec.upload(hs, bytes, &d_push))) return rc;
		if (n_push > 0) {
			double *buf = h->buf.template as<double>();
			rs_with_format(in_format, [&](auto format) {
				hipLaunchKernelGGL(resample_widen_kernel<decltype(format)::value>, dim3((unsigned)widen_blocks), dim3(kPlainBlock), 0, hs, d_push, n_push, d_chunk, buf, hist);
			});
			WC_HIP(hipGetLastError());
		}
		if (!recs.empty() && (rc = enqueue(hs, reinterpret_cast<const Rec *>(d_push + n_push), so, (const void *)h->buf.p))) return rc;
	}
	for (int u = 0; u < n; ++u) {
		auto &s = h->st[u];
		advance(s, count[u]);
		s.received += n_new[u];
		s.committed += count[u];
		if (flush && flush[u]) s.flushed = true;
		if (n_new[u] > 0) s.parity = 1 - s.parity;
	}
	return WC_OK;
}

}  // namespace
}  // namespace wc
