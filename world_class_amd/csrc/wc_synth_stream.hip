// Chunked Synthesis for many concurrent streams (wc_synth_stream_*): include/world_class_stream.h states the semantics -- the
// samples a stream commits are those of ONE whole-utterance Synthesis over all of its frames (reference src/synthesis.cpp:77-177).
// Per push:
//   ss_frames_kernel     each stream's frame window (f0 / sp / ap rows still needed) moves to the other ping-pong buffer, the
//                        new frames appended
//   ss_increment_kernel  phase increments of the samples that became final (the sample-rate F0 / VUV of reference :180-243,
//                        absolute times i / fs, rows rebased into the window)
//   ss_timebase_kernel   one wavefront per stream: the reference's sequential phase sum (:255-262) continued from the carried
//                        total phase with chain64 (the batch's serial time base), wrap detection (:264-283), the pulse list
//                        (the pulse left waiting by the last push first) and the noise sizes (:106-107)
//   -- host: pulse counts, pending pulse, commit bound --
//   the batch's response kernels (syn_launch_responses) on the pulses whose successor is known
//   ss_overlap_kernel    carried partial sums + the new responses in pulse order (the batch's syn_overlap_add_kernel order):
//                        the committed prefix to the packed output, the rest to the other carry buffer
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "wc_stages.hpp"
#include "wc_synthesis.hpp"
#include "../../include/world_class_codec.h"
#include "../../include/world_class_stream.h"

namespace wc {

struct SsDesc {
	long long win_old, win_new;  // row offsets of the stream's window in the old / new buffer
	long long in_off;            // first new frame in the packed input
	int keep_from, keep, n_in;   // rows [keep_from, keep_from + keep) of the old window are kept, n_in new frames appended
	int f_base, f_len;           // absolute frame of new row 0; frames received after the push
	int n0, n1;                  // samples [n0, n1) become final in this push
	int cap;                     // slots of the stream's pulse list
	int has_pend, pend_idx, pend_vuv;
	double pend_shift;
	double run, wrap, vu;        // phase sum, wrapped phase and VUV of sample n0 - 1
	long long inc_off, slot;     // the stream's stretch of the increment scratch / first slot of its pulse list
};

struct SsOut {
	double run, wrap, vu, last_shift;
	int count, first_idx, last_idx, last_vuv;
};

struct OlDesc {
	long long src_off, dst_off, y_off;  // carried samples (sample lo), new carry (sample cut), packed output (sample lo)
	long long slot, pre;                // the stream's pulse list slots / first pulse of the compact numbering
	int src_len, lo, hi, cut, n_p;      // samples [lo, hi) are formed: [lo, cut) committed, [cut, hi) carried
};

__global__ void ss_frames_kernel(const SsDesc *__restrict__ desc, int bins, const double *__restrict__ of0, const double *__restrict__ osp,
								 const double *__restrict__ oap, const double *__restrict__ if0, const double *__restrict__ isp,
								 const double *__restrict__ iap, double *__restrict__ nf0, double *__restrict__ nsp, double *__restrict__ nap) {
	const SsDesc d = desc[blockIdx.y];
	const long long total = (long long)(d.keep + d.n_in) * bins;
	for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
		const int row = (int)(k / bins), c = (int)(k - (long long)row * bins);
		const long long dst = (d.win_new + row) * bins + c;
		if (row < d.keep) {
			const long long src = (d.win_old + d.keep_from + row) * bins + c;
			nsp[dst] = osp[src];
			nap[dst] = oap[src];
			if (c == 0) nf0[d.win_new + row] = of0[d.win_old + d.keep_from + row];
		} else {
			const long long src = (d.in_off + row - d.keep) * bins + c;
			nsp[dst] = isp[src];
			nap[dst] = iap[src];
			if (c == 0) nf0[d.win_new + row] = if0[d.in_off + row - d.keep];
		}
	}
}

// syn_increment_kernel for the final samples of a stream: 2 pi f0_i / fs, the sign carrying the VUV
__global__ void ss_increment_kernel(const SsDesc *__restrict__ desc, const double *__restrict__ wf0, int fs, int fft_size, double fp,
									double *__restrict__ inc) {
	const SsDesc d = desc[blockIdx.y];
	Coarse co{wf0 + d.win_new, d.f_len, fs / fft_size + 1.0, fp, d.f_base};  // integer division (reference :97)
	const double cval = 2.0 * kPi / fs;
	for (int i = d.n0 + blockIdx.x * blockDim.x + threadIdx.x; i < d.n1; i += gridDim.x * blockDim.x) {
		double f, v;
		co.at(i / (double)fs, f, v);  // time_axis[i] (reference :227), absolute
		const bool voiced = v > 0.5;
		f = voiced ? f : 500.0;
		const double dd = f * cval;
		inc[d.inc_off + (i - d.n0)] = voiced ? dd : -dd;
	}
}

// syn_timebase_kernel continued from the carried state of the stream (one wavefront per stream)
__global__ __launch_bounds__(64) void ss_timebase_kernel(const SsDesc *__restrict__ desc, const double *__restrict__ inc_all, int fs,
														 PulseBuf p, SsOut *__restrict__ out) {
	const SsDesc d = desc[blockIdx.x];
	const int lane = threadIdx.x;
	const int n = d.n1 - d.n0;
	const double *__restrict__ inc_g = inc_all + d.inc_off;
	const double two_pi = 2.0 * kPi;
	const long long slot0 = d.slot;
	double run = d.run, prev_wrap = d.wrap, prev_vu = d.vu;
	int cnt = 0;
	if (d.has_pend) {
		if (lane == 0) {
			p.index[slot0] = d.pend_idx;
			p.shift[slot0] = d.pend_shift;
			p.vuv[slot0] = d.pend_vuv;
		}
		cnt = 1;
	}
	for (int base = 0; base < n; base += 64) {
		const int i = d.n0 + base + lane;  // absolute sample index
		const double sv = inc_g[base + lane];  // padded with zeros past n
		const double vu = sv > 0.0 ? 1.0 : 0.0;
		double mine = run;
		const double *__restrict__ pu = inc_g + base;  // wave-uniform address: scalar loads
		chain64(mine, pu);
		const double wrap = fmod(mine, two_pi);
		double w_prev = __shfl_up(wrap, 1, 64);
		double v_prev = __shfl_up(vu, 1, 64);
		if (lane == 0) { w_prev = prev_wrap; v_prev = prev_vu; }
		// pulse between samples i-1 and i  <=>  |wrap[i] - wrap[i-1]| > pi ; the pulse sits at i-1 (reference :264-283)
		const bool is_pulse = (base + lane < n) && (i >= 1) && (fabs(wrap - w_prev) > kPi);
		const unsigned long long mask = __ballot(is_pulse);
		if (is_pulse) {
			const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
			if (slot < d.cap) {
				const double y1 = w_prev - two_pi, y2 = wrap;
				const double xx = -y1 / (y2 - y1);
				p.index[slot0 + slot] = i - 1;
				p.shift[slot0 + slot] = xx / fs;
				p.vuv[slot0 + slot] = v_prev > 0.5 ? 1 : 0;
			}
		}
		cnt += __popcll(mask);
		// the state of the last final sample (lanes past n hold padding)
		const int last = min(63, n - 1 - base);
		run = __shfl(mine, last, 64);
		prev_wrap = __shfl(wrap, last, 64);
		prev_vu = __shfl(vu, last, 64);
	}
	cnt = min(cnt, d.cap);  // (the host sizes the list for one pulse per sample: never taken)
	__threadfence();
	__syncthreads();
	// noise_size = samples to the next pulse (reference :106-107); the last entry's is 0 (at a flush it is the utterance's last
	// pulse; otherwise it waits for its successor and is not synthesised in this push)
	for (int j = lane; j < cnt; j += 64) p.noise_size[slot0 + j] = (j + 1 < cnt) ? p.index[slot0 + j + 1] - p.index[slot0 + j] : 0;
	if (lane == 0) {
		SsOut o;
		o.run = run; o.wrap = prev_wrap; o.vu = prev_vu;
		o.count = cnt;
		o.first_idx = cnt > 0 ? p.index[slot0] : 0;
		o.last_idx = cnt > 0 ? p.index[slot0 + cnt - 1] : 0;
		o.last_shift = cnt > 0 ? p.shift[slot0 + cnt - 1] : 0.0;
		o.last_vuv = cnt > 0 ? p.vuv[slot0 + cnt - 1] : 0;
		out[blockIdx.x] = o;
	}
}

// Carried partial sums plus the response rows of the stream's newly final pulses, in pulse order (syn_overlap_add_kernel's tiles
// and order: reference :118-139, y[index + 1 + j] += response[j] pulse after pulse); rows == nullptr: no pulses, a copy that
// splits [lo, hi) into the committed and the carried part
constexpr int SS_T = 256, SS_K = 4, SS_TILE = SS_T * SS_K;
template <int N>
__global__ __launch_bounds__(SS_T) void ss_overlap_kernel(const OlDesc *__restrict__ desc, const int *__restrict__ pidx_all,
														  const double *__restrict__ rows_all, const double *__restrict__ src,
														  double *__restrict__ y, double *__restrict__ dst) {
	constexpr int M = N / 2;
	const OlDesc d = desc[blockIdx.y];
	const int t0 = d.lo + blockIdx.x * SS_TILE;
	if (t0 >= d.hi) return;
	const int n_p = rows_all ? d.n_p : 0;
	const int *__restrict__ pidx = pidx_all + d.slot;
	int lo = 0, hi = n_p;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (pidx[mid] < t0 - M) lo = mid + 1; else hi = mid;
	}
	const int last = t0 + SS_TILE - 2 + M;
	const int o0 = t0 + threadIdx.x;
	double acc[SS_K];
#pragma unroll
	for (int m = 0; m < SS_K; ++m) {
		const int o = o0 + m * SS_T;
		acc[m] = (o < d.hi && o - d.lo < d.src_len) ? src[d.src_off + (o - d.lo)] : 0.0;
	}
	const double *__restrict__ rows = rows_all ? rows_all + d.pre * N : nullptr;
	for (int i = lo; i < n_p; ++i) {
		if (pidx[i] > last) break;
		const int start = pidx[i] - M + 1;
#pragma unroll
		for (int m = 0; m < SS_K; ++m) {
			const int j = o0 + m * SS_T - start;
			acc[m] += (j >= 0 && j < N) ? rows[(long long)i * N + j] : 0.0;
		}
	}
#pragma unroll
	for (int m = 0; m < SS_K; ++m) {
		const int o = o0 + m * SS_T;
		if (o >= d.hi) continue;
		if (o < d.cut) y[d.y_off + (o - d.lo)] = acc[m];
		else dst[d.dst_off + (o - d.cut)] = acc[m];
	}
}

}  // namespace wc

using namespace wc;

// ---- the host half.  A push is one sequence (ss_push): check the arguments; lock, set the device, snapshot the state; plan the
// source side and the core on the host, where every refusal that depends on the arguments and the handle's state is made; only
// then reserve and enqueue -- the source side, the core up to the SsOut read-back -- commit on the host, enqueue the responses and
// the overlap-add, synchronise, note where each stream's newest source row now is and keep the state.
namespace {
// Where source frame src - 1 of a stream is: the row a push that retimes the stream interpolates from in front of its own frames.
//   None    no frame yet
//   Window  not retimed: the newest row of the frame window, which went in unmodified
//   Kept    not retimed: that row was scaled or stretched on its way in; the frame's coded row (nd coefficients) was kept on `side`
//           of a ping-pong pair (tf0 / tcsp / tcap) and is decoded if the stream becomes retimed
//   Lost    not retimed: scaled or stretched, and nothing was kept (kTailMissing)
//   Pair    retimed: on `side` of the pair of carried rows (cf0 / csp / cap)
struct SsPrev {
	enum Where { None, Window, Kept, Lost, Pair } where = None;
	int side = 0, nd = 0;  // (the side stays while Window / Lost: the next kept frame goes to the other one)
};

struct SsState {
	// -- the core's: what the frames a stream synthesises from have come to
	int F = 0;          // frames received
	int wbase = 0;      // absolute frame of window row 0
	int wlen = 0;       // rows in the window
	int n_fin = 0;      // samples whose phase is final
	int cut = 0;        // samples committed
	int clen = 0;       // carried partial sums (samples cut .. cut + clen)
	int has_pend = 0, pend_idx = 0, pend_vuv = 0;
	double pend_shift = 0.0;
	double run = 0.0, wrap = 0.0, vu = 0.0;
	unsigned long long rng_pos = 0;  // noise position of the pending (or next) pulse
	long long frames = 0, samples = 0;
	bool closed = false;
	// -- the source side's: what a stream synthesises from what it is given
	double mod_f0 = 1.0, mod_ratio = 0.0;  // wc_synth_stream_set_modification: what coded pushes apply to this stream's frames
	bool neutral() const { return mod_f0 == 1.0 && mod_ratio == 0.0; }
	// wc_synth_stream_set_speed.  A stream that is not retimed has no state of its own here but prev: its source frames are its frames.
	double speed = 1.0;
	bool retimed = false;    // formed along the time map since the first push with frames at a speed other than 1.0
	bool speed_set = false;  // wc_synth_stream_set_speed was called since create / reset: the stream may become retimed mid-stream
	bool formed = false;     // retimed: a synthesis frame exists, at source position `last`
	double last = 0.0;
	long long src = 0;       // retimed: source frames received (F counts the synthesis frames)
	SsPrev prev;
};
}  // namespace

struct wc_synth_stream {
	int fs, fft_size, n_streams, max_frames, fp_ms_x1000;
	double frame_period;  // seconds
	int gap, wcap, ccap, wsz;  // pulse gap bound (samples), window rows, carried samples, samples formed per push
	Device *dev;
	wc_synthesis *sy;
	std::vector<SsState> st;
	int parity = 0;
	DevBuf wf0[2], wsp[2], wap[2], carry[2], work, inc, pulses, resp, meta, owner, aux, cls;
	DevBuf dsp, dap;  // wc_synth_stream_push_coded_device: the pushed frames' decoded rows (max_frames x n_streams, on first use)
	// a coded push with wc_synth_stream_set_modification settings: per-frame spectral ratios | F0 scales (2 x max_frames x n_streams,
	// staged through h_mod, the source side's own: the core behind it stages its metadata through h_stage) and the scaled F0
	DevBuf dmod, sf0;
	// retimed pushes (wc_synth_stream_set_speed), reserved on the first one: the carried source rows (two sides x n_streams), the
	// retimed rows and F0 (max_frames x n_streams), descriptors | positions | scales | ratios | descriptor indices staged through h_rt
	DevBuf cf0, csp, cap, rf0, rsp, rap, drt;
	// the newest coded frame of every stream with a modification setting (F0 | fft_size/2 coefficients | the bands, per stream),
	// kept by the coded pushes that apply a setting
	DevBuf tf0, tcsp, tcap;  // (two sides x n_streams)
	HostBuf h_stage, h_mod, h_rt;
};

namespace {
// A push that fails at any point leaves every stream where it was: the host state is restored, and the device buffers of the
// streams are ping-pong pairs whose old side is only given up by the state of a push that succeeded.  Taken once per push, behind
// the lock.
struct SsGuard {
	wc_synth_stream *s;
	std::vector<SsState> st;
	int parity;
	bool keep = false;
	explicit SsGuard(wc_synth_stream *x) : s(x), st(x->st), parity(x->parity) {}
	~SsGuard() {
		if (keep) return;
		s->st = st;
		s->parity = parity;
	}
};

// first sample whose time i / fs is not below (F - 1) frame periods: samples before it are final once F frames are in
int final_limit(const wc_synth_stream *s, int F) {
	if (F < 2) return 0;
	const double edge = (double)(F - 1) * s->frame_period;  // Coarse::at's (j + 1) * fp
	long long g = (long long)std::floor(edge * s->fs) - 2;
	if (g < 0) g = 0;
	while (g / (double)s->fs < edge) ++g;
	return (int)std::min<long long>(g, INT_MAX);
}

int frame_of(const wc_synth_stream *s, int i) { return (int)std::floor(i / (double)s->fs / s->frame_period); }

// The newest coded frame of the streams of a coded push that have a modification setting and may be given a speed later (tail[u]: its
// index in the packed arrays, as a double; negative: none) to the handle: the source row such a stream carries if it becomes
// retimed.  tail[n_streams + u]: the row of the pair it goes to (side * n_streams + u, the side the stream does not hold)
__global__ void ss_keep_tail_kernel(const double *__restrict__ tail, const double *__restrict__ f0, const double *__restrict__ csp,
									const double *__restrict__ cap, int nd, int n_ap, int stride, double *__restrict__ tf0,
									double *__restrict__ tcsp, double *__restrict__ tcap) {
	const int u = blockIdx.x;
	if (tail[u] < 0.0) return;
	const long long i = (long long)tail[u], r = (long long)tail[gridDim.x + u];
	if (threadIdx.x == 0) tf0[r] = f0[i];
	for (int k = threadIdx.x; k < nd; k += blockDim.x) tcsp[r * stride + k] = csp[i * nd + k];
	for (int k = threadIdx.x; k < n_ap; k += blockDim.x) tcap[r * n_ap + k] = cap[i * n_ap + k];
}

// ---- wc_synth_stream_set_speed: the rule (host arithmetic, the same for every fft size) ----
// whether a push of n source frames treats the stream along its time map
bool ss_follows_map(const SsState &q, int n) { return q.retimed || (n > 0 && q.speed != 1.0); }

// The stream takes n source frames and forms its synthesis frames: p = last + speed (0.0 for the first) while p <= F - 1.  Returns
// their number, positions appended to pos, or limit + 1 as soon as there would be more than limit (q is then half way: callers work
// on a copy or under the guard).
int ss_form(SsState &q, int n, int limit, std::vector<double> *pos) {
	if (!q.retimed) {  // becomes retimed: so far its frames sat at whole positions
		q.retimed = true;
		q.src = q.F;
		q.formed = q.F > 0;
		q.last = q.F - 1.0;
	}
	q.src += n;
	int c = 0;
	for (;;) {
		const double p = q.formed ? q.last + q.speed : 0.0;
		if (!(p <= (double)(q.src - 1))) return c;
		if (c == limit) return limit + 1;
		if (pos) pos->push_back(p);
		q.last = p;
		q.formed = true;
		++c;
	}
}

// A stream about to become retimed whose newest frame was decoded with a modification setting and whose coded frame was not kept:
// it has no source row to carry.  (The kept frame costs a launch per coded push, so only streams that called
// wc_synth_stream_set_speed before that push pay for it.)
bool ss_tail_missing(const SsState &q) { return q.prev.where == SsPrev::Lost; }
const char *const kTailMissing =
	"synthesis stream: a stream whose frames were decoded with a modification setting becomes retimed mid-stream only if "
	"wc_synth_stream_set_speed was called for it (1.0 will do) before its newest frame was pushed";

// a push runs the retimed path if a stream that receives frames follows its map (or a lowered speed lets one form a frame without)
bool ss_push_is_retimed(const wc_synth_stream *s, const int *n_frames) {
	for (int u = 0; u < s->n_streams; ++u) {
		const SsState &q = s->st[u];
		if (q.closed) continue;
		if (n_frames[u] > 0 ? ss_follows_map(q, n_frames[u]) : (q.retimed && q.formed && q.last + q.speed <= (double)(q.src - 1))) return true;
	}
	return false;
}

__global__ void ss_scale_f0_kernel(const double *__restrict__ f0, const double *__restrict__ scale, long long n, double *__restrict__ out) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = f0[i] * scale[i];
}
}  // namespace

extern "C" {

wc_synth_stream *wc_synth_stream_create(int fs, int fft_size, double frame_period_ms, int n_streams, int max_frames_per_push) {
	if (n_streams <= 0 || max_frames_per_push <= 0) { set_error("synthesis stream: n_streams and max_frames_per_push must be positive"); return nullptr; }
	wc_synthesis *sy = wc_synthesis_create(fs, fft_size, frame_period_ms);
	if (!sy) return nullptr;
	wc_synth_stream *s = new wc_synth_stream();
	s->fs = fs; s->fft_size = fft_size; s->n_streams = n_streams; s->max_frames = max_frames_per_push;
	s->frame_period = frame_period_ms / 1000.;  // reference :31
	s->dev = syn_device(sy);
	s->sy = sy;
	const double lowest = fs / fft_size + 1.0;  // reference :97 (integer division)
	// voiced: the interpolated F0 stays above lowest / 2 (a voiced sample lies within half a frame of a voiced frame); unvoiced: 500 Hz
	s->gap = (int)std::ceil(std::max(2.0 * fs / lowest, fs / 500.0)) + 4;
	const double spf = s->frame_period * fs;
	s->wcap = max_frames_per_push + (int)std::ceil((s->gap + fft_size + 2.0 * spf) / spf) + 8;
	s->ccap = s->gap + fft_size + 64;
	s->wsz = (int)((max_frames_per_push + 2) * std::ceil(spf)) + s->gap + fft_size + 64;
	s->st.assign(n_streams, SsState());
	return s;
}

void wc_synth_stream_destroy(wc_synth_stream *s) {
	if (!s) return;
	s->dev->quiesce();
	for (int k = 0; k < 2; ++k) { s->wf0[k].release(); s->wsp[k].release(); s->wap[k].release(); s->carry[k].release(); }
	s->dsp.release(); s->dap.release(); s->dmod.release(); s->sf0.release(); s->h_mod.release();
	s->cf0.release(); s->csp.release(); s->cap.release(); s->rf0.release(); s->rsp.release(); s->rap.release(); s->drt.release(); s->h_rt.release();
	s->tf0.release(); s->tcsp.release(); s->tcap.release();
	s->work.release(); s->inc.release(); s->pulses.release(); s->resp.release(); s->meta.release(); s->owner.release(); s->aux.release(); s->cls.release(); s->h_stage.release();
	wc_synthesis_destroy(s->sy);
	delete s;
}

int wc_synth_stream_max_samples_per_push(const wc_synth_stream *s) { return s ? s->wsz : WC_ERR_INVALID; }

int wc_synth_stream_reset(wc_synth_stream *s, int u) {
	if (!s || u < 0 || u >= s->n_streams) return fail(WC_ERR_INVALID, "synthesis stream: bad stream index");
	DeviceLock lock(s->dev);
	s->st[u] = SsState();
	return WC_OK;
}

unsigned long long wc_synth_stream_rng_position(const wc_synth_stream *s, int u) {
	return (s && u >= 0 && u < s->n_streams) ? s->st[u].rng_pos : 0ull;
}
int wc_synth_stream_set_rng_position(wc_synth_stream *s, int u, unsigned long long position) {
	if (!s || u < 0 || u >= s->n_streams) return fail(WC_ERR_INVALID, "synthesis stream: bad stream index");
	DeviceLock lock(s->dev);
	s->st[u].rng_pos = position;
	return WC_OK;
}
long long wc_synth_stream_frames_received(const wc_synth_stream *s, int u) {
	if (!s || u < 0 || u >= s->n_streams) return -1;
	return s->st[u].retimed ? s->st[u].src : s->st[u].frames;
}
long long wc_synth_stream_frames_synthesised(const wc_synth_stream *s, int u) { return (s && u >= 0 && u < s->n_streams) ? s->st[u].frames : -1; }
double wc_synth_stream_source_position(const wc_synth_stream *s, int u) {
	if (!s || u < 0 || u >= s->n_streams) return std::nan("");
	const SsState &q = s->st[u];
	if (q.retimed) return q.formed ? q.last : std::nan("");
	return q.frames > 0 ? (double)(q.frames - 1) : std::nan("");
}
int wc_synth_stream_set_speed(wc_synth_stream *s, int u, double speed) {
	if (!s || u < 0 || u >= s->n_streams) return fail(WC_ERR_INVALID, "synthesis stream: bad stream index");
	if (!(speed > 0.0 && speed <= DBL_MAX)) return fail(WC_ERR_INVALID, "synthesis stream: speed must be finite and positive");
	DeviceLock lock(s->dev);
	SsState &q = s->st[u];
	// one source row is carried (frame F - 1): the next position last + speed must not lie before it
	if (q.retimed && q.formed && std::floor(q.last + speed) < (double)(q.src - 1))
		return fail(WC_ERR_INVALID, "synthesis stream: speed so low that the stream's next position, last + speed, lies before its newest source frame");
	q.speed = speed;
	q.speed_set = true;
	return WC_OK;
}
int wc_synth_stream_frames_for_push(const wc_synth_stream *s, int u, int n_frames) {
	if (!s || u < 0 || u >= s->n_streams || n_frames < 0) return fail(WC_ERR_INVALID, "synthesis stream: bad stream index or frame count");
	SsState q = s->st[u];
	if (!ss_follows_map(q, n_frames)) return std::min(n_frames, s->max_frames + 1);
	if (ss_tail_missing(q)) return fail(WC_ERR_INVALID, kTailMissing);
	return ss_form(q, n_frames, s->max_frames, nullptr);
}
long long wc_synth_stream_samples_committed(const wc_synth_stream *s, int u) { return (s && u >= 0 && u < s->n_streams) ? s->st[u].samples : -1; }

int wc_synth_stream_set_modification(wc_synth_stream *s, int u, double f0_scale, double spectral_ratio) {
	if (!s || u < 0 || u >= s->n_streams) return fail(WC_ERR_INVALID, "synthesis stream: bad stream index");
	if (!(f0_scale > 0.0 && f0_scale <= DBL_MAX)) return fail(WC_ERR_INVALID, "synthesis stream: f0_scale must be finite and positive");
	if (!(spectral_ratio == 0.0 || frame_ratio_valid(spectral_ratio, s->fft_size)))
		return fail(WC_ERR_INVALID, "synthesis stream: spectral_ratio must be 0 (none) or finite and at least 2 / fft_size");
	DeviceLock lock(s->dev);
	s->st[u].mod_f0 = f0_scale;
	s->st[u].mod_ratio = spectral_ratio;
	return WC_OK;
}

}  // extern "C"

namespace {
// The argument rules of a push, of full rows or coded ones (s, n_frames and samples_out are there; the lock is held): frame counts
// in range, a flushed stream takes nothing, no null arrays.  (That a flush needs two frames is a rule on the synthesis frames,
// which a retimed push only knows after its source plan: ss_plan_core.)
int ss_check_push(const wc_synth_stream *s, const int *n_frames, const int *flush, bool arrays, const double *d_y, long long &total_in) {
	total_in = 0;
	for (int u = 0; u < s->n_streams; ++u) {
		const int nf = n_frames[u];
		if (nf < 0 || nf > s->max_frames) return fail(WC_ERR_INVALID, "synthesis stream push: n_frames out of range");
		if (s->st[u].closed && (nf > 0 || (flush && flush[u]))) return fail(WC_ERR_INVALID, "synthesis stream push: stream was flushed; wc_synth_stream_reset it first");
		total_in += nf;
	}
	if (total_in > 0 && !arrays) return fail(WC_ERR_INVALID, "synthesis stream push: null frame arrays");
	if (!d_y) return fail(WC_ERR_INVALID, "synthesis stream push: null output");
	return WC_OK;
}

// ---- the source side of a retimed push (wc_synth_stream_set_speed) ----
struct RtLink {  // where a stream's carried row comes from and where its newest source row goes, resolved once the buffers exist
	int u;
	SsPrev from;     // (None: nothing to carry)
	int keep;        // the side of the pair of carried rows its newest source row goes to, -1: no new row
	long long wrow;  // from.where == Window: the row of the window buffers
};
struct RtPlan {
	std::vector<int> cnt;  // synthesis frames per stream
	std::vector<RtStreamDesc> desc;
	std::vector<RtLink> link;
	std::vector<double> pos, scale, ratio;  // per synthesis frame
	std::vector<int> owner;                 // per synthesis frame: its stream's index in desc
	bool stretch = false;
};

// the side of the pair of carried rows that the newest source row of a push goes to: the one the stream does not hold (a stream
// that becomes retimed holds side 0, where its kept coded frame is decoded to)
int ss_pair_side(const SsPrev &p) { return p.where == SsPrev::Pair ? 1 - p.side : 1; }

// Host arithmetic of a retimed push: the synthesis frames of every stream, their positions, scales and ratios, and the rule's
// refusals.  Changes the rule's state of the streams (under the guard); enqueues and allocates nothing.
int ss_plan_source(wc_synth_stream *s, const int *n_frames, bool coded, RtPlan &pl) {
	const int n = s->n_streams;
	pl.cnt.assign(n, 0);
	size_t room = 0;  // of the per-frame vectors, so that they grow once: about nf / speed synthesis frames for a stream on its map
	for (int u = 0; u < n; ++u)
		room += (size_t)std::min<double>(s->max_frames + 1, ss_follows_map(s->st[u], n_frames[u]) ? n_frames[u] / s->st[u].speed + 1 : n_frames[u]);
	pl.pos.reserve(room); pl.scale.reserve(room); pl.ratio.reserve(room); pl.owner.reserve(room);
	pl.desc.reserve(n); pl.link.reserve(n);
	long long in_off = 0;
	for (int u = 0; u < n; ++u) {
		const int nf = n_frames[u];
		SsState &q = s->st[u];
		if (q.closed) continue;
		RtStreamDesc d;
		std::memset(&d, 0, sizeof(d));
		RtLink k{u, SsPrev(), -1, 0};
		d.out_off = (long long)pl.pos.size();
		d.in_off = in_off;
		d.n_in = nf;
		int c;
		double sc = coded ? q.mod_f0 : 1.0, rt = 0.0;
		if (ss_follows_map(q, nf)) {
			const bool was = q.retimed;
			const long long before = was ? q.src : q.F;
			if (ss_tail_missing(q)) return fail(WC_ERR_INVALID, kTailMissing);
			d.f_before = before;
			c = ss_form(q, nf, s->max_frames, &pl.pos);
			if (c > s->max_frames) return fail(WC_ERR_INVALID, "synthesis stream push: more than max_frames_per_push synthesis frames for one stream");
			if (c > 0 && std::floor(pl.pos[d.out_off]) < (double)(before - 1))
				return fail(WC_ERR_INVALID, "synthesis stream push: internal: the next position lies before the carried row");  // (wc_synth_stream_set_speed refuses such a speed)
			k.from = q.prev;
			k.wrow = (long long)u * s->wcap + (q.F - 1 - q.wbase);
			if (!was && before > 0 && (q.F - 1 < q.wbase || q.F - 1 >= q.wbase + q.wlen)) return fail(WC_ERR_INVALID, "synthesis stream push: internal window arithmetic");
			if (nf > 0) k.keep = ss_pair_side(q.prev);
			if (coded) rt = q.mod_ratio;
		} else {  // not retimed: whole positions, its ratio (coded pushes) went into the decoder
			d.f_before = q.F;
			c = nf;
			for (int i = 0; i < nf; ++i) pl.pos.push_back((double)(q.F + i));
		}
		pl.scale.insert(pl.scale.end(), c, sc);
		pl.ratio.insert(pl.ratio.end(), c, rt);
		pl.owner.insert(pl.owner.end(), c, (int)pl.desc.size());  // (c > 0: the descriptor is pushed below)
		pl.stretch = pl.stretch || (c > 0 && rt != 0.0);
		pl.cnt[u] = c;
		in_off += nf;
		if (nf > 0 || c > 0) {
			pl.desc.push_back(d);
			pl.link.push_back(k);
		}
	}
	return WC_OK;
}

// Its device half: buffers on first use, descriptors and per-frame values up through h_rt, wc::retime_stream_enqueue on the source
// rows of this push (the caller's full rows or the decoded ones) into rf0 / rsp / rap, which the core then takes.
int ss_enqueue_retimed(wc_synth_stream *s, hipStream_t hs, RtPlan &pl, const double *d_f0, const double *d_sp, const double *d_ap) {
	const int n = s->n_streams, bins = s->fft_size / 2 + 1;
	const size_t cap = (size_t)s->max_frames * n, row = sizeof(double) * (size_t)bins;
	const long long total = (long long)pl.pos.size();
	const int nd = (int)pl.desc.size();
	int rc;
	if ((rc = s->cf0.reserve(sizeof(double) * 2 * n)) || (rc = s->csp.reserve(row * 2 * n)) || (rc = s->cap.reserve(row * 2 * n)) ||
		(rc = s->rf0.reserve(sizeof(double) * cap)) || (rc = s->rsp.reserve(row * cap)) || (rc = s->rap.reserve(row * cap))) return rc;
	if (nd == 0) return WC_OK;
	const size_t bytes = sizeof(RtStreamDesc) * (size_t)nd + (3 * sizeof(double) + sizeof(int)) * (size_t)total;
	if ((rc = s->drt.reserve(sizeof(RtStreamDesc) * (size_t)n + (3 * sizeof(double) + sizeof(int)) * cap)) || (rc = s->h_rt.reserve(bytes))) return rc;
	for (int a = 0; a < nd; ++a) {
		const RtLink &k = pl.link[a];
		RtStreamDesc &d = pl.desc[a];
		if (k.from.where == SsPrev::Window) {
			d.carry_f0 = s->wf0[s->parity].as<double>() + k.wrow;
			d.carry_sp = s->wsp[s->parity].as<double>() + k.wrow * bins;
			d.carry_ap = s->wap[s->parity].as<double>() + k.wrow * bins;
		} else if (k.from.where != SsPrev::None) {
			const bool kept = k.from.where == SsPrev::Kept;
			const long long r = (long long)(kept ? 0 : k.from.side) * n + k.u;
			if (kept) {  // (once per stream and reset: the frame the decoder stretched is decoded again as it was)
				const int n_ap = GetNumberOfAperiodicities(s->fs);
				const long long t = (long long)k.from.side * n + k.u;
				WC_HIP(hipMemcpyAsync(s->cf0.as<double>() + r, s->tf0.as<double>() + t, sizeof(double), hipMemcpyDeviceToDevice, hs));
				if ((rc = decode_features_enqueue(s->dev, hs, s->fs, s->fft_size, 1, k.from.nd, s->tcsp.as<double>() + t * (s->fft_size / 2),
												  s->tcap.as<double>() + t * n_ap, nullptr, s->csp.as<double>() + r * bins,
												  s->cap.as<double>() + r * bins))) return rc;
			}
			d.carry_f0 = s->cf0.as<double>() + r;
			d.carry_sp = s->csp.as<double>() + r * bins;
			d.carry_ap = s->cap.as<double>() + r * bins;
		}
		if (k.keep >= 0) {
			const long long r = (long long)k.keep * n + k.u;
			d.keep_f0 = s->cf0.as<double>() + r;
			d.keep_sp = s->csp.as<double>() + r * bins;
			d.keep_ap = s->cap.as<double>() + r * bins;
		}
	}
	char *h = static_cast<char *>(s->h_rt.p);
	double *hv = reinterpret_cast<double *>(h + sizeof(RtStreamDesc) * (size_t)nd);
	std::memcpy(h, pl.desc.data(), sizeof(RtStreamDesc) * (size_t)nd);
	if (total > 0) {
		std::memcpy(hv, pl.pos.data(), sizeof(double) * total);
		std::memcpy(hv + total, pl.scale.data(), sizeof(double) * total);
		std::memcpy(hv + 2 * total, pl.ratio.data(), sizeof(double) * total);
		std::memcpy(hv + 3 * total, pl.owner.data(), sizeof(int) * total);
	}
	WC_HIP(hipMemcpyAsync(s->drt.p, h, bytes, hipMemcpyHostToDevice, hs));
	if ((rc = s->h_rt.mark(hs))) return rc;
	const double *dv = reinterpret_cast<const double *>(static_cast<char *>(s->drt.p) + sizeof(RtStreamDesc) * (size_t)nd);
	return retime_stream_enqueue(s->dev, hs, s->fs, s->fft_size, nd, s->drt.as<RtStreamDesc>(), reinterpret_cast<const int *>(dv + 3 * total), total, dv, dv + total,
								 pl.stretch ? dv + 2 * total : nullptr, d_f0, d_sp, d_ap, s->rf0.as<double>(), s->rsp.as<double>(),
								 s->rap.as<double>());
}

// whether a coded push keeps the newest coded frame of stream u (ss_keep_tail_kernel): not retimed, a modification setting, and
// wc_synth_stream_set_speed was called for it
bool ss_keeps_tail(const SsState &q, int nf) { return nf > 0 && !q.retimed && !q.neutral() && q.speed_set; }

// The source side of a coded push (total_in > 0 frames): the pushed frames' coded rows are decoded (wc::decode_features_enqueue)
// into dsp / dap.  Streams with a setting of wc_synth_stream_set_modification: the settings expanded per frame go up through
// h_mod, the decoder stretches with them and the push takes f0 * f0_scale out of sf0 (d_f0 then points there).  In a retimed
// push the decoder stretches the frames of the streams that are not retimed only, and scale and ratio of the others -- and every
// F0 scale -- are applied per synthesis frame by the retiming kernel.
int ss_enqueue_decode(wc_synth_stream *s, hipStream_t hs, const int *n_frames, long long total_in, bool retimed, const double *&d_f0,
					  const double *d_coded_sp, int nd, const double *d_coded_ap) {
	// what the stages in front of the push apply per source frame
	auto scale_of = [&](int u) { return retimed ? 1.0 : s->st[u].mod_f0; };
	auto ratio_of = [&](int u) { return retimed && s->st[u].retimed ? 0.0 : s->st[u].mod_ratio; };
	auto keeps_tail = [&](int u) { return ss_keeps_tail(s->st[u], n_frames[u]); };
	bool scaled = false, stretched = false, tails = false;
	for (int u = 0; u < s->n_streams; ++u)
		if (n_frames[u] > 0) {
			scaled = scaled || scale_of(u) != 1.0;
			stretched = stretched || ratio_of(u) != 0.0;
			tails = tails || keeps_tail(u);
		}
	const size_t cap = (size_t)s->max_frames * s->n_streams;
	const size_t rows = sizeof(double) * cap * (s->fft_size / 2 + 1);
	int rc;
	if ((rc = s->dsp.reserve(rows)) || (rc = s->dap.reserve(rows))) return rc;
	const double *d_ratio = nullptr;
	if (scaled || stretched || tails) {
		const int ns = s->n_streams, n_ap = GetNumberOfAperiodicities(s->fs), stride = s->fft_size / 2;
		const size_t extra = tails ? 2 * (size_t)ns : 0;  // the kept frames' indices | their rows in the pair, behind ratios | scales
		if ((rc = s->dmod.reserve(sizeof(double) * (2 * cap + extra))) || (rc = s->sf0.reserve(sizeof(double) * cap)) ||
			(rc = s->h_mod.reserve(sizeof(double) * (2 * cap + extra)))) return rc;  // (waits for the staging buffer's earlier upload)
		if (tails && ((rc = s->tf0.reserve(sizeof(double) * 2 * ns)) || (rc = s->tcsp.reserve(sizeof(double) * 2 * (size_t)ns * stride)) ||
					  (rc = s->tcap.reserve(sizeof(double) * 2 * (size_t)ns * std::max(n_ap, 1))))) return rc;
		double *h_ratio = s->h_mod.as<double>(), *h_scale = h_ratio + total_in, *h_tail = h_scale + total_in;
		if (tails)
			for (long long u = 0, o = 0; u < ns; o += n_frames[u], ++u) {
				h_tail[u] = keeps_tail((int)u) ? (double)(o + n_frames[u] - 1) : -1.0;
				h_tail[ns + u] = (double)((long long)(1 - s->st[u].prev.side) * ns + u);  // a push that fails leaves the side it holds
			}
		long long o = 0;
		for (int u = 0; u < s->n_streams; ++u)
			for (int i = 0; i < n_frames[u]; ++i, ++o) {
				h_ratio[o] = ratio_of(u);
				h_scale[o] = scale_of(u);
			}
		WC_HIP(hipMemcpyAsync(s->dmod.p, s->h_mod.p, sizeof(double) * (2 * (size_t)total_in + extra), hipMemcpyHostToDevice, hs));
		if ((rc = s->h_mod.mark(hs))) return rc;
		if (tails) {
			hipLaunchKernelGGL(ss_keep_tail_kernel, dim3(ns), dim3(64), 0, hs, (const double *)(s->dmod.as<double>() + 2 * total_in), d_f0, d_coded_sp,
							   d_coded_ap, nd, n_ap, stride, s->tf0.as<double>(), s->tcsp.as<double>(), s->tcap.as<double>());
			WC_HIP(hipGetLastError());
		}
		if (stretched) d_ratio = s->dmod.as<double>();
		if (scaled) {
			const unsigned blocks = static_cast<unsigned>(std::min<long long>((total_in + 255) / 256, 65536));
			hipLaunchKernelGGL(ss_scale_f0_kernel, dim3(blocks), dim3(256), 0, hs, d_f0, (const double *)(s->dmod.as<double>() + total_in), total_in,
							   s->sf0.as<double>());
			WC_HIP(hipGetLastError());
			d_f0 = s->sf0.as<double>();
		}
	}
	return decode_features_enqueue(s->dev, hs, s->fs, s->fft_size, total_in, nd, d_coded_sp, d_coded_ap, d_ratio, s->dsp.as<double>(),
								   s->dap.as<double>());
}

// What a push that succeeded leaves behind: where each stream that took frames now has its newest source row.  (coded_nd: the
// coefficients of a coded push, 0 for full rows.)
void ss_note_prev(wc_synth_stream *s, const int *n_frames, int coded_nd) {
	for (int u = 0; u < s->n_streams; ++u) {
		SsState &q = s->st[u];
		SsPrev &p = q.prev;
		if (n_frames[u] <= 0) continue;
		if (q.retimed) p = SsPrev{SsPrev::Pair, ss_pair_side(p), 0};
		else if (coded_nd == 0 || q.neutral()) p.where = SsPrev::Window;
		else if (ss_keeps_tail(q, n_frames[u])) p = SsPrev{SsPrev::Kept, 1 - p.side, coded_nd};
		else p.where = SsPrev::Lost;
	}
}

// ---- the core: the push on the frames the streams synthesise from ----
// The metadata block of a push of na streams, on the device (meta) and in its staging twin (h_stage): the descriptors of the first
// upload, the time base's results, and what the second upload brings when the pulses are counted.
struct SsMeta {
	SsDesc *desc;
	SsOut *out;
	OlDesc *ol;
	UttDesc *utt;
	long long *prefix, *capoff, *pairs;  // pulse prefix [na + 1] | cap_off [na] | per-stream prefix pairs [2 na]
	int *first;                          // first_index [na]
	explicit SsMeta(void *base = nullptr, int na = 0) {
		desc = static_cast<SsDesc *>(base);
		out = reinterpret_cast<SsOut *>(desc + na);
		ol = reinterpret_cast<OlDesc *>(out + na);
		utt = reinterpret_cast<UttDesc *>(ol + na);
		prefix = reinterpret_cast<long long *>(utt + na);
		capoff = prefix + na + 1;
		pairs = capoff + na;
		first = reinterpret_cast<int *>(pairs + 2 * na);
	}
	static size_t bytes(int na) {
		return (sizeof(SsDesc) + sizeof(SsOut) + sizeof(OlDesc) + sizeof(UttDesc) + 4 * sizeof(long long) + sizeof(int)) * (size_t)na + sizeof(long long) + 256;
	}
	size_t second_bytes(int na) const { return (size_t)(reinterpret_cast<char *>(first + na) - reinterpret_cast<char *>(ol)); }  // ol .. first
};

struct SsCore {
	// the plan: the streams that are open, per stream (E, outlen) the first sample that is not final and the flushed length
	std::vector<int> act, E, outlen;
	std::vector<SsDesc> desc;
	long long inc_total = 0, slots = 0;
	int max_rows = 0, max_new = 0;
	// the enqueue
	PulseBuf pb;
	SsMeta dm;
	std::vector<SsOut> tb;
	// the commit
	std::vector<OlDesc> ol;
	std::vector<UttDesc> utt;
	std::vector<long long> prefix, capoff, pairs;
	std::vector<int> first, n_syn;
	std::vector<unsigned long long> start;
	long long total_p = 0;
	int max_span = 0;
};

// Host arithmetic: the windows and the samples that become final when stream u takes cnt[u] frames (the synthesis frames of a
// retimed push), and the refusals that depend on them.  Changes the window state of the streams (under the guard).
int ss_plan_core(wc_synth_stream *s, const int *cnt, const int *flush, bool retimed, SsCore &c) {
	const int n = s->n_streams;
	const double fp_ms = s->frame_period * 1000.0;
	c.E.assign(n, 0); c.outlen.assign(n, 0);
	c.act.reserve(n); c.desc.reserve(n);
	long long in_off = 0;
	for (int u = 0; u < n; ++u) {
		SsState &q = s->st[u];
		const int nf = cnt[u];
		const bool fl = flush && flush[u];
		if (q.closed) continue;
		const int F1 = q.F + nf;
		if (fl && F1 < 2)
			return fail(WC_ERR_INVALID, retimed ? "synthesis stream push: a stream needs at least two synthesis frames (reference src/synthesis.cpp:241-242)"
												: "synthesis stream push: a stream needs at least two frames (reference src/synthesis.cpp:241-242)");
		if ((double)F1 * s->frame_period * s->fs > (double)INT_MAX - 4.0 * s->wsz)
			return fail(WC_ERR_UNSUPPORTED, "synthesis stream push: a stream may hold at most 2^31 samples (the reference's int indices)");
		// rows still needed: those of the waiting pulse and of the first sample that is not final (two rows of margin for the
		// interpolation's left neighbour and the floor of the row arithmetic)
		int need = frame_of(s, q.n_fin);
		if (q.has_pend) need = std::min(need, frame_of(s, q.pend_idx));
		int base = std::max(std::min(need - 2, q.F), q.wbase);
		base = std::max(base, 0);
		SsDesc d;
		std::memset(&d, 0, sizeof(d));
		d.win_old = (long long)u * s->wcap;
		d.win_new = (long long)u * s->wcap;
		d.in_off = in_off;
		d.keep_from = base - q.wbase;
		d.keep = q.F - base;
		d.n_in = nf;
		if (d.keep < 0 || d.keep_from < 0 || d.keep_from + d.keep > q.wlen) return fail(WC_ERR_INVALID, "synthesis stream push: internal window arithmetic");
		if (d.keep + nf > s->wcap) return fail(WC_ERR_INVALID, "synthesis stream push: frame window too small (pulse gap beyond the bound)");
		d.f_base = base;
		d.f_len = F1;
		int e;
		if (fl) {
			c.outlen[u] = wc_synthesis_out_length(F1, fp_ms, s->fs);
			e = c.outlen[u];
		} else {
			e = std::min(final_limit(s, F1), std::max(wc_synthesis_out_length(std::max(F1, 2), fp_ms, s->fs) - 1, 0));
		}
		e = std::max(e, q.n_fin);
		c.E[u] = e;
		d.n0 = q.n_fin;
		d.n1 = e;
		d.cap = (e - q.n_fin) + 2;
		d.has_pend = q.has_pend; d.pend_idx = q.pend_idx; d.pend_vuv = q.pend_vuv; d.pend_shift = q.pend_shift;
		d.run = q.run; d.wrap = q.wrap; d.vu = q.vu;
		d.inc_off = c.inc_total;
		c.inc_total += ((long long)(e - q.n_fin) + 63) / 64 * 64 + 64;
		d.slot = c.slots;
		c.slots += d.cap;
		c.max_rows = std::max(c.max_rows, d.keep + nf);
		c.max_new = std::max(c.max_new, e - q.n_fin);
		in_off += nf;
		q.wbase = base; q.wlen = d.keep + nf; q.F = F1;
		c.act.push_back(u);
		c.desc.push_back(d);
	}
	return WC_OK;
}

// Buffers, the descriptors up, frame windows, increments, time base, and the time base's results back: fails for a HIP error only.
int ss_enqueue_core(wc_synth_stream *s, hipStream_t hs, SsCore &c, const double *d_f0, const double *d_sp, const double *d_ap) {
	const int n = s->n_streams, N = s->fft_size, bins = N / 2 + 1, na = (int)c.act.size(), par = s->parity;
	int rc;
	const size_t win_rows = (size_t)n * s->wcap;
	for (int k = 0; k < 2; ++k)
		if ((rc = s->wf0[k].reserve(sizeof(double) * win_rows)) || (rc = s->wsp[k].reserve(sizeof(double) * win_rows * bins)) ||
			(rc = s->wap[k].reserve(sizeof(double) * win_rows * bins)) || (rc = s->carry[k].reserve(sizeof(double) * (size_t)n * s->ccap)))
			return rc;
	if ((rc = s->inc.reserve(sizeof(double) * (size_t)std::max<long long>(c.inc_total, 64)))) return rc;
	if ((rc = s->pulses.reserve((size_t)c.slots * (sizeof(int) * 3 + sizeof(double))))) return rc;
	c.pb.shift = s->pulses.as<double>();
	c.pb.index = reinterpret_cast<int *>(c.pb.shift + c.slots);
	c.pb.noise_size = c.pb.index + c.slots;
	c.pb.vuv = c.pb.noise_size + c.slots;
	if ((rc = s->meta.reserve(SsMeta::bytes(na))) || (rc = s->h_stage.reserve(SsMeta::bytes(na)))) return rc;
	c.dm = SsMeta(s->meta.p, na);
	std::memcpy(s->h_stage.p, c.desc.data(), sizeof(SsDesc) * na);
	WC_HIP(hipMemcpyAsync(c.dm.desc, s->h_stage.p, sizeof(SsDesc) * na, hipMemcpyHostToDevice, hs));
	if ((rc = s->h_stage.mark(hs))) return rc;
	{
		const long long per = (long long)c.max_rows * bins;
		dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(64, (per + 255) / 256)), (unsigned)na);
		hipLaunchKernelGGL(ss_frames_kernel, grid, dim3(256), 0, hs, c.dm.desc, bins, s->wf0[par].as<double>(), s->wsp[par].as<double>(),
						   s->wap[par].as<double>(), d_f0, d_sp, d_ap, s->wf0[1 - par].as<double>(), s->wsp[1 - par].as<double>(),
						   s->wap[1 - par].as<double>());
	}
	WC_HIP(hipMemsetAsync(s->inc.p, 0, sizeof(double) * (size_t)std::max<long long>(c.inc_total, 64), hs));
	if (c.max_new > 0) {
		dim3 grid((unsigned)std::min(64, (c.max_new + 255) / 256), (unsigned)na);
		hipLaunchKernelGGL(ss_increment_kernel, grid, dim3(256), 0, hs, c.dm.desc, (const double *)s->wf0[1 - par].as<double>(), s->fs, N,
						   s->frame_period, s->inc.as<double>());
	}
	hipLaunchKernelGGL(ss_timebase_kernel, dim3(na), dim3(64), 0, hs, c.dm.desc, (const double *)s->inc.as<double>(), s->fs, c.pb, c.dm.out);
	WC_HIP(hipGetLastError());
	c.tb.resize(na);
	WC_HIP(hipMemcpyAsync(c.tb.data(), c.dm.out, sizeof(SsOut) * na, hipMemcpyDeviceToHost, hs));
	WC_HIP(hipStreamSynchronize(hs));
	return WC_OK;
}

// Host arithmetic behind the read-back: which pulses are final, what is committed, the state after this push.  Its refusals
// depend on what the time base found.
int ss_commit(wc_synth_stream *s, const int *flush, SsCore &c, int *samples_out) {
	const int M = s->fft_size / 2, na = (int)c.act.size();
	c.ol.resize(na); c.utt.resize(na); c.first.resize(na); c.n_syn.resize(na); c.start.resize(na);
	c.prefix.assign(na + 1, 0); c.capoff.resize(na); c.pairs.resize(2 * na);
	long long y_total = 0;
	for (int a = 0; a < na; ++a) {
		const int u = c.act[a];
		SsState &q = s->st[u];
		const bool fl = flush && flush[u];
		const SsOut &o = c.tb[a];
		const int cnt = o.count;
		const bool pend = !fl && cnt > 0;
		c.n_syn[a] = fl ? cnt : std::max(cnt - 1, 0);
		const int e = c.E[u];
		int cut, hi;
		if (fl) {
			cut = hi = c.outlen[u];
		} else {
			// later pulses lie at or after the waiting one, or at or after the last final sample; they reach back M - 1 samples
			const int p_min = pend ? std::min(o.last_idx, e - 1) : e - 1;
			cut = std::max(q.cut, p_min - M + 1);
			hi = std::max(q.cut + q.clen, std::max(e + M - 1, cut));
		}
		if (cut < q.cut) return fail(WC_ERR_INVALID, "synthesis stream push: internal commit arithmetic");
		if (hi - q.cut > s->wsz || hi - cut > s->ccap) return fail(WC_ERR_INVALID, "synthesis stream push: carry too small (pulse gap beyond the bound)");
		OlDesc &d = c.ol[a];
		d.src_off = (long long)u * s->ccap;
		d.dst_off = (long long)u * s->ccap;
		d.y_off = y_total;
		d.slot = c.desc[a].slot;
		d.pre = c.total_p;
		d.src_len = q.clen;
		d.lo = q.cut; d.hi = hi; d.cut = cut;
		d.n_p = c.n_syn[a];
		c.max_span = std::max(c.max_span, hi - q.cut);
		UttDesc &t = c.utt[a];
		std::memset(&t, 0, sizeof(t));
		t.f_off = (long long)u * s->wcap;
		t.f_len = q.F;
		t.f_base = q.wbase;
		// (block kernels, N = 512 / 4096: absolute sample o is added at work[u * wsz + o - lo], o < hi)
		t.y_off = (long long)u * s->wsz - q.cut;
		t.y_len = hi;
		t.rng_pos = q.rng_pos;
		c.start[a] = q.rng_pos;
		c.first[a] = o.first_idx;
		c.capoff[a] = c.desc[a].slot;
		c.prefix[a] = c.total_p;
		c.pairs[2 * a] = 0; c.pairs[2 * a + 1] = c.n_syn[a];
		c.total_p += c.n_syn[a];
		samples_out[u] = cut - q.cut;
		y_total += cut - q.cut;
		// ---- state after this push ----
		q.run = o.run; q.wrap = o.wrap; q.vu = o.vu;
		q.n_fin = e;
		if (cnt > 0) {
			const unsigned long long adv = (unsigned long long)(o.last_idx - o.first_idx);  // reference :106-107: draws up to the last pulse
			q.rng_pos += adv;
		}
		q.has_pend = pend; q.pend_idx = o.last_idx; q.pend_vuv = o.last_vuv; q.pend_shift = o.last_shift;
		q.cut = cut; q.clen = hi - cut;
		q.frames = q.F;
		q.samples = cut;
		if (fl) { q.closed = true; q.has_pend = 0; q.clen = 0; }
	}
	c.prefix[na] = c.total_p;
	return WC_OK;
}

// The second upload, the responses of the final pulses, the ordered overlap-add (committed prefix out, the rest carried) and the
// synchronisation that hands samples_out and d_y back complete.
int ss_enqueue_responses(wc_synth_stream *s, hipStream_t hs, SsCore &c, double *d_y) {
	const int n = s->n_streams, N = s->fft_size, na = (int)c.act.size(), par = s->parity;
	const bool atomic = !(N == 1024 || N == 2048);
	const long long total_p = c.total_p;
	const SsMeta &dm = c.dm;
	const PulseBuf &pb = c.pb;
	int rc;
	if ((rc = s->h_stage.reserve(SsMeta::bytes(na)))) return rc;  // (waits for the staging buffer's earlier upload)
	const SsMeta hm(s->h_stage.p, na);
	std::memcpy(hm.ol, c.ol.data(), sizeof(OlDesc) * na);
	std::memcpy(hm.utt, c.utt.data(), sizeof(UttDesc) * na);
	std::memcpy(hm.prefix, c.prefix.data(), sizeof(long long) * (na + 1));
	std::memcpy(hm.capoff, c.capoff.data(), sizeof(long long) * na);
	std::memcpy(hm.pairs, c.pairs.data(), sizeof(long long) * 2 * na);
	std::memcpy(hm.first, c.first.data(), sizeof(int) * na);
	WC_HIP(hipMemcpyAsync(dm.ol, hm.ol, dm.second_bytes(na), hipMemcpyHostToDevice, hs));
	if ((rc = s->h_stage.mark(hs))) return rc;
	double *carry_old = s->carry[par].as<double>(), *carry_new = s->carry[1 - par].as<double>();
	const unsigned tiles = (unsigned)std::max(1, (c.max_span + SS_TILE - 1) / SS_TILE);
	auto overlap = [&](const double *rows, const double *src, double *dst, const OlDesc *descs) {
		switch (N) {
			case 512: hipLaunchKernelGGL(ss_overlap_kernel<512>, dim3(tiles, na), dim3(SS_T), 0, hs, descs, (const int *)pb.index, rows, src, d_y, dst); break;
			case 1024: hipLaunchKernelGGL(ss_overlap_kernel<1024>, dim3(tiles, na), dim3(SS_T), 0, hs, descs, (const int *)pb.index, rows, src, d_y, dst); break;
			case 2048: hipLaunchKernelGGL(ss_overlap_kernel<2048>, dim3(tiles, na), dim3(SS_T), 0, hs, descs, (const int *)pb.index, rows, src, d_y, dst); break;
			default: hipLaunchKernelGGL(ss_overlap_kernel<4096>, dim3(tiles, na), dim3(SS_T), 0, hs, descs, (const int *)pb.index, rows, src, d_y, dst); break;
		}
	};
	// ---- responses of the final pulses ----
	std::vector<OlDesc> ol_expand;
	if (atomic) {
		// the carried sums and zeros to the work rows, where the block kernels add the responses with FP64 atomics
		if ((rc = s->work.reserve(sizeof(double) * (size_t)n * s->wsz))) return rc;
	}
	if (total_p > 0) {
		if (!atomic && (rc = s->resp.reserve(sizeof(double) * (size_t)total_p * N))) return rc;
		SynArgs sa;
		std::memset(&sa, 0, sizeof(sa));
		sa.utts = dm.utt; sa.n_utt = na; sa.pulse_prefix = dm.prefix; sa.cap_off = dm.capoff; sa.first_index = dm.first; sa.p = pb;
		sa.f0 = s->wf0[1 - par].as<double>(); sa.sp = s->wsp[1 - par].as<double>(); sa.ap = s->wap[1 - par].as<double>();
		sa.tw = s->dev->twiddle; sa.dc_remover = syn_dc_remover(s->sy);
		sa.out = atomic ? s->work.as<double>() : nullptr;
		sa.resp = atomic ? nullptr : s->resp.as<double>();
		sa.rng_start = nullptr; sa.trace = nullptr; sa.only_pulse = -1; sa.fs = s->fs; sa.frame_period = s->frame_period;
		// pulse -> stream of the compact numbering (the one-wavefront kernels), and a per-stream copy that starts at 0
		std::vector<int> owner((size_t)total_p);
		for (int a = 0; a < na; ++a) std::fill(owner.begin() + c.prefix[a], owner.begin() + c.prefix[a + 1], a);
		DevBuf &pu = s->owner;
		if ((rc = pu.reserve(sizeof(int) * (size_t)total_p * 2))) return rc;
		WC_HIP(hipMemcpyAsync(pu.p, owner.data(), sizeof(int) * (size_t)total_p, hipMemcpyHostToDevice, hs));
		WC_HIP(hipMemsetAsync(pu.as<int>() + total_p, 0, sizeof(int) * (size_t)total_p, hs));
		WC_HIP(hipStreamSynchronize(hs));  // (owner is a host vector)
		// the class lists of the split launch (N = 2048 rows), sized for the whole push: a launch per stream uses their front
		const bool split = N == 2048 && !atomic && syn_split(s->sy);
		if (split && (rc = s->cls.reserve(sizeof(int) * syn_class_ints(total_p, na)))) return rc;
		if (atomic) {
			ol_expand = c.ol;
			for (auto &d : ol_expand) { d.dst_off = d.src_off / s->ccap * s->wsz; d.cut = d.lo; }
		}
		// the noise draws of stream a's final pulses: [start, start + (E - first_index) + 1)
		auto n_draws = [&](int a) -> uint64_t { return c.n_syn[a] == 0 ? 0 : (uint64_t)(c.E[c.act[a]] - c.first[a]) + 1; };
		DrawRange draws;
		for (int a = 0; a < na; ++a) draws.add(c.start[a], n_draws(a));
		if (atomic) {
			// expand: carried sums -> work rows (everything "carried", nothing committed)
			if ((rc = s->aux.reserve(sizeof(OlDesc) * na))) return rc;
			WC_HIP(hipMemcpyAsync(s->aux.p, ol_expand.data(), sizeof(OlDesc) * na, hipMemcpyHostToDevice, hs));
			overlap(nullptr, carry_old, s->work.as<double>(), s->aux.as<OlDesc>());
			WC_HIP(hipStreamSynchronize(hs));  // (ol_expand is a host vector)
		}
		if (draws.one_table()) {
			if ((rc = s->dev->ensure_rng(draws.lo, draws.hi))) return rc;
			sa.rng_table = s->dev->rng_table.as<uint32_t>(); sa.rng_base = s->dev->rng_base;
			sa.pulse_utt = pu.as<int>();
			sa.total_pulses = total_p;
			if (split && (rc = syn_launch_class_lists(sa, s->cls.as<int>(), nullptr, hs))) return rc;
			if ((rc = syn_launch_responses(N, sa, hs))) return rc;
		} else {
			// one launch per stream, each with its own stretch of the table
			for (int a = 0; a < na; ++a) {
				if (c.n_syn[a] == 0) continue;
				if ((rc = s->dev->ensure_rng(c.start[a], c.start[a] + n_draws(a)))) return rc;
				SynArgs one = sa;
				one.utts = dm.utt + a; one.n_utt = 1; one.pulse_prefix = dm.pairs + 2 * a; one.cap_off = dm.capoff + a; one.first_index = dm.first + a;
				one.rng_table = s->dev->rng_table.as<uint32_t>(); one.rng_base = s->dev->rng_base;
				one.pulse_utt = pu.as<int>() + total_p;
				one.resp = atomic ? nullptr : s->resp.as<double>() + c.prefix[a] * N;
				one.total_pulses = c.n_syn[a];
				if (split && (rc = syn_launch_class_lists(one, s->cls.as<int>(), nullptr, hs))) return rc;
				if ((rc = syn_launch_responses(N, one, hs))) return rc;
				WC_HIP(hipStreamSynchronize(hs));  // (the next stream's table replaces this one)
			}
		}
	}
	// ---- ordered overlap-add: committed prefix out, the rest carried ----
	if (atomic && total_p > 0) {
		std::vector<OlDesc> sp(c.ol);
		for (auto &d : sp) { d.src_off = d.src_off / s->ccap * s->wsz; d.src_len = d.hi - d.lo; d.n_p = 0; }
		if ((rc = s->h_stage.reserve(SsMeta::bytes(na)))) return rc;
		std::memcpy(s->h_stage.p, sp.data(), sizeof(OlDesc) * na);
		WC_HIP(hipMemcpyAsync(dm.ol, s->h_stage.p, sizeof(OlDesc) * na, hipMemcpyHostToDevice, hs));
		if ((rc = s->h_stage.mark(hs))) return rc;
		overlap(nullptr, s->work.as<double>(), carry_new, dm.ol);
	} else {
		overlap(atomic ? nullptr : s->resp.as<double>(), carry_old, carry_new, dm.ol);
	}
	WC_HIP(hipGetLastError());
	WC_HIP(hipStreamSynchronize(hs));
	return WC_OK;
}

// The push: the body of wc_synth_stream_push_device (full rows in d_a / d_b) and wc_synth_stream_push_coded_device (coded rows of
// nd coefficients).  Everything in front of the first ss_enqueue_* is host arithmetic: a push that is refused for its arguments or
// for the handle's state reserves and enqueues nothing.
int ss_push(wc_synth_stream *s, const int *n_frames, const int *flush, const double *d_f0, const double *d_a, const double *d_b, bool coded,
			int nd, double *d_y, int *samples_out) {
	if (!s || !n_frames || !samples_out) return fail(WC_ERR_INVALID, "synthesis stream push: null argument");
	if (const char *why = coded ? decode_features_check(s->fs, s->fft_size, nd) : nullptr) return fail(WC_ERR_INVALID, why);
	DeviceLock lock(s->dev);  // (the settings are written under it)
	const int n = s->n_streams;
	// Full rows are pushed as they are: the settings of wc_synth_stream_set_modification are applied where coded rows are decoded, so
	// a push that gives full rows to a stream with a setting is refused rather than synthesised unmodified.
	for (int u = 0; !coded && u < n; ++u)
		if (n_frames[u] > 0 && !s->st[u].neutral())
			return fail(WC_ERR_INVALID, "synthesis stream push: a stream with a modification setting takes coded frames only (wc_synth_stream_push_coded_device)");
	long long total_in;
	int rc;
	if ((rc = ss_check_push(s, n_frames, flush, d_f0 && d_a && d_b, d_y, total_in))) return rc;
	WC_HIP(hipSetDevice(s->dev->id));
	SsGuard guard(s);
	for (int u = 0; u < n; ++u) samples_out[u] = 0;
	// ---- the plans.  A push without a stream that follows a time map has no source plan: its frames are its synthesis frames ----
	const bool retimed = ss_push_is_retimed(s, n_frames);
	RtPlan pl;
	if (retimed && (rc = ss_plan_source(s, n_frames, coded, pl))) return rc;
	SsCore c;
	if ((rc = ss_plan_core(s, retimed ? pl.cnt.data() : n_frames, flush, retimed, c))) return rc;
	if (c.act.empty()) { guard.keep = true; return WC_OK; }
	// ---- the source side: decode (scale and stretch in front of it), retime ----
	hipStream_t hs = s->dev->active();
	if (coded) {
		if (total_in > 0 && (rc = ss_enqueue_decode(s, hs, n_frames, total_in, retimed, d_f0, d_a, nd, d_b))) return rc;
		d_a = s->dsp.as<double>(); d_b = s->dap.as<double>();
	}
	if (retimed) {
		if ((rc = ss_enqueue_retimed(s, hs, pl, d_f0, d_a, d_b))) return rc;
		d_f0 = s->rf0.as<double>(); d_a = s->rsp.as<double>(); d_b = s->rap.as<double>();
	}
	// ---- the core ----
	if ((rc = ss_enqueue_core(s, hs, c, d_f0, d_a, d_b)) || (rc = ss_commit(s, flush, c, samples_out)) || (rc = ss_enqueue_responses(s, hs, c, d_y))) return rc;
	ss_note_prev(s, n_frames, coded ? nd : 0);
	s->parity = 1 - s->parity;
	guard.keep = true;
	return WC_OK;
}
}  // namespace

extern "C" {

// Streams with a speed (wc_synth_stream_set_speed): the rows are retimed without scale or ratio and the push runs on the retimed rows.
int wc_synth_stream_push_device(wc_synth_stream *s, const int *n_frames, const int *flush, const double *d_f0, const double *d_sp,
								const double *d_ap, double *d_y, int *samples_out) {
	return ss_push(s, n_frames, flush, d_f0, d_sp, d_ap, false, 0, d_y, samples_out);
}

int wc_synth_stream_push_coded_device(wc_synth_stream *s, const int *n_frames, const int *flush, const double *d_f0,
									  const double *d_coded_sp, int number_of_dimensions, const double *d_coded_ap, double *d_y,
									  int *samples_out) {
	return ss_push(s, n_frames, flush, d_f0, d_coded_sp, d_coded_ap, true, number_of_dimensions, d_y, samples_out);
}

}  // extern "C"
