// Morph streams (include/world_class_stream.h: wc_morph_stream): two voices per stream arrive push by push, each consumed at its own
// speed, and every push writes the morphed frames that both voices' rows now allow as full rows -- the rows wc_synth_stream_push_device
// takes.  The streaming form of wc_morph_parameters_device (wc_morph.hip), as retime_stream_kernel is that of retime_kernel.
//
//   morph_stream_kernel<STRETCH>   one workgroup of RT_T lanes per formed frame; the frame is morph_kernel's at the same two
//     positions, weights and ratios: the same mp_f0 / mp_ap_row / mp_sp_row of wc_morph_rows.hpp on the same retimed rows.  A
//     source row of a voice is a row of this push's packed arrays or, where its index lies below the push's first frame, a row of the
//     stream's backlog: retime_stream_kernel's ki < 0 addressing with a backlog in the place of one carried row.  The host, which
//     forms the positions anyway, resolves both rows of both voices per frame (MsFrame: a row of the push, or a backlog slot), so a
//     workgroup has no descriptor to look up in front of its rows -- the reason retime_stream_kernel takes its owner array instead
//     of bisecting, carried one step further; the host-written owner of a frame leads to its stream's settings only (MsSet).  Positions lie within the rows received (p <= F - 1): no clamp, nothing not finite.
//     Workgroups behind the formed frames copy the rows each stream must keep (MsKeep) into backlog slots that no workgroup of
//     the launch reads.  STRETCH = false: no LDS; chosen by the host when no stream that forms frames in the push has a ratio.
//
//   The backlog.  Per stream and voice the rows keep .. F - 1 stay, keep = floor(last) (0 before the first frame), at most
//   max_backlog of them.  Every row that is ever kept takes the next number of a sequence per (stream, voice) and sits in slot
//   number % cap, cap = max_backlog + min(max_backlog, max_frames_per_push).  The rows a state holds carry consecutive numbers, at
//   most max_backlog of them, and a push adds at most min(max_backlog, max_frames_per_push) behind them: the new rows never land on
//   a slot the state before the push still needs.  So a push that fails on the device leaves the rows of the last good push, the
//   kept rows are never copied again, and the host state of a stream and voice is four numbers.
//
//   A push is host arithmetic (the rule, every refusal), one asynchronous copy of the frame and keep records out of page-locked
//   staging, and one launch; the coded push decodes both voices' pushed rows in front of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/world_class_stream.h"
#include "wc_morph_rows.hpp"
#include "wc_retime_rows.hpp"
#include "wc_stages.hpp"

using namespace wc;

namespace {

// A row reference: >= 0 a row of the push's packed arrays of that voice, < 0 the backlog slot ~ref (counted over the whole handle).
struct MsFrame {
	double pa, pb;
	int ia, ja, ib, jb;
	int owner, pad;  // the frame's stream: its settings, nothing its rows wait for
};
struct MsSet {  // a stream's settings at this push
	double w, wf, ra, rb;
};
struct MsKeep {
	int row, slot;  // row of the push's packed arrays -> backlog slot
	int voice, pad;
};

struct MsArgs {
	const MsSet *sets;
	const MsFrame *frames;
	const MsKeep *keeps;
	long long total_out;
	int fs, fft_size;
	const double *f0_a, *sp_a, *ap_a, *f0_b, *sp_b, *ap_b;
	double *bf0, *bsp, *bap;  // the backlog: F0 and both rows per slot
	double *f0_out, *sp_out, *ap_out;
};

__device__ __forceinline__ const double *ms_row(const double *__restrict__ in, const double *__restrict__ backlog, int ref, int width) {
	return ref >= 0 ? in + (long long)ref * width : backlog + (long long)~ref * width;
}

template <bool STRETCH>
__global__ __launch_bounds__(RT_T) void morph_stream_kernel(MsArgs A) {
	const int tid = threadIdx.x;
	const long long g = blockIdx.x;
	const int bins = A.fft_size / 2 + 1;
	if (g >= A.total_out) {  // a row of the push goes to the backlog
		const MsKeep k = A.keeps[g - A.total_out];
		const double *__restrict__ f0 = k.voice ? A.f0_b : A.f0_a, *__restrict__ sp = k.voice ? A.sp_b : A.sp_a, *__restrict__ ap = k.voice ? A.ap_b : A.ap_a;
		if (tid == 0) A.bf0[k.slot] = f0[k.row];
		const long long from = (long long)k.row * bins, to = (long long)k.slot * bins;
		rt_row(sp + from, sp + from, 1.0, 0.0, A.bsp + to, bins, tid);
		rt_row(ap + from, ap + from, 1.0, 0.0, A.bap + to, bins, tid);
		return;
	}
	const MsFrame f = A.frames[g];
	const MsSet set = A.sets[f.owner];
	// rt_place without its clamp: the host keeps 0 <= p <= F - 1
	const double aa = f.pa - floor(f.pa), ab = f.pb - floor(f.pb);
	const double wa0 = 1.0 - aa, wb0 = 1.0 - ab;

	if (tid == 0)
		A.f0_out[g] = mp_f0(rt_f0(*ms_row(A.f0_a, A.bf0, f.ia, 1), *ms_row(A.f0_a, A.bf0, f.ja, 1), wa0, aa),
							rt_f0(*ms_row(A.f0_b, A.bf0, f.ib, 1), *ms_row(A.f0_b, A.bf0, f.jb, 1), wb0, ab), set.wf);
	const MpRow pa{ms_row(A.ap_a, A.bap, f.ia, bins), ms_row(A.ap_a, A.bap, f.ja, bins), wa0, aa};
	const MpRow pb{ms_row(A.ap_b, A.bap, f.ib, bins), ms_row(A.ap_b, A.bap, f.jb, bins), wb0, ab};
	mp_ap_row(pa, pb, set.w, A.ap_out + g * bins, bins, tid);
	const MpRow sa{ms_row(A.sp_a, A.bsp, f.ia, bins), ms_row(A.sp_a, A.bsp, f.ja, bins), wa0, aa};
	const MpRow sb{ms_row(A.sp_b, A.bsp, f.ib, bins), ms_row(A.sp_b, A.bsp, f.jb, bins), wb0, ab};
	// (the ratios are 0 or valid: the setter refuses the others)
	mp_sp_row<STRETCH>(sa, sb, set.w, set.ra, set.rb, A.sp_out + g * bins, A.fs, A.fft_size, tid);
}

// ---- the host half: the rule of the header ----
struct MsVoice {
	long long F = 0;     // source frames received
	long long seq = 0;   // sequence number of row keep(): row r >= keep sits in slot (seq + r - keep) % cap
	double last = 0.0;   // position of the newest formed frame (while formed)
	double speed = 1.0, ratio = 0.0;
};
struct MsState {
	MsVoice v[2];
	bool formed = false;
	double w = 0.0, wf = 0.0;
	long long frames = 0;  // frames formed
	long long keep(int x) const { return formed ? (long long)std::floor(v[x].last) : 0; }
};

// The stream takes n_a / n_b source frames and forms its frames: p = last + speed per voice (0.0 for the first) while both
// p <= F - 1.  Returns their number, the positions appended to pos (pa, pb per frame), or limit + 1 as soon as there would be more
// than limit (q is then half way: callers work on a copy).
int ms_form(MsState &q, int n_a, int n_b, int limit, std::vector<double> *pos) {
	q.v[0].F += n_a;
	q.v[1].F += n_b;
	int c = 0;
	for (;;) {
		const double pa = q.formed ? q.v[0].last + q.v[0].speed : 0.0;
		const double pb = q.formed ? q.v[1].last + q.v[1].speed : 0.0;
		if (!(pa <= (double)(q.v[0].F - 1) && pb <= (double)(q.v[1].F - 1))) return c;
		if (c == limit) return limit + 1;
		if (pos) { pos->push_back(pa); pos->push_back(pb); }
		q.v[0].last = pa;
		q.v[1].last = pb;
		q.formed = true;
		++q.frames;
		++c;
	}
}

}  // namespace

struct wc_morph_stream {
	int fs, fft_size, n_streams, max_frames, max_backlog, cap;  // cap: backlog slots per stream and voice
	Device *dev;
	std::vector<MsState> st, next;  // next: the states a push plans, kept if it succeeds
	std::vector<double> pos;
	std::vector<int> cnt;
	DevBuf bf0, bsp, bap;    // the backlog: 2 voices x n_streams x cap slots
	RecPair rec;             // the frame and keep records of a push
	DevBuf dsp[2], dap[2];   // wc_morph_stream_push_coded_device: the pushed frames' decoded rows per voice (on first use)
	size_t frames_cap() const { return (size_t)n_streams * max_frames; }
	size_t keeps_cap() const { return (size_t)2 * n_streams * std::min(max_backlog, max_frames); }
	// the records of a push, in the staging and on the device: the settings of every stream | the frames | the rows to keep
	size_t rec_bytes() const { return sizeof(MsSet) * n_streams + sizeof(MsFrame) * frames_cap() + sizeof(MsKeep) * keeps_cap(); }
};

namespace {

bool ms_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

int ms_push(wc_morph_stream *m, const int *n_a, const double *d_f0_a, const double *d_a_a, const double *d_b_a, const int *n_b,
			const double *d_f0_b, const double *d_a_b, const double *d_b_b, bool coded, int nd, double *d_f0_out, double *d_sp_out,
			double *d_ap_out, int *frames_out) {
	if (!m || !n_a || !n_b || !frames_out) return fail(WC_ERR_INVALID, "morph stream push: null argument");
	if (const char *why = coded ? decode_features_check(m->fs, m->fft_size, nd) : nullptr) return fail(WC_ERR_INVALID, why);
	DeviceLock lock(m->dev);  // (the settings are written under it)
	const int n = m->n_streams;
	long long in[2] = {0, 0};
	for (int u = 0; u < n; ++u) {
		if (n_a[u] < 0 || n_b[u] < 0) return fail(WC_ERR_INVALID, "morph stream push: negative frame count");
		if (n_a[u] > m->max_frames || n_b[u] > m->max_frames) return fail(WC_ERR_INVALID, "morph stream push: more than max_frames_per_push frames for one stream");
		in[0] += n_a[u];
		in[1] += n_b[u];
	}
	if ((in[0] > 0 && !(d_f0_a && d_a_a && d_b_a)) || (in[1] > 0 && !(d_f0_b && d_a_b && d_b_b)))
		return fail(WC_ERR_INVALID, "morph stream push: null input array");
	// ---- the plan: host arithmetic on a copy of the states, every refusal in front of the first enqueue ----
	MsSet *set = m->rec.begin<MsSet>();
	if (!set) return WC_ERR_DEVICE;
	MsFrame *fr = reinterpret_cast<MsFrame *>(set + n);
	MsKeep *kp = reinterpret_cast<MsKeep *>(fr + m->frames_cap());  // (moved up behind the frames once their number is known)
	m->next = m->st;
	long long total_out = 0, n_keep = 0, off[2] = {0, 0};
	bool stretch = false;
	for (int u = 0; u < n; ++u) {
		const MsState &old = m->st[u];
		MsState &q = m->next[u];
		const int cnt[2] = {n_a[u], n_b[u]};
		m->pos.clear();
		const int c = ms_form(q, cnt[0], cnt[1], m->max_frames, &m->pos);
		if (c > m->max_frames) return fail(WC_ERR_INVALID, "morph stream push: more than max_frames_per_push frames formed for one stream");
		long long base[2], keep_old[2], slot_old[2];  // first slot of the stream's voice; the first row the old state holds and its slot
		for (int x = 0; x < 2; ++x) {
			if (q.v[x].F - q.keep(x) > m->max_backlog)
				return fail(WC_ERR_INVALID, "morph stream push: a voice would keep more than max_backlog rows (the other voice is behind)");
			base[x] = ((long long)x * n + u) * m->cap;
			keep_old[x] = old.keep(x);
			slot_old[x] = old.v[x].seq % m->cap;
		}
		// source row r of voice x: a row of this push, or the backlog slot the state before the push holds it in
		auto ref = [&](int x, long long r) -> int {
			const MsVoice &o = old.v[x];
			if (r >= o.F) return (int)(off[x] + (r - o.F));
			const long long s = slot_old[x] + (r - keep_old[x]);  // (r - keep_old < max_backlog <= cap)
			return ~(int)(base[x] + (s >= m->cap ? s - m->cap : s));
		};
		set[u].w = q.w; set[u].wf = q.wf; set[u].ra = q.v[0].ratio; set[u].rb = q.v[1].ratio;
		for (int k = 0; k < c; ++k) {
			MsFrame &f = fr[total_out + k];
			f.pa = m->pos[2 * k]; f.pb = m->pos[2 * k + 1];
			const long long ia = (long long)std::floor(f.pa), ib = (long long)std::floor(f.pb);
			f.ia = ref(0, ia); f.ja = f.pa - ia > 0.0 ? ref(0, ia + 1) : f.ia;
			f.ib = ref(1, ib); f.jb = f.pb - ib > 0.0 ? ref(1, ib + 1) : f.ib;
			f.owner = u; f.pad = 0;
		}
		if (c > 0 && (q.v[0].ratio != 0.0 || q.v[1].ratio != 0.0)) stretch = true;
		for (int x = 0; x < 2; ++x) {
			const MsVoice &o = old.v[x];
			MsVoice &v = q.v[x];
			const long long keep_new = q.keep(x), fresh = o.seq + (o.F - keep_old[x]);  // fresh: the next unused number
			v.seq = keep_new < o.F ? o.seq + (keep_new - keep_old[x]) : fresh;
			for (long long r = std::max(keep_new, o.F); r < v.F; ++r) {
				MsKeep &k = kp[n_keep++];
				k.row = (int)(off[x] + (r - o.F));
				k.slot = (int)(base[x] + (v.seq + (r - keep_new)) % m->cap);
				k.voice = x; k.pad = 0;
			}
			off[x] += cnt[x];
		}
		m->cnt[u] = c;
		total_out += c;
	}
	if (total_out > 0 && !(d_f0_out && d_sp_out && d_ap_out)) return fail(WC_ERR_INVALID, "morph stream push: null output array");
	std::copy(m->cnt.begin(), m->cnt.end(), frames_out);  // (no refusal is left)
	if (total_out + n_keep == 0) { m->st.swap(m->next); return WC_OK; }
	// ---- enqueue: decode (coded pushes), the records, the launch ----
	WC_HIP(hipSetDevice(m->dev->id));
	hipStream_t hs = m->dev->active();
	int rc;
	if (coded) {
		const size_t row_bytes = sizeof(double) * (m->fft_size / 2 + 1) * m->frames_cap();
		const double *csp[2] = {d_a_a, d_a_b}, *cap[2] = {d_b_a, d_b_b};
		for (int x = 0; x < 2; ++x) {
			if (in[x] == 0) continue;
			if ((rc = m->dsp[x].reserve(row_bytes)) || (rc = m->dap[x].reserve(row_bytes))) return rc;
			if ((rc = decode_features_enqueue(m->dev, hs, m->fs, m->fft_size, in[x], nd, csp[x], cap[x], nullptr, m->dsp[x].as<double>(), m->dap[x].as<double>())))
				return rc;
		}
		d_a_a = m->dsp[0].as<double>(); d_b_a = m->dap[0].as<double>();
		d_a_b = m->dsp[1].as<double>(); d_b_b = m->dap[1].as<double>();
	}
	// the keep records follow the frame records of this push in the staging and on the device
	std::memmove(fr + total_out, kp, sizeof(MsKeep) * (size_t)n_keep);
	const size_t bytes = sizeof(MsSet) * (size_t)n + sizeof(MsFrame) * (size_t)total_out + sizeof(MsKeep) * (size_t)n_keep;
	MsArgs a;
	if ((rc = m->rec.upload(hs, bytes, &a.sets))) return rc;
	a.frames = reinterpret_cast<const MsFrame *>(a.sets + n);
	a.keeps = reinterpret_cast<const MsKeep *>(a.frames + total_out);
	a.total_out = total_out; a.fs = m->fs; a.fft_size = m->fft_size;
	a.f0_a = d_f0_a; a.sp_a = d_a_a; a.ap_a = d_b_a; a.f0_b = d_f0_b; a.sp_b = d_a_b; a.ap_b = d_b_b;
	a.bf0 = m->bf0.as<double>(); a.bsp = m->bsp.as<double>(); a.bap = m->bap.as<double>();
	a.f0_out = d_f0_out; a.sp_out = d_sp_out; a.ap_out = d_ap_out;
	if ((rc = m->dev->time_begin("morph_stream_kernel", hs))) return rc;
	const dim3 grid((unsigned)(total_out + n_keep));
	if (stretch) hipLaunchKernelGGL(morph_stream_kernel<true>, grid, dim3(RT_T), 0, hs, a);
	else hipLaunchKernelGGL(morph_stream_kernel<false>, grid, dim3(RT_T), 0, hs, a);
	WC_HIP(hipGetLastError());
	if ((rc = m->dev->time_end("morph_stream_kernel", hs))) return rc;
	m->st.swap(m->next);
	return WC_OK;
}

bool ms_index_ok(const wc_morph_stream *m, int u) { return m && u >= 0 && u < m->n_streams; }

}  // namespace

extern "C" {

wc_morph_stream *wc_morph_stream_create(int fs, int fft_size, int n_streams, int max_frames_per_push, int max_backlog) {
	if (!fft_size_supported(fft_size)) { set_error("morph stream: fft_size must be 512, 1024, 2048 or 4096"); return nullptr; }
	if (fs <= 0) { set_error("morph stream: fs must be positive"); return nullptr; }
	if (n_streams <= 0 || max_frames_per_push <= 0) { set_error("morph stream: n_streams and max_frames_per_push must be positive"); return nullptr; }
	if (max_backlog < 2) { set_error("morph stream: max_backlog must be at least 2"); return nullptr; }
	if ((long long)n_streams * max_frames_per_push > 0x7fffffffll || (long long)n_streams * max_backlog > 0x0fffffffll) {
		set_error("morph stream: n_streams x max_frames_per_push or n_streams x max_backlog too large");
		return nullptr;
	}
	Device *dev = current_device();
	if (!dev) return nullptr;
	DeviceLock lock(dev);
	wc_morph_stream *m = new wc_morph_stream();
	m->fs = fs; m->fft_size = fft_size; m->n_streams = n_streams; m->max_frames = max_frames_per_push; m->max_backlog = max_backlog;
	m->cap = max_backlog + std::min(max_backlog, max_frames_per_push);
	m->dev = dev;
	m->st.assign(n_streams, MsState());
	m->next.reserve(n_streams);
	m->cnt.assign(n_streams, 0);
	m->pos.reserve(2 * (size_t)max_frames_per_push + 2);
	const size_t slots = (size_t)2 * n_streams * m->cap, bins = fft_size / 2 + 1;
	const size_t rec = m->rec_bytes();
	if (m->bf0.reserve(sizeof(double) * slots) || m->bsp.reserve(sizeof(double) * slots * bins) || m->bap.reserve(sizeof(double) * slots * bins) ||
		m->rec.reserve(rec)) {
		wc_morph_stream_destroy(m);
		return nullptr;
	}
	return m;
}

void wc_morph_stream_destroy(wc_morph_stream *m) {
	if (!m) return;
	m->dev->quiesce();
	m->bf0.release(); m->bsp.release(); m->bap.release(); m->rec.release();
	for (int x = 0; x < 2; ++x) { m->dsp[x].release(); m->dap[x].release(); }
	delete m;
}

int wc_morph_stream_reset(wc_morph_stream *m, int u) {
	if (!ms_index_ok(m, u)) return fail(WC_ERR_INVALID, "morph stream: bad stream index");
	DeviceLock lock(m->dev);
	m->st[u] = MsState();
	return WC_OK;
}

int wc_morph_stream_set_speeds(wc_morph_stream *m, int u, double speed_a, double speed_b) {
	if (!ms_index_ok(m, u)) return fail(WC_ERR_INVALID, "morph stream: bad stream index");
	if (!(ms_finite(speed_a) && speed_a > 0.0 && ms_finite(speed_b) && speed_b > 0.0))
		return fail(WC_ERR_INVALID, "morph stream: a speed must be finite and > 0");
	DeviceLock lock(m->dev);
	m->st[u].v[0].speed = speed_a;
	m->st[u].v[1].speed = speed_b;
	return WC_OK;
}

int wc_morph_stream_set_weight(wc_morph_stream *m, int u, double weight, double f0_weight) {
	if (!ms_index_ok(m, u)) return fail(WC_ERR_INVALID, "morph stream: bad stream index");
	if (!(ms_finite(weight) && ms_finite(f0_weight))) return fail(WC_ERR_INVALID, "morph stream: the weight and the F0 weight must be finite");
	DeviceLock lock(m->dev);
	m->st[u].w = weight;
	m->st[u].wf = f0_weight;
	return WC_OK;
}

int wc_morph_stream_set_ratios(wc_morph_stream *m, int u, double ratio_a, double ratio_b) {
	if (!ms_index_ok(m, u)) return fail(WC_ERR_INVALID, "morph stream: bad stream index");
	if (!((ratio_a == 0.0 || frame_ratio_valid(ratio_a, m->fft_size)) && (ratio_b == 0.0 || frame_ratio_valid(ratio_b, m->fft_size))))
		return fail(WC_ERR_INVALID, "morph stream: a ratio must be 0 (none) or finite and >= 2.0 / fft_size");
	DeviceLock lock(m->dev);
	m->st[u].v[0].ratio = ratio_a;
	m->st[u].v[1].ratio = ratio_b;
	return WC_OK;
}

int wc_morph_stream_frames_for_push(const wc_morph_stream *m, int u, int n_a, int n_b) {
	if (!ms_index_ok(m, u)) return fail(WC_ERR_INVALID, "morph stream: bad stream index");
	if (n_a < 0 || n_b < 0) return fail(WC_ERR_INVALID, "morph stream: negative frame count");
	DeviceLock lock(m->dev);
	MsState q = m->st[u];
	return ms_form(q, n_a, n_b, m->max_frames, nullptr);
}

int wc_morph_stream_push_device(wc_morph_stream *m, const int *n_a, const double *d_f0_a, const double *d_sp_a, const double *d_ap_a,
								const int *n_b, const double *d_f0_b, const double *d_sp_b, const double *d_ap_b, double *d_f0_out,
								double *d_sp_out, double *d_ap_out, int *frames_out) {
	return ms_push(m, n_a, d_f0_a, d_sp_a, d_ap_a, n_b, d_f0_b, d_sp_b, d_ap_b, false, 0, d_f0_out, d_sp_out, d_ap_out, frames_out);
}

int wc_morph_stream_push_coded_device(wc_morph_stream *m, const int *n_a, const double *d_f0_a, const double *d_coded_sp_a,
									  const double *d_coded_ap_a, const int *n_b, const double *d_f0_b, const double *d_coded_sp_b,
									  const double *d_coded_ap_b, int number_of_dimensions, double *d_f0_out, double *d_sp_out,
									  double *d_ap_out, int *frames_out) {
	return ms_push(m, n_a, d_f0_a, d_coded_sp_a, d_coded_ap_a, n_b, d_f0_b, d_coded_sp_b, d_coded_ap_b, true, number_of_dimensions, d_f0_out,
				   d_sp_out, d_ap_out, frames_out);
}

double wc_morph_stream_source_position(const wc_morph_stream *m, int u, int source) {
	if (!ms_index_ok(m, u) || source < 0 || source > 1 || !m->st[u].formed) return std::nan("");
	return m->st[u].v[source].last;
}

long long wc_morph_stream_frames_received(const wc_morph_stream *m, int u, int source) {
	if (!ms_index_ok(m, u) || source < 0 || source > 1) return -1;
	return m->st[u].v[source].F;
}

int wc_morph_stream_backlog(const wc_morph_stream *m, int u, int source) {
	if (!ms_index_ok(m, u) || source < 0 || source > 1) return WC_ERR_INVALID;
	return (int)(m->st[u].v[source].F - m->st[u].keep(source));
}

long long wc_morph_stream_frames_formed(const wc_morph_stream *m, int u) {
	if (!ms_index_ok(m, u)) return -1;
	return m->st[u].frames;
}

}  // extern "C"
