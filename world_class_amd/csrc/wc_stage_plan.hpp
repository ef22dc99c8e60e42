// The host half that the stage handles share, as plain C++ with no HIP in it (a host compiler takes this header alone:
// tests/cpp/stage_plan_check.cpp): the utterance descriptor the kernels read, the layout of a batch in the packed arrays, the
// noise draws a stage can make per utterance, and the range of stream positions a call asks Device::ensure_rng for.
#pragma once
#include <cstddef>
#include <cstdint>

namespace wc {

// utterance descriptors uploaded per batch call
struct UttDesc {
	long long x_off;   // first sample in the packed sample array
	long long f_off;   // first frame (row) in the packed frame arrays
	long long y_off;   // first output sample (synthesis)
	int x_len, f_len, y_len;
	int f_base;        // absolute frame held in row f_off (synthesis streams; 0 for batch calls): frame k is row f_off + k - f_base
	unsigned long long rng_pos;  // stream position at which this utterance starts the stage
};
// (the kernels read the records as the host wrote them: the device's view must not move)
static_assert(sizeof(UttDesc) == 48 && offsetof(UttDesc, x_len) == 24 && offsetof(UttDesc, rng_pos) == 40, "UttDesc is read on the device");

// The layout of a batch: utterance u's samples, frames and output samples lie behind those of the utterances before it.  A length
// array a stage has none of is nullptr (offsets and lengths 0), rng_pos == nullptr: every utterance starts at position 0.  The
// caller has checked the lengths; the totals come back.
struct BatchTotals {
	long long x, f, y;
};
inline BatchTotals batch_layout(int n_utt, const int *x_length, const int *f0_length, const int *out_length, const uint64_t *rng_pos,
								UttDesc *utts) {
	BatchTotals t = {0, 0, 0};
	for (int u = 0; u < n_utt; ++u) {
		UttDesc &d = utts[u];
		d.x_off = x_length ? t.x : 0; d.f_off = f0_length ? t.f : 0; d.y_off = out_length ? t.y : 0;
		d.x_len = x_length ? x_length[u] : 0; d.f_len = f0_length ? f0_length[u] : 0; d.y_len = out_length ? out_length[u] : 0;
		d.f_base = 0;
		d.rng_pos = rng_pos ? rng_pos[u] : 0ull;
		t.x += d.x_len; t.f += d.f_len; t.y += d.y_len;
	}
	return t;
}

// Upper bounds of the stream positions one utterance can consume in a stage (a length below 0 counts as 0).
// CheapTrick: a frame's window (at most fft_size + 1 samples) and its fft_size / 2 + 1 bins
inline uint64_t cheaptrick_draws(int fft_size, int f0_length) {
	return (uint64_t)(2 * (fft_size / 2) + 1 + fft_size / 2 + 1) * (uint64_t)(f0_length > 0 ? f0_length : 0);
}
// D4C: LoveTrain's window (1.5 periods of its 40 Hz floor either side) and the three windows of the main pass (two periods of 47 Hz)
inline uint64_t d4c_draws(int fs, int f0_length) {
	const uint64_t lt_max = (uint64_t)(2 * (int)(3.0 * fs / 40.0 / 2.0 + 1.0) + 1);
	const uint64_t main_max = 3ull * (uint64_t)(2 * (int)(4.0 * fs / 47.0 / 2.0 + 1.0) + 1);
	return (lt_max + main_max) * (uint64_t)(f0_length > 0 ? f0_length : 0);
}
// Synthesis: one draw per output sample
inline uint64_t synthesis_draws(int out_length) { return (uint64_t)(out_length > 0 ? out_length : 0); }

// The stream positions [lo, hi) of a call's draws, for Device::ensure_rng.  An utterance that draws nothing adds nothing: its
// position -- a stream reset hours after the others -- must not stretch the table.  empty(): nothing draws, no call of ensure_rng.
struct DrawRange {
	uint64_t lo = ~0ull, hi = 0;
	void add(uint64_t position, uint64_t draws) {
		if (draws == 0) return;
		lo = position < lo ? position : lo;
		hi = position + draws > hi ? position + draws : hi;
	}
	// a start position alone (the analysis streams judge the span of their streams' positions, not of the draws behind them)
	void add_start(uint64_t position) {
		lo = position < lo ? position : lo;
		hi = position > hi ? position : hi;
	}
	bool empty() const { return lo > hi; }
	// The stream handles' rule: positions within 2^28 of each other go through one batched call on one draw table; streams whose
	// noise positions lie further apart than one draw table covers (one of them was reset hours after the others started) get one
	// call per stream, each with its own stretch of the table.
	bool one_table() const { return empty() || hi - lo <= (1ull << 28); }
};

}  // namespace wc
