// Device-side pieces of the Synthesis stage shared by the batch kernels (wc_synthesis.hip) and the concurrent-stream
// synthesis (wc_synth_stream.hip): the pulse list, the coarse F0 / VUV contour, the sequential phase chain and the arguments
// of the per-pulse response kernels.
#pragma once
#include <cstdint>

#include "wc_device.hpp"
#include "wc_internal.hpp"

namespace wc {

struct PulseBuf {
	int *index;       // sample index of the pulse
	double *shift;    // fractional time shift (s)
	int *noise_size;  // samples to the next pulse (0 for the last pulse)
	int *vuv;         // interpolated VUV at the pulse
};

// interp1 of a coarse contour given on the uniform axis j * fp (j = 0 .. L) at time t, with the
// reference's histc semantics (reference src/world_matlabfunctions.cpp:136-182): k = clamp(#{j : j fp <= t}, 1, L)
struct Coarse {
	const double *f0;
	int L;
	double lowest_f0, fp;
	int base = 0;  // absolute frame held in f0[0] (synthesis streams: a window of the frames)
	__device__ __forceinline__ double cf_in(int j) const {  // reference :232-236
		double v = f0[j - base];
		return (v < lowest_f0) ? 0.0 : v;
	}
	__device__ __forceinline__ double cv_in(int j) const { return (cf_in(j) == 0.0) ? 0.0 : 1.0; }
	// one extrapolated point at j == L (reference :239-242)
	__device__ __forceinline__ double cf(int j) const { return j < L ? cf_in(j) : cf_in(L - 1) * 2 - cf_in(L - 2); }
	__device__ __forceinline__ double cv(int j) const { return j < L ? cv_in(j) : cv_in(L - 1) * 2 - cv_in(L - 2); }
	__device__ __forceinline__ void at(double t, double &f, double &v) const {
		int j = (int)(t / fp);
		j = max(0, min(j, L));
		while (j < L && t >= (j + 1) * fp) ++j;
		while (j > 0 && t < j * fp) --j;
		int k = min(max(j + 1, 1), L);
		double x0 = (k - 1) * fp, x1 = k * fp;
		double s = (t - x0) / (x1 - x0);
		double f_a = cf(k - 1), f_b = cf(k), v_a = cv(k - 1), v_b = cv(k);
		f = f_a + s * (f_b - f_a);
		v = v_a + s * (v_b - v_a);
	}
};

// 64 steps of the sequential phase sum, entirely in one asm block: lane L ends with run + |p[0]| + ... + |p[L]|
// added in exactly that order.  The increments are fetched with scalar loads (8 doubles per s_load_dwordx16)
// into two register tuples that are refilled while the other one is being consumed (SMEM returns out of
// order, so the only legal wait is lgkmcnt(0): wait, issue the next load, then run the 8 dependent adds).
// The set of participating lanes shrinks by shifting EXEC, so each step is one dependent v_add_f64.
// (the two tuples are the fixed registers s[40:55] and s[56:71], declared as clobbers)
__device__ __forceinline__ void chain64(double &mine, const double *__restrict__ p) {
	unsigned long long save;
	asm volatile(
		"s_mov_b64 %[sv], exec\n\t"
		"s_load_dwordx16 s[40:55], %[p], 0x0\n\t"
		"s_waitcnt lgkmcnt(0)\n\t"
		"s_load_dwordx16 s[56:71], %[p], 0x40\n\t"
		"v_add_f64 %[m], %[m], |s[40:41]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[42:43]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[44:45]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[46:47]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[48:49]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[50:51]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[52:53]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[54:55]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"s_waitcnt lgkmcnt(0)\n\t"
		"s_load_dwordx16 s[40:55], %[p], 0x80\n\t"
		"v_add_f64 %[m], %[m], |s[56:57]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[58:59]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[60:61]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[62:63]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[64:65]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[66:67]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[68:69]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[70:71]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"s_waitcnt lgkmcnt(0)\n\t"
		"s_load_dwordx16 s[56:71], %[p], 0xc0\n\t"
		"v_add_f64 %[m], %[m], |s[40:41]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[42:43]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[44:45]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[46:47]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[48:49]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[50:51]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[52:53]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[54:55]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"s_waitcnt lgkmcnt(0)\n\t"
		"s_load_dwordx16 s[40:55], %[p], 0x100\n\t"
		"v_add_f64 %[m], %[m], |s[56:57]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[58:59]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[60:61]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[62:63]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[64:65]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[66:67]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[68:69]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[70:71]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"s_waitcnt lgkmcnt(0)\n\t"
		"s_load_dwordx16 s[56:71], %[p], 0x140\n\t"
		"v_add_f64 %[m], %[m], |s[40:41]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[42:43]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[44:45]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[46:47]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[48:49]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[50:51]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[52:53]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[54:55]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"s_waitcnt lgkmcnt(0)\n\t"
		"s_load_dwordx16 s[40:55], %[p], 0x180\n\t"
		"v_add_f64 %[m], %[m], |s[56:57]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[58:59]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[60:61]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[62:63]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[64:65]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[66:67]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[68:69]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[70:71]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"s_waitcnt lgkmcnt(0)\n\t"
		"s_load_dwordx16 s[56:71], %[p], 0x1c0\n\t"
		"v_add_f64 %[m], %[m], |s[40:41]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[42:43]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[44:45]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[46:47]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[48:49]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[50:51]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[52:53]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[54:55]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"s_waitcnt lgkmcnt(0)\n\t"
		"v_add_f64 %[m], %[m], |s[56:57]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[58:59]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[60:61]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[62:63]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[64:65]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[66:67]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[68:69]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"v_add_f64 %[m], %[m], |s[70:71]|\n\t s_lshl_b64 exec, exec, 1\n\t"
		"s_mov_b64 exec, %[sv]\n\t"
		: [m] "+v"(mine), [sv] "=&s"(save)
		: [p] "s"(p)
		: "scc", "memory", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53",
		  "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70",
		  "s71");
}

struct SynArgs {
	const UttDesc *utts;
	int n_utt;
	const long long *pulse_prefix;  // exclusive prefix of the per-utterance pulse counts (n_utt + 1)
	const long long *cap_off;
	const int *first_index;
	PulseBuf p;
	const double *f0, *sp, *ap;
	const uint32_t *rng_table;
	unsigned long long rng_base;
	const double2 *tw;
	const double *dc_remover;
	double *out;
	const int *pulse_utt;  // the one-wavefront kernel: utterance of every pulse of the compact numbering (syn_pulse_utt_kernel)
	// the split launch of the N = 2048 kernel (syn_launch_class_lists; NULL: one launch over all pulses): the compact numbers of the
	// voiced pulses at cls_list[0 ..), of the unvoiced ones at cls_list[total_pulses ..), each in pulse order; cls_count[2]
	const int *cls_list, *cls_count;
	double *resp;  // the one-wavefront kernel: [pulse][N] responses in output order, summed by syn_overlap_add_kernel (NULL: atomics into out)
	long long total_pulses;  // launch size (capacity); the real count is pulse_prefix[n_utt]
	const unsigned long long *rng_start;  // per-utterance stream position (device), NULL = utts[u].rng_pos
	unsigned long long *trace;  // WC_SYN_TRACE builds: 16 shader-clock stamps per pulse
	long long only_pulse;  // debugging aid (builds with -DWC_DEBUG_HOOKS, env WC_DEBUG_ONLY_PULSE): synthesise only this pulse, -1 = all
	int fs;
	double frame_period;
};

// The per-pulse response kernels of wc_synthesis.hip for a pulse list that is already complete (index, shift, noise_size, vuv,
// pulse_prefix, first_index): N = 1024 / 2048 write a response row per pulse to a.resp (a.pulse_utt filled), which the caller
// sums in pulse order; N = 512 / 4096 add into a.out + utts[u].y_off with FP64 atomics (samples 0 <= o < y_len).
// (N = 2048 with a.cls_list set: one launch per class, voiced first)
int syn_launch_responses(int fft_size, const SynArgs &a, hipStream_t s);
// The class lists of a complete pulse list, on the device (enqueue only): fills buf (syn_class_ints(a.total_pulses, a.n_utt) ints)
// and points a.cls_list / a.cls_count into it; pulse_utt != NULL: filled as well (what syn_pulse_utt_kernel does).
size_t syn_class_ints(long long total_pulses, int n_utt);
int syn_launch_class_lists(SynArgs &a, int *buf, int *pulse_utt, hipStream_t s);

}  // namespace wc
