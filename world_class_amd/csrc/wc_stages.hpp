// Enqueue-only entry points of the four stages (no host synchronisation), used by the fused pipeline
// (wc_pipeline.hip).  Each is defined next to its stage's kernels.
#pragma once
#include <utility>
#include <vector>

#include "wc_internal.hpp"
#include "wc_stretch.hpp"

// the transform sizes of CheapTrick, Synthesis, the codec and the row calls
inline bool fft_size_supported(int fft_size) { return fft_size == 512 || fft_size == 1024 || fft_size == 2048 || fft_size == 4096; }

// part: 3 = the whole chain, 1 = its front only, 2 = the tail behind a front that an earlier call with the same arguments enqueued;
// bp_done: recorded behind the band-pass; tail_after: the tail waits for it
int hv_enqueue(wc_harvest *h, hipStream_t s, int n_utt, const double *d_x, const int *x_length, double *d_tpos, double *d_f0,
			   bool full, hipEvent_t mid_event, hipEvent_t start_after, int part = 3, hipEvent_t bp_done = nullptr,
			   hipEvent_t tail_after = nullptr);
int hv_overflowed(wc_harvest *h, hipStream_t s, bool *overflow, bool *tie = nullptr, std::vector<int> *tie_utts = nullptr);
// stretches [u0, u1) of consecutive utterances out of a sorted list
std::vector<std::pair<int, int>> hv_runs_of(const std::vector<int> &us);
// the utterances whose refinement raised the tie flag are run again on this handle: the same options, band-pass as direct FIR sums
wc_harvest *hv_exact_twin(wc_harvest *h);
// Harvest in two parts (incremental streams): phases 1 = front (decimation .. refinement), 2 = tail (unreliable .. output), 3 = both
void hv_set_phases(wc_harvest *h, int mask);
int hv_row_width(const wc_harvest *h);
int hv_reserve_rows(wc_harvest *h, long long total_1ms_frames);
double *hv_candidate_rows(wc_harvest *h);
double *hv_score_rows(wc_harvest *h);

int ct_prepare(wc_cheaptrick *c, hipStream_t s, int n_utt, const int *x_length, const double *d_f0, const int *f0_length,
			   const uint64_t *rng_pos, long long *total_out);
int ct_frames(wc_cheaptrick *c, hipStream_t s, int n_utt, const double *d_x, const double *d_tpos, const double *d_f0,
			  double *d_sp, long long total, hipEvent_t *rows_done);
const unsigned long long *ct_end_positions(const wc_cheaptrick *c);

int d4c_enqueue(wc_d4c *d, hipStream_t s, int n_utt, const double *d_x, const int *x_length, const double *d_tpos,
				const double *d_f0, const int *f0_length, int fft_size, double *d_ap, const uint64_t *rng_pos,
				const unsigned long long *d_start);
const unsigned long long *d4c_end_positions(const wc_d4c *d);

int syn_prepare(wc_synthesis *sy, hipStream_t s, int n_utt, const double *d_f0, const int *f0_length, const int *out_length,
				double *d_out, const uint64_t *rng_pos, bool full);
int syn_pulses(wc_synthesis *sy, hipStream_t s, const double *d_f0, const double *d_sp, const double *d_ap, double *d_out,
			   const unsigned long long *d_start);
int syn_finish(wc_synthesis *sy, hipStream_t s, uint64_t *rng_pos_out, bool *overflow);

// the device a handle lives on (the host-pointer batch entry points stage their buffers there, not on the calling thread's device)
wc::Device *hv_device(const wc_harvest *h);
wc::Device *ct_device(const wc_cheaptrick *c);
wc::Device *d4c_device(const wc_d4c *d);
wc::Device *syn_device(const wc_synthesis *sy);
bool syn_split(const wc_synthesis *sy);  // voiced and unvoiced pulses in a launch each (N = 2048 rows; WC_SYN_SPLIT=0: off)
const double *syn_dc_remover(const wc_synthesis *sy);  // getDCRemover's table on the device (reference src/synthesis.cpp:290-303)
int syn_fs(const wc_synthesis *sy);

// The feature codec's plans (wc_codec.hip) and feature decoding for Synthesis from coded features (wc_synth_coded.hip)
namespace wc {
struct CodecPlanArgs {  // what a kernel takes: segment indices (1-based) and fractions of an interp1 between two fixed axes, DCT weights
	const int *k;
	const double *s;
	const double2 *w;
};
// One direction's plan of (device, fs, fft_size) on the device.  Coding (GetParametersForCoding, reference src/codec.cpp:125-142):
// k, s from bins 0 .. fft_size/2 (in mel) onto the fft_size/2 points of the mel axis, the DCT weights w, and at fft_size 2048 / 4096
// k, s once more in the one-wavefront coder's order (kp, sp).  Decoding (GetParametersForDecoding, :144-166): k, s from the mel axis
// onto bins 0 .. fft_size/2 and all fft_size/2 IDCT weights.
struct CodecPlan {
	DevBuf k, s, w, kp, sp;
	CodecPlanArgs args() const { return {k.as<int>(), s.as<double>(), w.as<double2>()}; }
	CodecPlanArgs wave_args() const { return {kp.as<int>(), sp.as<double>(), w.as<double2>()}; }
};
// the plan of (dev, fs, fft_size, coding), built and uploaded on first use (the only step of a codec call that allocates or waits)
// and kept for the life of the process; a failure leaves no entry behind
int codec_plan(Device *dev, int fs, int fft_size, bool coding, const CodecPlan **out);
// the codec's workgroup-per-frame kernels enqueued on st (arguments already checked)
int codec_code_sp_launch(Device *dev, hipStream_t st, int fft_size, long long n_frames, int nd, const double *d_sp, double *d_coded,
						 const CodecPlan &pl);
int codec_decode_sp_launch(Device *dev, hipStream_t st, int fft_size, long long n_frames, int nd, const double *d_coded, double *d_sp,
						   const CodecPlan &pl);
int codec_code_ap_launch(hipStream_t st, int fs, int fft_size, long long n_frames, const double *d_ap, double *d_coded);
int codec_decode_ap_launch(hipStream_t st, int fs, int fft_size, long long n_frames, const double *d_coded, double *d_ap);

// nullptr if (fs, fft_size, nd) can be decoded, else why not: fft_size 512 .. 4096, 1 <= nd <= fft_size/2, fs >= 12 kHz (at
// least one aperiodicity band)
const char *decode_features_check(int fs, int fft_size, int nd);
// Both coded rows of n_frames frames -> rows of fft_size/2+1 doubles, enqueued on s at every size (arguments already checked): the
// one-wavefront kernel at fft_size 2048, the codec's workgroup-per-frame kernels at the others, either on the cached plan.
// d_spectral_ratio (per frame, or nullptr): the rows of d_sp stretched as by modify_frames_enqueue -- inside the one-wavefront kernel
// at fft_size 2048, by that call behind the decoders at the other sizes.
int decode_features_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, long long n_frames, int nd, const double *d_coded_sp,
							const double *d_coded_ap, const double *d_spectral_ratio, double *d_sp, double *d_ap);

// Per-frame parameter modification (wc_io.hip; arguments already checked): f0[i] *= d_f0_scale[i], row i of d_sp stretched by
// d_spectral_ratio[i]; any pointer may be nullptr
int modify_frames_enqueue(hipStream_t s, int fs, int fft_size, long long n_frames, double *d_f0, double *d_sp, const double *d_f0_scale,
						  const double *d_spectral_ratio);

// Time-scale modification (wc_retime.hip).  retime_check: nullptr if wc_retime_parameters_device takes the sizes and the lengths, else
// why not; the output frames of the batch come back.  retime_enqueue: the arguments already checked, the descriptors staged and the
// kernel enqueued on s.
const char *retime_check(int fs, int fft_size, int n_utt, const int *in_length, const int *out_length, long long *total_out);
int retime_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, int n_utt, const int *in_length, const double *d_f0_in,
				   const double *d_sp_in, const double *d_ap_in, const int *out_length, const double *d_position, const double *d_f0_scale,
				   const double *d_spectral_ratio, double *d_f0_out, double *d_sp_out, double *d_ap_out, long long total_out);

// The streaming form (wc_synth_stream_set_speed): one descriptor per stream of the push, in the order of the packed arrays.  The
// synthesis frames [out_off, next out_off) of the stream sit at d_position (absolute source frames); source frame f_before + k is
// row in_off + k of the packed input, k < n_in, and source frame f_before - 1 is the carried row.  keep_*: where the newest source
// row of the push is kept for the next one, or nullptr.  The descriptors and the per-frame arrays are already on the device (the
// caller's staging), and so is d_owner, the index of its stream's descriptor per synthesis frame; one launch of total_out + n_desc
// workgroups, d_spectral_ratio == nullptr: no stretch.
struct RtStreamDesc {
	long long out_off, in_off, f_before;
	const double *carry_f0, *carry_sp, *carry_ap;
	double *keep_f0, *keep_sp, *keep_ap;
	int n_in;
};
int retime_stream_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, int n_desc, const RtStreamDesc *d_desc, const int *d_owner,
						  long long total_out, const double *d_position, const double *d_f0_scale, const double *d_spectral_ratio, const double *d_f0_in,
						  const double *d_sp_in, const double *d_ap_in, double *d_f0_out, double *d_sp_out, double *d_ap_out);

// Voice morphing (wc_morph.hip).  morph_check: nullptr if wc_morph_parameters_device takes the sizes and the lengths, else why not;
// the output frames of the batch come back.  morph_enqueue: the arguments already checked, the descriptors staged and the kernel
// enqueued on s.
const char *morph_check(int fs, int fft_size, int n_pairs, const int *a_length, const int *b_length, const int *out_length,
						long long *total_out);
int morph_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, int n_pairs, const int *a_length, const double *d_f0_a,
				  const double *d_sp_a, const double *d_ap_a, const int *b_length, const double *d_f0_b, const double *d_sp_b,
				  const double *d_ap_b, const int *out_length, const double *d_position_a, const double *d_position_b,
				  const double *d_weight, const double *d_f0_weight, const double *d_ratio_a, const double *d_ratio_b, double *d_f0_out,
				  double *d_sp_out, double *d_ap_out, long long total_out);

// Feature coding (wc_code_features.hip)
// nullptr if (fs, fft_size, nd) can be coded, else why not: fft_size 512 .. 4096, 1 <= nd <= fft_size/4+1, and with the
// aperiodicity fs >= 12 kHz (at least one band)
const char *code_features_check(int fs, int fft_size, int nd, bool with_ap);
// builds and uploads the coding plan of (dev, fs, fft_size) unless it is there already (the only step of a coding call that
// allocates or waits; callers that must not fail behind a state change run it first)
int code_features_prepare(Device *dev, int fs, int fft_size);
// Both rows of n_frames frames -> coded rows, enqueued on s (arguments already checked; d_ap and d_coded_ap both NULL: sp only).
// fft_size 2048 / 4096: the one-wavefront kernel; 512 / 1024: the codec's workgroup-per-frame kernels on the cached plan.
int code_features_enqueue(Device *dev, hipStream_t s, int fs, int fft_size, long long n_frames, int nd, const double *d_sp,
						  const double *d_ap, double *d_coded_sp, double *d_coded_ap);
}  // namespace wc
