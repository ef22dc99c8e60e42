/* ---- Frame filtering on the device: shape a waveform by an envelope gain per frame (extension) ----
 *
 * Every path of this library that changes a voice's spectrum ends in the vocoder.  This one does not: it filters the waveform itself
 * with one gain row per frame, as spectral-differential conversion does (Kobayashi & Toda): F0, excitation and phase stay the
 * speaker's own.  The decoder of the feature codec is exp of a linear map of the coded row, so the decoded difference of two coded
 * rows IS the power ratio of the two envelopes: wc_frame_filter_run_coded_device(to = converted, from = source) stands behind
 * pipeline-coded -> (GMM -> MLPG -> GV) where coded Synthesis would stand.  A header of its own with a binding table of its own in
 * the Python mirror (world_class_amd/filter.py: FILTER_SIGNATURES); tests/filter_rule.py states THE rule in numpy.
 *
 * Layout.  d_x and d_y are packed by x_length, as d_out of wc_synthesis_compute_device is by out_length.  d_rows holds
 * fft_size/2+1 doubles per frame and is packed by f_length, as d_sp is; the coded rows are packed the same way, with
 * number_of_dimensions doubles per frame.  kind says what a row of d_rows is: WC_FILTER_POWER, a power gain, the kind of a
 * spectrogram row, ls = log(g) / 2; WC_FILTER_LOG, natural-log amplitude gains, taken as they are.
 *
 * THE rule.  Everything is in double.  N = fft_size, n = x_length[u], ls_t the log amplitude gains of segment t.
 *   Centres.    h = frame_period_ms * fs / 1000.0.
 *               c_t = (long long)floor(((double)t * frame_period_ms) * (double)fs / 1000.0 + 0.5).
 *   Segments.   S is the least count with c_{S-1} >= n - 1 (wc_frame_filter_segments).  Segment t (0 <= t < S) uses row
 *               min(t, f_length - 1): the last row is held if the caller gave fewer rows.  Rows from S on are not read.
 *   Weights.    A sample k with c_t < k < c_{t+1} has up = (double)(k - c_t) / (double)(c_{t+1} - c_t).  It enters segment t+1 with
 *               weight up and segment t with weight 1.0 - up.  k == c_t enters segment t with weight 1.0.
 *   Span.       Segment t spans a_t = (t ? c_{t-1} + 1 : 0) to b_t = min(n - 1, c_{t+1} - 1), with L_t = b_t - a_t + 1.  Its values
 *               are s_t[j] = x[a_t + j] * w, placed at j = 0..L_t-1 of N points and zero behind.
 *   Response.   M_t is the minimum-phase spectrum of ls_t, as tests/minimum_phase_rule.py states it: the reference's
 *               MinimumPhaseAnalysis, with e^{+i} transforms.  With forward that file's e^{+i} transform,
 *               R = forward(s_t)[0..N/2] * M_t, extended by Hermitian symmetry, and r_t[j] = Re(sum_k R[k] e^{-2 pi i jk/N}) / N.
 *               This is the circular convolution of the segment with the causal minimum-phase response, wrap included: the rule is
 *               the circular one, and a caller wants responses that have decayed within N - L_t samples.
 *   Bad rows.   If a value of ls_t is not finite, the whole row r_t is NaN.  For WC_FILTER_POWER this is judged after the log, so a
 *               gain <= 0, NaN or infinite counts.
 *   Output.     y[k] = 0.0, then y[k] += r_t[k - a_t] for every segment with a_t <= k < a_t + N, t ascending.  No atomics.  Every
 *               sample of y is written.  The result depends neither on the launch shape nor on which utterances share a batch.
 *   Coded call. d[i] = to[i] - from[i]; from == NULL means d = to; with skip_energy != 0, d[0] = 0.0.  The rows of the
 *               spectral-envelope decoder on d, exactly as wc_decode_spectral_envelope_device writes them, go into the handle's
 *               scratch, then the WC_FILTER_POWER call runs: the result equals those two public calls bit for bit.
 * The rule is frame-local: y[0 .. a_t) depends only on x[0 .. c_t) and rows < t.
 *
 * Both run calls only enqueue, on wc_set_stream's stream.  d_y == d_x is allowed, because the outputs are written by a second
 * kernel after every row is formed; any other overlap is refused.  The handle lives on the device that is current at create; one
 * handle serves one call at a time (a call on another stream waits, on the device, for the handle's last call), and two host
 * threads on two handles run side by side.  Scratch: segments x fft_size doubles of response rows for the whole batch (64 x 10 s at
 * 48 kHz / 5 ms: 2.1 GB, the same order as Synthesis's response rows), plus for the coded call the difference and the decoded rows
 * (frames x (number_of_dimensions + fft_size/2+1) doubles).  It lives in the handle, grows on demand and goes with it.
 *
 * Refusals.  Create returns NULL, run returns WC_ERR_INVALID; the text is in wc_last_error.  Every refusal happens before anything
 * is allocated, enqueued or written.  Create refuses: an fft_size other than 512, 1024, 2048 or 4096; fs <= 0; h not finite or < 1;
 * 2 * ceil(h) - 1 > fft_size / 2 (the longest segment must leave half the transform to the response: N = 1024 at 16 kHz takes 16 ms
 * frames and refuses 16.0625 ms).  Run refuses: a NULL handle; n_utt < 0; a negative length; x_length[u] > 0 with f_length[u] < 1;
 * a kind outside {0, 1}; NULL arrays with work to do; d_y overlapping anything but d_x exactly; for the coded call,
 * number_of_dimensions outside 1..fft_size/2 and a NULL d_coded_to.  x_length[u] == 0 writes nothing for that utterance. */
#ifndef WORLD_CLASS_FILTER_H
#define WORLD_CLASS_FILTER_H

#include "world_class_c.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WC_FILTER_POWER 0
#define WC_FILTER_LOG 1

typedef struct wc_frame_filter wc_frame_filter;

wc_frame_filter *wc_frame_filter_create(int fs, int fft_size, double frame_period_ms);
void wc_frame_filter_destroy(wc_frame_filter *f);

/* S of the rule for a signal of x_length samples (host arithmetic only); 0 for x_length == 0 */
int wc_frame_filter_segments(const wc_frame_filter *f, int x_length);

int wc_frame_filter_run_device(wc_frame_filter *f, int n_utt, const double *d_x, const int *x_length, int kind,
                               const double *d_rows, const int *f_length, double *d_y);

int wc_frame_filter_run_coded_device(wc_frame_filter *f, int n_utt, const double *d_x, const int *x_length,
                                     const double *d_coded_to, const double *d_coded_from, int number_of_dimensions,
                                     int skip_energy, const int *f_length, double *d_y);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_FILTER_H */
