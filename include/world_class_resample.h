/* ---- Sample-rate conversion on the device: batches and streams (extension) ----
 *
 * A polyphase Kaiser-windowed-sinc resampler for rational ratios in FP64, in front of the analysis side (wc_stream_create takes only
 * rates that are a multiple of 1000 Hz and of Harvest's decimation) and behind the synthesis side.  A header of its own with a binding
 * table of its own in the Python mirror (world_class_amd/resample.py: RESAMPLE_SIGNATURES).
 *
 * The rule.  fs_in != fs_out, both > 0; zeros (default 64), rolloff (default 0.9475937167399596), beta (default 14.769656459379492);
 * 0 / 0.0 selects the default.
 *   g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g
 *   s = rolloff * min(1.0, (double)L / M), K = (int)ceil(zeros / s), taps = 2K + 1
 * Table G[p][j], p = 0 .. L-1, j = 0 .. 2K, k = j - K (built on the host in double, uploaded at create):
 *   d = (double)(k*L - p) / (double)L              (the numerator is an exact integer)
 *   u = d * s / zeros
 *   w = |u| < 1 ? I0(beta * sqrt(1 - u*u)) / I0(beta) : 0
 *   v = s * d
 *   G = s * (v == 0 ? 1 : sin(pi*v) / (pi*v)) * w
 * Output of an utterance of N input samples: N_out = ceil(N*L / M) in 64-bit integers, and for n < N_out
 *   q = (n*M) div L, p = (n*M) mod L               (64-bit)
 *   y[n] = (((0.0 + x[q-K]*G[p][0]) + x[q-K+1]*G[p][1]) + ... + x[q+K]*G[p][2K])
 * every product rounded, then every sum rounded (no fma), j ascending, EVERY tap added, x outside [0, N) read as +0.0.
 * wc_resample_device and the streams compute exactly this, bit for bit, on the table of wc_resample_filter.
 *
 * A stream commits output n once q(n) + K <= T - 1, T the samples received:
 *   committed(T) = T > K ? min(ceil((T-K)*L / M), ceil(T*L / M)) : 0,   after a flush ceil(T*L / M).
 * A push commits committed(after) - committed(before) outputs, in order and exactly once; the zero tail is added by the flush alone.
 * Latency is K input samples.  The concatenated outputs of a stream are, bit for bit, wc_resample_device's of the whole signal.
 *
 * Formats.  in_format: 0 double, 1 int16 (/32768.0, wc_pcm16_to_double_device's arithmetic), 2 float32 -- as in
 * wc_stream_push_device_fmt.  out_format: 0 double, 1 int16 with wc_double_to_pcm16_device's quantisation.
 *
 * Refused with WC_ERR_INVALID (a negative result; NULL from a _create), the text in wc_last_error: equal rates, a rate below 1,
 * zeros < 0, rolloff outside (0, 1] (0.0 is the default), a beta that is not finite, negative or above 700 (I0 overflows), a table
 * L x (2K+1) of more than 2^21 doubles. */
#ifndef WORLD_CLASS_RESAMPLE_H
#define WORLD_CLASS_RESAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- pure host functions: no handle, no device ---- */
/* L, M and K of the rule (any of the three pointers may be NULL) */
int wc_resample_plan(int fs_in, int fs_out, int zeros, double rolloff, double beta, int *up, int *down, int *half_width);
/* the table, L x (2K+1) doubles, phase-major; capacity: doubles that taps can hold */
int wc_resample_filter(int fs_in, int fs_out, int zeros, double rolloff, double beta, double *taps, long long capacity);
/* N_out of n_in >= 0 samples */
long long wc_resample_out_length(int fs_in, int fs_out, long long n_in);
/* committed(samples_in) of a stream, flushed != 0: after its flush */
long long wc_resample_committed(int fs_in, int fs_out, int zeros, double rolloff, long long samples_in, int flushed);
/* How the kernels cut the work, for tests and tools.  An utterance or a push of at least *phase_min outputs is cut into tiles of
 * *tile_outputs outputs, each of whose wavefronts takes 64 outputs of ONE phase p; a shorter one, and every one where
 * *tile_outputs is 0 (the input tile would not fit the local memory), goes output by output in blocks of *plain_block. */
int wc_resample_tiling(int fs_in, int fs_out, int zeros, double rolloff, int *tile_outputs, int *phase_min, int *plain_block);

/* ---- batch ----
 * wc_resampler_create uploads the table; like every other _create it needs a HIP device.  wc_resample_device: n_utt utterances,
 * packed like every batch here -- utterance u's input at sum of x_length[< u], its output at sum of out_length[< u],
 * out_length = wc_resample_out_length(x_length).  It only enqueues, on wc_set_stream's stream (the descriptors go up through
 * page-locked staging of the handle).  Refused: a length below 1, a batch whose packed output exceeds 2^31 - 1 samples, a format out
 * of range, NULL arrays. */
typedef struct wc_resampler wc_resampler;
wc_resampler *wc_resampler_create(int fs_in, int fs_out, int zeros, double rolloff, double beta);
void wc_resampler_destroy(wc_resampler *r);
int wc_resample_device(wc_resampler *r, int n_utt, const void *d_x, int in_format, const int *x_length, void *d_y, int out_format);

/* ---- streams ----
 * n_streams independent signals on one handle.  n_new and flush are host arrays, 0 <= n_new[u] <= max_samples_per_push, flush NULL:
 * none.  d_chunk is packed by n_new, d_y by samples_out (which the call fills on the host before it returns), as in
 * wc_stream_push_device and wc_synth_stream_push_device; wc_resample_stream_max_out_per_push is the capacity d_y needs per stream
 * (a flush of a full push).
 *
 * Arguments are checked and counts computed on the host before anything is enqueued; a refused push (a count out of range, samples
 * for a flushed stream, NULL arrays with samples to read or to write, a format out of range) leaves every stream as it was.  A flushed
 * stream takes no more samples until wc_resample_stream_reset.  Streams need not move in lockstep, and no stream's outputs depend on
 * another stream's.  A push only enqueues: one asynchronous copy of the per-stream records out of page-locked staging of the handle
 * and up to three launches.  Counters are 64-bit; the kernels see positions relative to the stream's buffer only (q and p of the
 * push's first output are reduced on the host), so a stream that runs for days stays exact.
 *
 * State per stream: the last 2K input samples as doubles, in a ping-pong pair of buffers of 2K + max_samples_per_push doubles.  A
 * push widens the new samples behind the history, runs the batch call's kernels on that buffer and writes the new tail to the other
 * buffer's head, so an error on the device leaves the last good state.
 *
 * wc_resample_stream_create refuses a count below 1 and a max_samples_per_push for which max_out_per_push x M leaves 31 bits. */
typedef struct wc_resample_stream wc_resample_stream;
wc_resample_stream *wc_resample_stream_create(int fs_in, int fs_out, int zeros, double rolloff, double beta, int n_streams,
                                              int max_samples_per_push);
void wc_resample_stream_destroy(wc_resample_stream *h);
int wc_resample_stream_max_out_per_push(const wc_resample_stream *h);
int wc_resample_stream_reset(wc_resample_stream *h, int stream);
int wc_resample_stream_push_device(wc_resample_stream *h, const void *d_chunk, int in_format, const int *n_new, const int *flush,
                                   void *d_y, int out_format, int *samples_out);
/* -1 for a bad index */
long long wc_resample_stream_samples_received(const wc_resample_stream *h, int stream);
long long wc_resample_stream_samples_committed(const wc_resample_stream *h, int stream);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_RESAMPLE_H */
