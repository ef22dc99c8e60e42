/* world_class_stream.h -- chunked ("streaming") Harvest + CheapTrick for many concurrent streams (extension).
 *
 * The reference has no streaming mode: Harvest (reference src/harvest.cpp) is non-causal -- zero-phase decimation
 * (:1400-1410), a +-100-frame section extension (:431-440), a forward-backward smoothing filter run over the contour
 * padded by 300 frames either side (:676-703) -- and CheapTrick draws its noise from a position that depends on every
 * earlier frame.  The semantics defined here (BASELINE config 5):
 *
 *   Every stream accumulates its samples in a device-resident history of at most  W = lookback + chunk + lookahead  ms.
 *   A push appends `chunk` ms to every stream and runs the WHOLE-UTTERANCE Harvest of this library on each stream's
 *   history window -- the same kernels, the window being an utterance that starts at an absolute time which is a
 *   multiple of lcm(8 ms, frame period), so that frame grid, decimation phase and the smoothing filter's start phase
 *   fall where they fall in the whole signal.  Of the window's contour only the frames at least `lookahead` ms before the
 *   newest sample (and, once the history is full, at least `lookback` ms after the oldest) are committed: each absolute
 *   frame k (time k * frame_period) is committed exactly once, in order, `chunk / frame_period` frames per push in the
 *   steady state.  CheapTrick then runs on the committed frames only, reading the samples from the history and taking
 *   its noise draws from the stream's own position in the reference's xorshift128 sequence, which is carried from push to
 *   push -- exactly the draws the frames would have got in one whole-utterance call.
 *   A stream is closed by a push with flush[u] != 0 (its last chunk may be shorter): all remaining frames are committed,
 *   the window ending where the signal ends.
 *   One property of the reference has to be pinned for this to be well defined: its decimator aligns the sampling phase to
 *   the END of the signal (reference src/world_matlabfunctions.cpp:201-206, nbeg = length mod ratio, MATLAB's decimate), so
 *   the contour of a whole-utterance call changes by tenths of a Hz with (total length mod decimation ratio) -- one or two
 *   trailing samples -- which no stream can know in advance.  Harvest therefore always sees windows that are a multiple of
 *   the ratio long: full chunks are, and of a short final chunk the last (length mod ratio) samples are used by CheapTrick
 *   only.  The stream equals the whole-utterance call exactly for totals that are multiples of the ratio; for others it
 *   equals Harvest on the signal without those trailing samples (frame count wc_get_samples of that length) followed by
 *   CheapTrick on the complete signal.
 *
 *   Result: the committed (tpos, f0, spectrogram rows) equal those of ONE whole-utterance Harvest + CheapTrick call on
 *   the complete signal wherever the influence of the window edges has died out: lookahead and lookback of >= 400 ms
 *   (300 padded + 100 extension frames at Harvest's internal 1 ms grid) make that every frame on ordinary speech;
 *   tests/test_gpu_stream.py compares whole streams (voicing decisions identical, F0 within 1e-9 Hz -- last-bit
 *   differences come from the limit cycle of the smoothing filter's backward pass, whose phase depends on where the
 *   window ends -- spectrogram within 1e-7 relative).  Algorithmic latency: lookahead + chunk (+ the push's run time).
 *
 * Layout: d_chunk holds the new samples of the streams back to back (stream u's at sum(n_new[<u])); the outputs are
 * packed the same way by the number of frames committed for each stream (frames_out, host array).  Capacity needed:
 * wc_stream_max_frames_per_push() rows per stream.
 */
#ifndef WORLD_CLASS_STREAM_H
#define WORLD_CLASS_STREAM_H

#include "world_class_c.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wc_stream wc_stream;

/* fs must be a multiple of 1000 with fs/1000 a multiple of Harvest's decimation ratio (8, 16, 24, 32, 48, 96 kHz ...);
 * frame_period_ms a whole number of ms; chunk_ms, lookback_ms, lookahead_ms multiples of lcm(8, frame_period_ms).
 * Harvest / CheapTrick options as in wc_harvest_create / wc_cheaptrick_create (fft_size 0 = automatic). */
wc_stream *wc_stream_create(int fs, int n_streams, double frame_period_ms, int chunk_ms, int lookback_ms, int lookahead_ms,
                            double harvest_f0_floor, double harvest_f0_ceil, double q1, double cheaptrick_f0_floor, int fft_size);
void wc_stream_destroy(wc_stream *s);
/* Incremental mode (call before the first push; 0 switches back).  Harvest's front -- decimation, band-pass, zero crossings, raw
 * candidates, refinement -- is local: what it yields for a 1 ms frame depends on +-`context_ms` of signal (160 ms covers the
 * longest band-pass, the lowest band's periods, the refinement window and the +-3-frame overlap with room to spare).  In this mode
 * a push runs the front on the newest chunk + 2 context only and appends the refined candidate / score rows of the frames that
 * have their full context to a per-stream ring; only Harvest's tail (unreliable-candidate test, contour logic, smoothing) runs over
 * the window, on rows from the ring.  The context is part of the lookahead (rows exist up to `context` behind the newest sample, the
 * tail looks `lookahead - context` ahead of the newest committed frame): lookahead 560 ms with context 160 ms gives the tail the
 * same 400 ms it has with whole windows.  Same committed frames, same parity bar; about half the work per push. */
int wc_stream_set_incremental(wc_stream *s, int context_ms);
int wc_stream_get_fft_size(const wc_stream *s);
int wc_stream_chunk_samples(const wc_stream *s);        /* samples per stream of a full chunk */
int wc_stream_max_frames_per_push(const wc_stream *s);  /* most frames one push can commit for one stream (a flush) */
/* Forget stream u's history and position (a new signal starts on it). */
int wc_stream_reset(wc_stream *s, int stream);
/* n_new: host array, samples appended per stream: wc_stream_chunk_samples() (NULL = that for all), 0 (stream idle this
 * push) or, only together with flush[u], anything in between.  flush: host array of flags or NULL.
 * d_tpos / d_f0: committed frames (absolute times in seconds), d_sp: their spectrogram rows [fft_size/2+1];
 * frames_out: host array [n_streams], frames committed by this push. */
int wc_stream_push_device(wc_stream *s, const double *d_chunk, const int *n_new, const int *flush, double *d_tpos, double *d_f0,
                          double *d_sp, int *frames_out);
/* The same with the new samples as int16 PCM (chunk_format 1: sample / 32768, the reference's wavread scaling) or float32 (2),
 * widened on the device; 0 = float64. */
int wc_stream_push_device_fmt(wc_stream *s, const void *d_chunk, int chunk_format, const int *n_new, const int *flush, double *d_tpos,
                              double *d_f0, double *d_sp, int *frames_out);
/* Position of stream u in the reference's noise sequence (reference src/world_matlabfunctions.cpp:243-264): where CheapTrick's next
 * committed frame takes its draws.  0 after creation and after wc_stream_reset -- the position a fresh reference process starts
 * from; set it to continue the numbering of an earlier analysis (e.g. the value wc_rng_get_position() reports after one). */
unsigned long long wc_stream_rng_position(const wc_stream *s, int stream);
int wc_stream_set_rng_position(wc_stream *s, int stream, unsigned long long position);
/* Aperiodicity (opt-in, before the first push; a negative threshold switches it off again): D4C (wc_d4c_create's threshold) runs on the
 * frames each push commits, on the same window batch and whole-ms relative times as CheapTrick, with a noise position of its own
 * per stream.  Needs lookback and lookahead of at least 38 ms (D4C's and LoveTrain's windows reach 37.5 ms either side of a frame).
 * What cannot be exact: a whole-utterance D4C takes its LoveTrain draws for ALL frames before any main-pass draw (reference
 * src/d4c.cpp:113-160), and a stream cannot know where that boundary falls, so each push's frames draw their LoveTrain noise and
 * then their main-pass noise from the stream's D4C position.  The noise has amplitude kMySafeGuardMinimum (1e-12): against one
 * whole-utterance D4C on the stream's committed F0 the LoveTrain voicing is identical and ap within 1e-7.  Without the option
 * nothing changes.  With it, push through wc_stream_push_device_ex (d_ap: rows of fft_size/2+1, packed like d_sp). */
int wc_stream_set_aperiodicity(wc_stream *s, double d4c_threshold);
int wc_stream_push_device_ex(wc_stream *s, const void *d_chunk, int chunk_format, const int *n_new, const int *flush, double *d_tpos,
                             double *d_f0, double *d_sp, double *d_ap, int *frames_out);
/* The same push with the committed frames CODED (world_class_codec.h: wc_code_features_device): the rows go to buffers of the handle
 * (max_frames_per_push x n_streams rows, allocated on the first coded push, released by wc_stream_destroy) and are coded from
 * there on the caller's stream into d_coded_sp (number_of_dimensions doubles per frame, 1 .. fft_size/4+1) and d_coded_ap
 * (GetNumberOfAperiodicities(fs) per frame), packed by frames_out like d_f0.  d_coded_ap goes with wc_stream_set_aperiodicity
 * (and an fs of at least 12 kHz): non-NULL on a stream with it, NULL on one without (spectral envelope only); the other two
 * combinations are refused.  Arguments are checked and the buffers reserved before the push: a refused call leaves every stream's
 * state untouched.  Coded and plain pushes may alternate on a handle; frames, noise positions and accounting are those of the
 * plain push.  With wc_synth_stream_push_coded_device and wc_synth_stream_set_modification this closes the loop analysis ->
 * modify -> synthesis in the coded domain without a row leaving the device: 60 + 5 doubles per frame instead of 2 x 1025 at 48 kHz. */
int wc_stream_push_coded_device(wc_stream *s, const void *d_chunk, int chunk_format, const int *n_new, const int *flush, double *d_tpos,
                                double *d_f0, double *d_coded_sp, int number_of_dimensions, double *d_coded_ap, int *frames_out);
/* D4C's noise position of stream u (0 after creation and reset) */
unsigned long long wc_stream_d4c_rng_position(const wc_stream *s, int stream);
int wc_stream_set_d4c_rng_position(wc_stream *s, int stream, unsigned long long position);
/* frames committed so far / samples received so far for stream u */
long long wc_stream_frames_committed(const wc_stream *s, int stream);
long long wc_stream_samples_received(const wc_stream *s, int stream);

/* ---- Chunked Synthesis for many concurrent streams (extension) ----
 *
 * Stream u receives frames 0, 1, 2, ... (f0, spectrogram row, aperiodicity row of fft_size/2+1) in order, frame k at time
 * k * frame_period.  The samples it commits are the samples of ONE wc_synthesis_compute_device call over all of its frames
 * (out_length = wc_synthesis_out_length(total frames), noise from the stream's position, which is 0 after create and reset):
 * at fft_size 1024 and 2048 bit for bit with the batch's default path (the same response rows summed in the same pulse order;
 * the batch's A/B variants WC_SYN_IMPL=block and WC_SYN_OLA=atomic, and batches whose rows exceed its row budget, add with FP64
 * atomics instead and agree within 1e-12), at 512 and 4096 within 1e-12 (the batch's block kernels add with FP64 atomics there).  Every output sample is committed exactly once and in order, as
 * soon as no later frame can change it (reference src/synthesis.cpp):
 *   - sample i's F0 / VUV interpolates frames floor(i / fs / frame_period) and the one after it (:180-243): it is final once
 *     i / fs < (F - 1) * frame_period for F frames received; the extrapolated point at f0_length exists only at the flush;
 *   - a pulse at sample i is found when sample i + 1 is final (:264-283); its noise_size needs the NEXT pulse (:106-107), so
 *     the newest pulse waits for its successor (the last pulse of the utterance gets 0 at the flush);
 *   - a pulse's response covers samples index - fft_size/2 + 1 .. index + fft_size/2 (:118-139).
 * So after a push with F frames received the stream has committed every sample below  min(P, E - 1) - fft_size/2 + 1,  where E
 * is the first sample at or after (F - 1) frame periods and P the waiting pulse.  Latency bound (tested): committed >=
 * (F - 2) * frame_period * fs - gap - fft_size/2, with the pulse gap at most 2 fs / (fs/fft_size + 1) samples in voiced
 * stretches (the interpolated F0 stays above half the lowest F0) and fs/500 in unvoiced ones: about one frame period, plus the
 * current pulse gap (of the F0 that reaches Synthesis: f0 * f0_scale under wc_synth_stream_set_modification), plus fft_size/2 samples.  A flush commits everything up to wc_synthesis_out_length; a stream with fewer
 * than two frames when flushed is an error.  Streams need not move in lockstep; a push that fails leaves every stream as it
 * was.  A stream holds at most 2^31 samples (the reference's int indices).
 *
 * Per stream the handle carries the absolute next sample, the total and wrapped phase of the last final sample (the reference's
 * sequential sum continued bit for bit), the waiting pulse, the noise position, a window of the frames that pending samples and
 * pulses still need, and the partial sums of samples that final pulses have reached but later ones may still reach.
 */
typedef struct wc_synth_stream wc_synth_stream;
/* fft_size 512, 1024, 2048 or 4096 (as wc_synthesis_create); max_frames_per_push: most frames one push gives one stream */
wc_synth_stream *wc_synth_stream_create(int fs, int fft_size, double frame_period_ms, int n_streams, int max_frames_per_push);
void wc_synth_stream_destroy(wc_synth_stream *s);
int wc_synth_stream_max_samples_per_push(const wc_synth_stream *s);  /* d_y capacity per stream */
int wc_synth_stream_reset(wc_synth_stream *s, int stream);
/* n_frames: host array, frames appended per stream (0 = idle).  The frames are packed back to back in d_f0 / d_sp / d_ap (rows of
 * fft_size/2+1), as wc_stream_push_device packs the frames it commits.  flush: host flags or NULL.  d_y: the committed samples,
 * packed by samples_out[u] (host array). */
int wc_synth_stream_push_device(wc_synth_stream *s, const int *n_frames, const int *flush, const double *d_f0, const double *d_sp,
                                const double *d_ap, double *d_y, int *samples_out);
/* The same with coded rows (world_class_codec.h): d_coded_sp / d_coded_ap hold number_of_dimensions / GetNumberOfAperiodicities(fs)
 * doubles per frame, packed like d_f0.  They are decoded (wc_decode_features_device) into rows of the handle (max_frames_per_push x
 * n_streams, allocated on the first coded push, released by wc_synth_stream_destroy) and pushed as by wc_synth_stream_push_device:
 * the samples are those of one wc_synthesis_compute_coded_device call per stream.  number_of_dimensions and fs are checked as
 * there; a push that fails leaves every stream as it was. */
int wc_synth_stream_push_coded_device(wc_synth_stream *s, const int *n_frames, const int *flush, const double *d_f0,
                                      const double *d_coded_sp, int number_of_dimensions, const double *d_coded_ap,
                                      double *d_y, int *samples_out);
/* Pitch and formant shift of one stream (the demo's ParameterModification, world_class_io.h), a host-side setting: (1.0, 0.0) --
 * neutral -- after wc_synth_stream_create and wc_synth_stream_reset.  Refused with WC_ERR_INVALID, the setting unchanged, unless
 * f0_scale is finite and > 0 and spectral_ratio is 0 (none) or finite and >= 2.0 / fft_size.  It applies to the frames that later
 * wc_synth_stream_push_coded_device calls give that stream, so a change between two pushes takes effect at a frame boundary: the
 * push decodes those frames with wc_decode_features_modified_device at the stream's ratio and synthesises them with
 * f0 * f0_scale (kept in a buffer of the handle, max_frames_per_push x n_streams doubles, reserved on first use; the caller's
 * d_f0 is not written).  The per-frame values go up through page-locked staging of the handle with an asynchronous copy, without
 * a host synchronisation of their own.  A push in which every stream that receives frames is neutral is the push without
 * settings: the same samples and the same cost.  The pulse-gap bound of the header's latency statement is a bound on the F0 that
 * reaches Synthesis: with a setting it holds for f0 * f0_scale.
 * wc_synth_stream_push_device takes full rows as they are and applies no setting: while a stream that receives frames in that
 * push has a setting other than (1.0, 0.0) the push is refused and every stream keeps its state. */
int wc_synth_stream_set_modification(wc_synth_stream *s, int stream, double f0_scale, double spectral_ratio);
/* Speed of one stream (time-scale modification, the streaming form of wc_retime_parameters_device and
 * wc_synthesis_compute_coded_retimed_device), a host-side setting like wc_synth_stream_set_modification: 1.0 after
 * wc_synth_stream_create and wc_synth_stream_reset; refused with WC_ERR_INVALID, the setting unchanged, unless it is finite and > 0
 * (and, for a retimed stream, unless floor(last + speed) >= F - 1: below).
 * The frames a caller pushes are SOURCE frames; what the stream synthesises are SYNTHESIS frames, formed along the time map
 *   pos[0] = 0,  pos[k] = pos[k-1] + speed_k   (one double addition, speed_k the speed in effect at the push that forms frame k),
 * cut at F - 1 for F source frames received.  A push that gives the stream n source frames makes F += n and then forms, one after
 * the other, every frame whose position p = last + speed (0.0 for the first) satisfies p <= F - 1 -- the condition that source
 * rows floor(p) and, for a fractional p, floor(p) + 1 are in; nothing formed is ever revised, a flush forms nothing extra (positions
 * beyond F - 1 are dropped, the end frame is not held).  The frame at p is wc_retime_parameters_device's frame at that position,
 * bit for bit: i = floor(p), a = p - i; a == 0 copies source frame i, a > 0 writes (1 - a) * row[i] + a * row[i + 1] for both rows
 * with that call's voiced / unvoiced F0 rule; then f0 *= f0_scale and the sp row is stretched by the stream's spectral_ratio
 * (wc_synth_stream_set_modification, coded pushes), per synthesis frame as in wc_synthesis_compute_coded_retimed_device.  The frames
 * formed are appended to the stream as wc_synth_stream_push_device appends rows: the samples are those of ONE
 * wc_synthesis_compute_coded_retimed_device (coded pushes) or wc_retime_parameters_device + wc_synthesis_compute_device (full rows)
 * call over all source frames with the stream's positions, and the commit rule, the noise draws and the latency bound above hold
 * in synthesis frames; in source frames a stream waits at most one frame longer, for frame ceil(p).
 * Which streams are retimed: a stream becomes retimed at the first push that gives it frames while its speed is not 1.0 and stays
 * so until wc_synth_stream_reset, also after the speed returns to 1.0.  A retimed stream in a coded push is decoded by the unmodified
 * decoder, scale and ratio applied per synthesis frame behind the interpolation; wc_synth_stream_push_device takes full rows for it
 * (retimed without scale or ratio; a stream with a modification setting is still refused there).  A stream that is not retimed is
 * handled as without this setting whatever its neighbours do (in a coded push its ratio goes into the decoder; beside retimed streams
 * its rows pass the retiming kernel at whole positions, a copy), no stream's samples depend on another stream's settings, and a
 * push in which no stream that receives frames is retimed runs the code it ran before: no extra launch, copy or allocation (but
 * for the kept coded frame of streams with a modification setting that called this function, below).
 * Per retimed stream the handle carries `last`, F and ONE source row (frame F - 1: after a push the next position lies beyond
 * F - 2); the carried rows are a ping-pong pair, the retimed rows (max_frames_per_push x n_streams, both matrices and F0) and the
 * page-locked staging of descriptors, positions, scales and ratios are reserved on the first retimed push and released by
 * wc_synth_stream_destroy.  Two things follow from the one carried row.  A stream that becomes retimed after frames at speed 1.0
 * takes its carried row from its frame window; if its newest frame was decoded with a modification setting, that row is already
 * scaled and stretched, so once wc_synth_stream_set_speed was called for a stream (any value, 1.0 included; until the next reset) the
 * coded pushes that apply a setting to it while it is not retimed also keep its newest CODED frame in the handle (one small launch in
 * such a push, fed by the staging copy the settings take anyway; a ping-pong pair, so a push that is refused leaves the frame of the
 * push before; streams that never called this function do not run it) and the frame is decoded once more, unmodified, when the
 * stream becomes retimed.  A stream with a setting whose newest frame was pushed before any call of this function has no such frame:
 * the push that would make it retimed, and wc_synth_stream_frames_for_push, are refused with WC_ERR_INVALID; call this function with
 * 1.0 before the first frame, or push once more at 1.0 after the call.  The frames formed
 * before that were stretched inside the decoder: against the whole-utterance retimed call their rows differ as
 * wc_decode_features_modified_device differs from decode + wc_modify_parameters_frames_device (1e-12 relative), the frames formed
 * from then on not at all.  And the next position last + speed needs row floor(last + speed), while rows before F - 1 are gone: for
 * a retimed stream that has formed a frame this function refuses a speed with floor(last + speed) < F - 1 (F source frames received)
 * and keeps the setting.  That depends on the phase: at last = F - 1 every speed passes, at last = F - 1.5 none below 0.5; after a fast
 * stretch a stream slows down over several pushes.  No push fails for it, of this stream or another.
 * Refused with WC_ERR_INVALID on the host before anything is enqueued, every stream, carried row and kept frame as it was: a push
 * that would form more than max_frames_per_push synthesis frames for one stream (the count stops at that bound: a speed of 1e-300
 * costs nothing), and a flush that leaves a stream with fewer than two synthesis frames. */
int wc_synth_stream_set_speed(wc_synth_stream *s, int stream, double speed);
/* `last`: the position in source frames of the newest synthesis frame formed; NaN before the first one or for a bad index */
double wc_synth_stream_source_position(const wc_synth_stream *s, int stream);
/* synthesis frames formed so far (wc_synth_stream_frames_received counts the source frames pushed; equal unless retimed); -1 for a
 * bad index */
long long wc_synth_stream_frames_synthesised(const wc_synth_stream *s, int stream);
/* synthesis frames a push of n_frames source frames would form for the stream at its current setting: host arithmetic only, capped
 * at max_frames_per_push + 1 (a push that would be refused for its count); WC_ERR_INVALID (negative) for a bad argument and for a
 * stream that cannot become retimed (no kept frame, above) */
int wc_synth_stream_frames_for_push(const wc_synth_stream *s, int stream, int n_frames);
/* noise position of stream u: where its next (or waiting) pulse takes its draws */
unsigned long long wc_synth_stream_rng_position(const wc_synth_stream *s, int stream);
int wc_synth_stream_set_rng_position(wc_synth_stream *s, int stream, unsigned long long position);
long long wc_synth_stream_frames_received(const wc_synth_stream *s, int stream);
long long wc_synth_stream_samples_committed(const wc_synth_stream *s, int stream);

/* ---- Morph streams: two voices per stream, blended push by push into synthesis frames (extension) ----
 *
 * The streaming form of wc_morph_parameters_device (world_class_io.h), as wc_synth_stream_set_speed is that of
 * wc_retime_parameters_device.  The handle sits IN FRONT of a synthesis stream: a push takes source frames of voice A and of voice B
 * for every stream and writes the morphed frames they now allow as full rows (F0, sp row, ap row of fft_size/2+1) into the caller's
 * buffers; the caller hands those rows to wc_synth_stream_push_device, which is unchanged.  Nothing of wc_synth_stream is touched, and
 * the rows take the trip through device memory that the retimed rows of a synthesis stream take.
 *
 * The rule (host arithmetic).  Per stream the handle keeps Fa and Fb, the source frames received from each voice; whether a frame
 * has been formed; last_a and last_b, the positions of the newest formed frame; and the settings speed_a, speed_b (1.0), weight,
 * f0_weight (0.0), ratio_a, ratio_b (0.0: none) -- host-side settings that take effect at the next push.  A push gives stream u
 * n_a[u] frames of A and n_b[u] frames of B (either may be 0): Fa += n_a, Fb += n_b, and then frames are formed one after the other:
 *   pa = last_a + speed_a,  pb = last_b + speed_b   (one double addition each; 0.0 and 0.0 for the first frame of the stream),
 * while pa <= Fa - 1 and pb <= Fb - 1; each frame takes the weight, F0 weight and ratios in effect at this push, and last_a = pa,
 * last_b = pb.  Nothing formed is ever revised and there is no flush: positions past the last row are dropped and end frames are not
 * held, as in wc_synth_stream_set_speed.
 * Every formed frame is, bit for bit, the frame wc_morph_parameters_device writes for ONE pair (all of A, all of B) at
 * d_position_a = pa, d_position_b = pb, d_weight, d_f0_weight, d_ratio_a, d_ratio_b: its copy paths at a weight of 0 or 1 and at
 * whole positions, its nearer-source F0 rule, its log-domain stretch.  (Positions never need that call's end clamp: p <= F - 1.)
 * No stream's frames depend on another stream's counts or settings.
 *
 * The backlog.  Two voices are consumed at two rates, so rows of the voice that is fed faster wait for the other.  After a push
 * voice x keeps rows keep_x .. Fx - 1, keep_x = floor(last_x) (0 before the first frame): no positive speed can ask for an older
 * row; backlog_x = Fx - keep_x.  Because row floor(last_x) stays, wc_morph_stream_set_speeds takes any finite speed > 0 at any time
 * (the phase-dependent refusal of wc_synth_stream_set_speed does not arise).  The handle is created with max_backlog (>= 2) rows
 * per stream and voice and allocates at create: per stream and voice max_backlog + min(max_backlog, max_frames_per_push) slots of
 * F0 and both rows -- the rows a push adds go to slots that the state before the push does not hold, so a push that fails on the
 * device with a HIP error leaves the host state and the kept rows of the last good push, and kept rows are never copied twice --
 * together with the device array and the two page-locked staging buffers of the per-frame records.  wc_morph_stream_destroy
 * releases them.
 *
 * Refused with WC_ERR_INVALID on the host before anything is enqueued, every stream, setting and kept row as it was: a negative
 * count; n_a[u] or n_b[u] above max_frames_per_push; a push that would form more than max_frames_per_push frames for one stream
 * (the count stops at the bound: a speed of 1e-300 costs nothing); a push after which a backlog would exceed max_backlog; NULL
 * arrays with frames to read or to write; and in the setters a speed that is not finite and > 0, a weight or F0 weight that is not
 * finite, a ratio that is neither 0 nor finite and >= 2.0 / fft_size, a bad stream index.
 *
 * Layout: n_a / n_b are host arrays; each voice's frames are packed stream by stream in its three arrays, as for
 * wc_synth_stream_push_device; the formed frames are packed by frames_out[u] (host array), the outputs hold n_streams x
 * max_frames_per_push rows.  fft_size is 512, 1024, 2048 or 4096.  A push is stream-ordered on the caller's stream (wc_set_stream)
 * and only enqueues: the positions, weights, ratios and row references of the formed frames go up through the handle's staging
 * with one asynchronous copy, one launch forms the frames and keeps the rows (the variant without shared memory while no stream
 * that forms frames has a ratio).  A handle is driven on one stream at a time. */
typedef struct wc_morph_stream wc_morph_stream;
wc_morph_stream *wc_morph_stream_create(int fs, int fft_size, int n_streams, int max_frames_per_push, int max_backlog);
void wc_morph_stream_destroy(wc_morph_stream *m);
/* the stream as after create: no frames, speeds 1, weights 0, ratios 0 */
int wc_morph_stream_reset(wc_morph_stream *m, int stream);
int wc_morph_stream_set_speeds(wc_morph_stream *m, int stream, double speed_a, double speed_b);
int wc_morph_stream_set_weight(wc_morph_stream *m, int stream, double weight, double f0_weight);
int wc_morph_stream_set_ratios(wc_morph_stream *m, int stream, double ratio_a, double ratio_b);
/* frames a push of n_a and n_b source frames would form for the stream at its current speeds: host arithmetic only, capped at
 * max_frames_per_push + 1 (a push that would be refused for its count); WC_ERR_INVALID (negative) for a bad argument */
int wc_morph_stream_frames_for_push(const wc_morph_stream *m, int stream, int n_a, int n_b);
int wc_morph_stream_push_device(wc_morph_stream *m, const int *n_a, const double *d_f0_a, const double *d_sp_a, const double *d_ap_a,
                                const int *n_b, const double *d_f0_b, const double *d_sp_b, const double *d_ap_b,
                                double *d_f0_out, double *d_sp_out, double *d_ap_out, int *frames_out);
/* The same with coded rows (world_class_codec.h): number_of_dimensions / GetNumberOfAperiodicities(fs) doubles per frame.  The pushed
 * rows of both voices are decoded by the unmodified decoder (wc_decode_features_device; its refusals) into buffers of the handle
 * (n_streams x max_frames_per_push rows per voice and matrix, reserved on the first coded push, released by
 * wc_morph_stream_destroy), then the push is the full-row push: its frames equal wc_decode_features_device followed by
 * wc_morph_stream_push_device bit for bit.  The backlog always holds full rows, so coded and full-row pushes may alternate. */
int wc_morph_stream_push_coded_device(wc_morph_stream *m, const int *n_a, const double *d_f0_a, const double *d_coded_sp_a,
                                      const double *d_coded_ap_a, const int *n_b, const double *d_f0_b, const double *d_coded_sp_b,
                                      const double *d_coded_ap_b, int number_of_dimensions,
                                      double *d_f0_out, double *d_sp_out, double *d_ap_out, int *frames_out);
/* source: 0 = voice A, 1 = voice B.  last_a / last_b: NaN before the first frame or for a bad index */
double wc_morph_stream_source_position(const wc_morph_stream *m, int stream, int source);
/* source frames received / rows kept (backlog_x) / frames formed so far; -1 for a bad index */
long long wc_morph_stream_frames_received(const wc_morph_stream *m, int stream, int source);
int wc_morph_stream_backlog(const wc_morph_stream *m, int stream, int source);
long long wc_morph_stream_frames_formed(const wc_morph_stream *m, int stream);

#ifdef __cplusplus
}
#endif

/* ---- Alignment streams: a live voice followed row by row through a known track (extension) ----
 * The streaming form of wc_align_features_ex_device at step pattern 0 with an open end: every pushed row gets its position in the
 * track and the cost so far, from one row of state per stream.  The rule and the wc_align_stream_* calls are in the header below. */
#include "world_class_align_stream.h"
/* A search window around the last position and a position that never falls (wc_align_stream_set_window): the header below. */
#include "world_class_align_window.h"
/* Settled positions from a lagged backtrack: where the row L frames ago lies on the path behind the newest row, and the flush
 * (wc_align_stream_reserve_lag, _set_lag, _push_settled_device, _tail_device): the header below. */
#include "world_class_align_lag.h"
/* Track-morph streams: a live voice morphed with a resident track at positions the kernel reads from device memory, such as the
 * settled positions above, push by push and with a flush (wc_track_morph_*): the header below. */
#include "world_class_track_morph.h"

#endif /* WORLD_CLASS_STREAM_H */
