/* ---- Warp streams: a resident take played on a live voice's timing (extension) ----
 *
 * world_class_warp.h resamples whole signals along whole maps.  Here the signal is a track that is resident in the handle and the
 * map arrives entry by entry: an alignment stream (world_class_align_stream.h, world_class_align_lag.h) follows a live voice through
 * the track and writes one settled position per pushed row into device memory, and this handle consumes those doubles where they
 * lie and writes the track's waveform on the voice's timing -- a backing vocal, a dubbed line, a guide track that follows a
 * performer.  A header of its own with a binding table of its own in the Python mirror (world_class_amd/warp_stream.py:
 * WARP_STREAM_SIGNATURES); nothing of world_class_warp.h is touched.
 *
 * Committed outputs.  The map rule of world_class_warp.h is causal up to one entry: output n reads the entries floor(t) and
 * floor(t) + 1, t = (double)n / out_per_entry.  After E >= 1 consumed entries a stream has committed c(E) outputs, c(0) = 0:
 *   c(E) = the number of n >= 0 with (double)n / out_per_entry <= (double)(E - 1)
 * -- the rule's own division, in double.  The condition is monotone in n, so wc_warp_stream_committed starts at
 * floor((E - 1) x out_per_entry) and corrects with the predicate; c is the predicate, not the product.  (It has equalled
 * wc_warp_map_out_length(E, out_per_entry) wherever both were compared; nothing proves that they agree everywhere.)
 *
 * A prefix is enough.  Output n < c(E) under the map rule at L = E is, bit for bit, the map rule at any L' >= E on a map with the
 * same first E entries: where t < E - 1 both interpolate the entries floor(t) and floor(t) + 1 <= E - 1; where t == E - 1 the short
 * map holds its end and the long one takes its w == 0 branch, and both give map[E - 1].  So the host counts a push's outputs from
 * the number of entries alone and never looks at a position, and a stream's concatenated outputs are the whole call's.
 *
 * The whole call.  wc_warp_along_map_device is wc_warp_map_positions_device followed by wc_warp_device without the positions in
 * between: output n of utterance u is wc_warp_device's output at wc_warp_map_positions' position, bit for bit; the kernel forms the
 * position from the map where wc_warp_device's reads it, and no position array is written or read.  Packed like those two calls:
 * utterance u's input at the sum of x_length[< u], its map at the sum of map_length[< u], its outputs at the sum of out_length[< u].
 * It only enqueues, on wc_set_stream's stream, with its records through the handle's page-locked staging.  Refused, before the
 * first enqueue, with everything either of the two calls refuses: NULL arrays, n_utt < 1, an x_length or map_length below 1, an
 * out_length below 0, a packed output above 2^31 - 1 samples, a format out of range, an out_per_entry or in_per_unit that is not
 * finite and positive.
 *
 * Tracks.  wc_warp_stream_create allocates n_tracks slots of max_track_samples samples, kept in track_format (0 double, 1 int16,
 * 2 float32: the converters' formats) -- one format per handle, so one kernel variant serves every launch.  Its first seven
 * arguments are wc_vresampler_create's plan.  wc_warp_stream_set_track_device(h, track, n_samples, d_x) copies n_samples samples
 * (1 <= n_samples <= max_track_samples) of that format into a slot, stream-ordered.  Many streams may share a slot; the call is
 * refused while a stream that has received rows is attached to it.  wc_warp_stream_track_length: n_samples, 0 for a slot that has
 * not been set, -1 for a bad index.
 *
 * wc_warp_stream_reset(h, stream, track, delay, out_per_entry, in_per_unit) attaches the stream to a slot that has been set, with a
 * delay D, 0 <= D <= max_delay: the lag of the alignment stream whose settled positions it will be given (0: positions of the rows
 * themselves, a d_b_on_a, any time map).  Counts go to zero and the next output is n = 0.  Each stream has its own out_per_entry
 * <= max_out_per_entry and in_per_unit; the track's rate need not be the output's.
 *
 * The push.  A push gives stream u n_rows[u] doubles (a host array of counts), packed stream by stream in d_map: exactly d_settled
 * of wc_align_stream_push_settled_device called with the same counts.  With i the index of a pushed row since the reset:
 *   i <  D   the row's double is not read;
 *   i >= D   the row's double is map entry i - D.
 * So a push consumes max(n + n_rows[u] - D, 0) - max(n - D, 0) entries, n the rows received before, the first of them
 * max(D - n, 0) doubles into the stream's slice, and samples_out[u] = c(E_after) - c(E_before): host arithmetic on counts alone,
 * filled before the call returns.  The outputs c(E_before) .. c(E_after) - 1 are packed by samples_out in d_y, which holds
 * n_streams x wc_warp_stream_max_out_per_push samples.
 *
 * The flush.  When the voice ends, its last min(D, n) entries still wait in the alignment stream.  wc_warp_stream_flush_device(h,
 * want, d_tail, ..) takes d_tail in the layout wc_align_stream_tail_device writes for the same want: min(D + 1, n) doubles per
 * wanted stream, packed in stream order, of which the last min(D, n) are the remaining entries (when n > D the first belongs to an
 * entry a push has consumed, and is skipped).  The outputs up to c(n) are written, samples_out[u] of them for a wanted stream and
 * 0 for the others; d_y holds n_streams x wc_warp_stream_max_out_per_flush samples.  Afterwards the stream has ended: rows are
 * refused until the next reset.  A wanted stream with D = 0 or without rows is refused, as the tail call refuses it.
 *
 * Bit identity.  For any cut into pushes, a stream's concatenated outputs, flush included, are wc_warp_along_map_device's for (the
 * track, the map of all consumed entries, out_length = c(E_total)): wc_warp_map_positions followed by wc_warp_device.  A NaN entry
 * is silence at the outputs that read it and touches no other, also when it is the entry carried from one push to the next.
 * Positions may fall, jump, repeat or leave the track.  No stream's outputs depend on another stream.
 *
 * State.  Per stream on the device: the last consumed entry, kept in a pair of which a push reads one and writes the other, so a
 * push never writes what the state before it needs; a push that fails on the device with a HIP error leaves the host state and
 * the carried entry of the last good push.  The counters are 64-bit on the host; the kernel sees the absolute n only in
 * (double)n.  wc_warp_stream_create allocates everything: the tracks, the carried entries, the device array and the two
 * page-locked staging buffers of the records.  wc_warp_stream_destroy releases them.
 *
 * Refused with WC_ERR_INVALID on the host before anything is enqueued, every stream as it was: a bad stream or track index; a count
 * that is negative or above max_entries_per_push; rows for a stream that is not attached or has ended; NULL arrays with entries to
 * read or outputs to write; a NULL n_rows, want or samples_out; a delay outside 0 .. max_delay; a reset onto a slot that has not
 * been set; an out_per_entry that is not finite and positive or is above max_out_per_entry; an in_per_unit that is not finite and
 * positive; set_track_device with n_samples outside 1 .. max_track_samples, a NULL array or as above; a format out of range; a flush
 * with a wanted stream that is not attached, has ended, has D = 0 or has no rows.  wc_warp_stream_create returns NULL, the text in
 * wc_last_error, for a plan the converter refuses, a count below 1, max_delay < 0, a max_out_per_entry that is not finite and
 * positive, a track_format out of range, or a max_out_per_push or packed output that leaves 31 bits; byte counts are formed in
 * 64-bit.
 *
 * A push is stream-ordered on the caller's stream (wc_set_stream) and only enqueues: one asynchronous copy of the records out of
 * the handle's staging and at most two launches -- the tiled group, and the plain group, which takes the pushes below segment_min
 * outputs (wc_warp_tiling) and every push on a plan without a tile, and keeps the carried entries.  It makes no device-to-host copy
 * and no synchronisation.  A handle is driven on one stream at a time. */
#ifndef WORLD_CLASS_WARP_STREAM_H
#define WORLD_CLASS_WARP_STREAM_H

#include "world_class_warp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* c(entries) at out_per_entry: a pure host function.  Refused: entries < 0, an out_per_entry that is not finite and positive, a
 * result of 2^62 and more */
long long wc_warp_stream_committed(long long entries, double out_per_entry);

int wc_warp_along_map_device(wc_vresampler *r, int n_utt, const void *d_x, int in_format, const int *x_length, const double *d_map,
                             const int *map_length, double out_per_entry, double in_per_unit, const int *out_length, void *d_y,
                             int out_format);

typedef struct wc_warp_stream wc_warp_stream;
wc_warp_stream *wc_warp_stream_create(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, double beta,
                                      int phase_bits, int degree, int n_streams, int n_tracks, int max_track_samples, int track_format,
                                      int max_entries_per_push, int max_delay, double max_out_per_entry);
void wc_warp_stream_destroy(wc_warp_stream *h);
int wc_warp_stream_set_track_device(wc_warp_stream *h, int track, int n_samples, const void *d_x);
int wc_warp_stream_reset(wc_warp_stream *h, int stream, int track, int delay, double out_per_entry, double in_per_unit);
int wc_warp_stream_max_out_per_push(const wc_warp_stream *h);
int wc_warp_stream_max_out_per_flush(const wc_warp_stream *h);
int wc_warp_stream_push_device(wc_warp_stream *h, const int *n_rows, const double *d_map, void *d_y, int out_format, int *samples_out);
int wc_warp_stream_flush_device(wc_warp_stream *h, const int *want, const double *d_tail, void *d_y, int out_format, int *samples_out);
/* rows received / map entries consumed / outputs committed so far; -1 for a bad index */
long long wc_warp_stream_rows_received(const wc_warp_stream *h, int stream);
long long wc_warp_stream_entries_consumed(const wc_warp_stream *h, int stream);
long long wc_warp_stream_samples_committed(const wc_warp_stream *h, int stream);
int wc_warp_stream_get_delay(const wc_warp_stream *h, int stream); /* -1: bad index */
int wc_warp_stream_track_length(const wc_warp_stream *h, int track);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_WARP_STREAM_H */
