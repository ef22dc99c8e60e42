/* ---- Track-morph streams: a live voice morphed with a resident track at positions read on the device (extension) ----
 *
 * Included by world_class_stream.h just below world_class_align_lag.h; kept in a file of its own, with a binding table of its own
 * in the Python mirror (world_class_amd/stream.py: TRACK_MORPH_SIGNATURES).
 *
 * An alignment stream (world_class_align_stream.h, world_class_align_lag.h) tells a live voice where it is in a track: for every
 * pushed row one double in device memory, d_settled, the half-integer position wc_morph_parameters_device (world_class_io.h) takes as
 * d_position_b.  This handle consumes those doubles where they are.  It sits IN FRONT of a synthesis stream as wc_morph_stream does
 * (world_class_stream.h): a push takes rows of the live voice (voice A) for every stream and one position per row, and writes the
 * frames they now allow as full rows (F0, sp row, ap row of fft_size/2+1) into the caller's buffers; voice B is a track that is
 * resident in the handle.  Nothing of wc_morph_stream, wc_align_stream or wc_synth_stream is touched.
 *
 * Tracks.  wc_track_morph_create allocates n_tracks slots of max_track_frames full rows.  wc_track_morph_set_track_device(h, track,
 * m, d_f0_b, d_sp_b, d_ap_b) copies m rows (1 <= m <= max_track_frames) into a slot, stream-ordered.  Many streams may share a slot;
 * the call is refused while a stream that has received rows is attached to it.  wc_track_morph_track_length: m, 0 for a slot that
 * has not been set, -1 for a bad index.
 *
 * wc_track_morph_reset(h, stream, track, delay) attaches the stream to a slot that has been set, with a delay D, 0 <= D <= max_delay:
 * the lag of the alignment stream whose settled positions it will be given (0: positions of the rows themselves).  Counts go to
 * zero, the weight and the F0 weight to 0, both ratios to 0 (none).  wc_track_morph_set_weight and wc_track_morph_set_ratios are
 * host-side settings that take effect at the next push or flush, with the refusals of wc_morph_stream_set_weight /
 * wc_morph_stream_set_ratios.
 *
 * The rule.  A push gives stream u n_a[u] rows of the live voice (a host array; the rows packed stream by stream in the three
 * arrays as for wc_synth_stream_push_device) and ONE DOUBLE PER PUSHED ROW in d_position_b, packed the same way: exactly d_settled
 * of wc_align_stream_push_settled_device (or d_position of wc_align_stream_push_device when D = 0) called with the same counts.
 * With i the index of a pushed row since the reset:
 *   i <  D   the row forms nothing and its entry is not read;
 *   i >= D   the row forms output frame t = i - D from A's row t and the track at the entry of row i.
 * So frames_out[u] = max(n + n_a[u] - D, 0) - max(n - D, 0), n the rows received before: host arithmetic on counts alone.  No host
 * code ever looks at a position; the kernel reads it.  The formed frames are packed by frames_out[u] (host array); the outputs hold
 * n_streams x max_frames_per_push rows.  Each frame takes the weight, F0 weight and ratios in effect at the call that forms it.
 *
 * The flush.  When the voice ends, its last min(D, n) rows still wait.  wc_track_morph_flush_device(h, want, d_tail, ..) takes
 * d_tail in the layout wc_align_stream_tail_device writes for the same want: K = min(D + 1, n) doubles per wanted stream, for rows
 * n - K .. n - 1, packed in stream order.  It forms frames max(n - D, 0) .. n - 1 from the last min(D, n) of those entries (when
 * n > D the first entry belongs to a frame a push has formed, and is skipped); frames_out[u] = min(D, n) for a wanted stream, 0 for
 * the others; the outputs hold n_streams x max_delay rows.  Afterwards the stream has ended: nothing waits and rows are refused
 * until the next reset.  A wanted stream with D = 0 or without rows is refused, as the tail call refuses it.
 *
 * Bit identity.  Every formed frame t is, bit for bit, frame t of wc_morph_parameters_device for ONE pair (all rows of A pushed so
 * far, the track) at d_position_a[t] = (double)t, d_position_b[t] = the entry consumed, and the weight, F0 weight and ratios of that
 * call -- including that call's end clamp of the position to [0, m - 1] and its frame that is NaN throughout (F0 and both rows) for
 * a position that is not finite.  A's side is that call's arithmetic at a whole position, so an inf or NaN inside a row of A does
 * what it does there.  Positions may fall, jump or repeat.  No stream's frames depend on another stream or on how the rows are cut
 * into pushes.
 *
 * The ring.  Rows of A that have been pushed but not yet formed wait in a ring per stream, at most D rows of F0 and both rows.
 * Every row that is ever kept takes the next number of a sequence per stream and sits in slot number % cap, cap = max_delay +
 * min(max_delay, max_frames_per_push) (wc_morph_stream's numbering): a push never writes a slot the state before it needs, so a
 * push that fails on the device with a HIP error leaves the host state and the kept rows of the last good push.  max_delay = 0
 * allocates no ring.  wc_track_morph_create allocates everything: the tracks, the ring, the device array and the two page-locked
 * staging buffers of the records.  wc_track_morph_destroy releases them.
 *
 * Refused with WC_ERR_INVALID on the host before anything is enqueued, every stream, setting and kept row as it was: a bad stream
 * or track index; a count that is negative or above max_frames_per_push; rows for a stream that is not attached or has ended; NULL
 * arrays with rows to read, positions to read or frames to write; a NULL n_a, want or frames_out; a delay out of range; a reset
 * onto a slot that has not been set; set_track_device with m out of range, a NULL array or as above; a weight or F0 weight that is
 * not finite; a ratio that is neither 0 nor finite and >= 2.0 / fft_size; a flush with a wanted stream that is not attached, has
 * ended, has D = 0 or has no rows.  wc_track_morph_create returns NULL for fft_size outside 512 / 1024 / 2048 / 4096, fs <= 0, a
 * count below 1 or max_delay < 0; byte counts are formed in 64-bit.
 *
 * A push is stream-ordered on the caller's stream (wc_set_stream) and only enqueues: one asynchronous copy of the records out of
 * the handle's staging (48 bytes per stream, 16 per formed frame, 8 per kept row) and one launch that forms the frames and keeps
 * the rows (the variant without shared memory while no stream that forms frames has a ratio).  It makes no device-to-host copy and
 * no synchronisation.  A handle is driven on one stream at a time. */
#ifndef WORLD_CLASS_TRACK_MORPH_H
#define WORLD_CLASS_TRACK_MORPH_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wc_track_morph wc_track_morph;
wc_track_morph *wc_track_morph_create(int fs, int fft_size, int n_streams, int n_tracks, int max_track_frames, int max_frames_per_push,
                                      int max_delay);
void wc_track_morph_destroy(wc_track_morph *h);
int wc_track_morph_set_track_device(wc_track_morph *h, int track, int m, const double *d_f0_b, const double *d_sp_b, const double *d_ap_b);
int wc_track_morph_reset(wc_track_morph *h, int stream, int track, int delay);
int wc_track_morph_set_weight(wc_track_morph *h, int stream, double weight, double f0_weight);
int wc_track_morph_set_ratios(wc_track_morph *h, int stream, double ratio_a, double ratio_b);
int wc_track_morph_push_device(wc_track_morph *h, const int *n_a, const double *d_f0_a, const double *d_sp_a, const double *d_ap_a,
                               const double *d_position_b, double *d_f0_out, double *d_sp_out, double *d_ap_out, int *frames_out);
int wc_track_morph_flush_device(wc_track_morph *h, const int *want, const double *d_tail,
                                double *d_f0_out, double *d_sp_out, double *d_ap_out, int *frames_out);
/* rows of A received / frames formed so far; -1 for a bad index */
long long wc_track_morph_frames_received(const wc_track_morph *h, int stream);
long long wc_track_morph_frames_formed(const wc_track_morph *h, int stream);
int wc_track_morph_pending(const wc_track_morph *h, int stream); /* rows of A kept, not yet formed; -1 for a bad index */
int wc_track_morph_get_delay(const wc_track_morph *h, int stream); /* -1: bad index */
int wc_track_morph_track_length(const wc_track_morph *h, int track);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_TRACK_MORPH_H */
