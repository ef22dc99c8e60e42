/* ---- Alignment streams: a live voice followed row by row through a known track (extension) ----
 *
 * Included by world_class_stream.h; kept in a file of its own, with a binding table of its own in the Python mirror
 * (world_class_amd/stream.py: ALIGN_STREAM_SIGNATURES), beside the symbols of that header.
 *
 * The streaming form of wc_align_features_ex_device (world_class_io.h) at step_pattern 0, band 0 and WC_ALIGN_OPEN_END.  A path is
 * known only when both utterances have ended, but the POSITION is not: the cost and j_last that the whole call reports for the first
 * i + 1 rows of A depend only on D(i, .), and D(i, .) depends only on D(i - 1, .) and d(i, .).  So a handle keeps one row of D per
 * stream, and every pushed row gets "where in the track am I, at what cost" when it arrives: a d_position_b for
 * wc_morph_parameters_device (whose positions need not be monotone), a target for wc_morph_stream_set_speeds.
 *
 * A handle owns n_tracks track slots and n_streams streams.  Rows have dims doubles; only the coefficients dim_begin <= c < dim_end
 * are compared; both are fixed at create.
 *
 * Track.  wc_align_stream_set_track_device(h, track, m, d_feat_b) copies m rows (1 <= m <= max_track_frames) into the slot.  It is
 * stream-ordered; the caller may free its array once the call has been enqueued and the stream has been synchronised, as for any
 * other input.  Many streams may follow one track.  It is refused while a stream that has received rows is attached to the slot.
 *
 * Stream.  wc_align_stream_reset(h, stream, track, flags) attaches the stream to a track that has been set; flags is 0 or
 * WC_ALIGN_OPEN_BEGIN (world_class_io.h); the stream's row count returns to zero.  A stream that was never reset takes no rows.
 *
 * Push.  wc_align_stream_push_device(h, n_rows, d_feat_a, d_position, d_cost): n_rows[u] is a host array with
 * 0 <= n_rows[u] <= max_rows_per_push; the rows are packed stream by stream, as everywhere; the two outputs are packed the same way,
 * one double each per pushed row.
 *
 * The rule.  Let i be the index of the pushed row in its stream since the reset and m the track's length.  Row i of D is the row of
 * wc_align_features_ex_device at step_pattern 0 and band 0:
 *   d(i, j) has that call's exact rounding: ascending c from 0.0; difference, product and sum rounded apart; correctly rounded root.
 *   D(0, 0) = d(0, 0); under WC_ALIGN_OPEN_BEGIN D(0, j) = d(0, j) for every j.
 *   Otherwise D(i, j) = d(i, j) + best of Dd = D(i - 1, j - 1), Du = D(i - 1, j), Dl = D(i, j - 1), chosen by exactly that call's three
 *   comparisons: the diagonal if Dd <= Du && Dd <= Dl, else up if Du <= Dl, else left.  A predecessor outside the matrix counts as
 *   +inf.  (Comparisons, not fmin: they fix what NaN does.)
 *   Then the open-end scan of row i runs by ascending j from best = +inf, and j is taken when D(i, j) < best:
 *   d_cost = D(i, j*) and d_position = (double)j*; if no cell wins (NaN or +inf throughout) d_cost = D(i, m - 1) and d_position = NaN.
 * For every stream, every way the rows are cut into pushes and every row i, d_cost equals, bit for bit, d_cost of
 * wc_align_features_ex_device for the single pair (rows 0..i of A, the track) with step_pattern 0, band 0 and
 * flags = stream flags | WC_ALIGN_OPEN_END, and where that total is finite d_position equals span[1].
 * No stream's results depend on another stream's counts, tracks or flags.
 *
 * Refused with WC_ERR_INVALID on the host before anything is enqueued, every stream as it was: a bad index; a negative count or one
 * above max_rows_per_push; rows for a stream that is not attached; NULL arrays with rows to read or to write; set_track with m out of
 * range or on a slot in use as above; flags outside {0, WC_ALIGN_OPEN_BEGIN}; a reset onto an empty slot.  wc_align_stream_create
 * returns NULL for dims < 1, a coefficient window that is not 0 <= dim_begin < dim_end <= dims, a count below 1, and
 * n_streams x max_rows_per_push x max_track_frames above 2^28 cells (the whole call's cap).
 *
 * wc_align_stream_create allocates everything: the tracks, per stream max_rows_per_push x max_track_frames doubles of local costs
 * and two state rows of max_track_frames doubles, the descriptors and their page-locked staging.  wc_align_stream_destroy frees it.
 * A push only enqueues on the caller's stream (wc_set_stream): one asynchronous copy of the descriptors and two launches (the local
 * costs of the pushed rows by the whole call's cost kernel, then one wavefront per stream that has rows).  A handle is driven on one
 * stream at a time. */
#ifndef WORLD_CLASS_ALIGN_STREAM_H
#define WORLD_CLASS_ALIGN_STREAM_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wc_align_stream wc_align_stream;
wc_align_stream *wc_align_stream_create(int dims, int dim_begin, int dim_end, int n_streams, int n_tracks, int max_track_frames,
                                        int max_rows_per_push);
void wc_align_stream_destroy(wc_align_stream *h);
int wc_align_stream_set_track_device(wc_align_stream *h, int track, int m, const double *d_feat_b);
int wc_align_stream_reset(wc_align_stream *h, int stream, int track, int flags);
int wc_align_stream_push_device(wc_align_stream *h, const int *n_rows, const double *d_feat_a, double *d_position, double *d_cost);
/* rows the stream has received since its reset / rows of the track in the slot (0: empty); -1 for a bad index */
long long wc_align_stream_rows_received(const wc_align_stream *h, int stream);
int wc_align_stream_track_length(const wc_align_stream *h, int track);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_ALIGN_STREAM_H */
