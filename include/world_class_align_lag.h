/* ---- Alignment streams: settled positions from a lagged backtrack (extension) ----
 *
 * Included by world_class_stream.h just below world_class_align_window.h; kept in a file of its own, with a binding table of its own
 * in the Python mirror (world_class_amd/stream.py: ALIGN_LAG_SIGNATURES).
 *
 * The position of an alignment stream (world_class_align_stream.h) is the open-end scan of one row of D: the end the best path
 * would have if the voice stopped at this row.  It is no point on a path; it jitters and it jumps between places that sound alike.
 * The FINAL path is known only when the voice has ended, but the path behind the newest row is known now, and a few rows back it
 * hardly changes any more.  A stream with a LAG of L rows keeps the choices of its last rows, walks back from the newest row's
 * position and reports where the row L frames ago lies on that path: the half-integer centre of the path's cells in that row, which
 * is what d_b_on_a of wc_align_features_ex_device (world_class_io.h) holds and what wc_retime_parameters_device and
 * wc_morph_parameters_device consume.
 *
 * wc_align_stream_reserve_lag(h, max_lag) allocates the choices: one byte per cell, max_lag + max_rows_per_push rows of
 * max_track_frames bytes per stream (and one int per stream).  Once per handle, max_lag >= 1; WC_ERR_INVALID above 2^30 bytes
 * (counted in 64-bit on the host before the device is touched).  wc_align_stream_create is as before: a handle that never reserves
 * allocates no ring.
 *
 * wc_align_stream_set_lag(h, stream, lag) is host state only, under the conditions of wc_align_stream_set_window: the stream is
 * attached and has no rows yet.  0 <= lag <= max_lag (0 without a reservation).  lag = 0 removes the lag, and so does every
 * wc_align_stream_reset: every call sequence without set_lag behaves exactly as before.  wc_align_stream_get_lag returns the lag, -1
 * for a bad index.  Lag and window are independent: a stream may have either, both or neither.
 *
 * The rule.  While a stream has lag L > 0, every cell (i, j) it computes -- with or without a window, through either push call --
 * records its choice:
 *   start   row 0 at j = 0, or any j of row 0 under WC_ALIGN_OPEN_BEGIN;
 *   diagonal, up or left: the branch that the three comparisons of world_class_align_stream.h take.
 * The path P(i) of row i (the index since the reset) starts at (i, j*_i), where j*_i is the position written for row i (under
 * WC_ALIGN_WINDOW_MONOTONE the floored scan's winner), and follows the choices until a start: diagonal to (r - 1, j - 1), up to
 * (r - 1, j), left to (r, j - 1).  For pushed row i let t = max(i - L, 0):
 *   d_settled = (jmin + jmax) * 0.5 over the cells of P(i) in row t; NaN when row i's position is NaN.
 * So the first L rows report where row 0 lies as seen from the newest row, and from then on every row reports row i - L; no sentinel
 * is needed.  A stream with lag 0 gets d_settled = d_position.
 *
 * wc_align_stream_push_settled_device(h, n_rows, d_feat_a, d_position, d_cost, d_settled) is wc_align_stream_push_device with one
 * more output, packed like the other two; d_position and d_cost are those of wc_align_stream_push_device bit for bit.
 * wc_align_stream_push_device itself still works on a stream with a lag: it records the choices and writes no settled value; the
 * two may be interleaved.
 *
 * wc_align_stream_tail_device(h, want, d_tail) is the flush: when the voice ends, the last L rows get their positions.  want is a
 * host array of n_streams ints.  For every stream with want[u] != 0, with n rows received and K = min(L + 1, n), it writes K doubles:
 * the same half-integer for rows n - K .. n - 1 of P(n - 1), ascending; all NaN where row n - 1's position was NaN.  The output is
 * packed stream by stream in stream order; the host knows K from wc_align_stream_rows_received and wc_align_stream_get_lag.  It
 * changes no state and may be called at any time.
 *
 * Consequences:
 *   1. The results do not depend on how the rows are cut into pushes.
 *   2. No stream's results depend on another stream.
 *   3. For an unwindowed stream and every row i whose total is finite, d_settled equals, bit for bit, d_b_on_a[t] of
 *      wc_align_features_ex_device for the single pair (rows 0..i, the track) with step_pattern 0, band 0 and
 *      flags = stream flags | WC_ALIGN_OPEN_END; the tail equals the last K entries of that call's d_b_on_a on all rows.
 *   4. A window of width >= m without the monotone flag gives the unwindowed stream's settled values.
 *   5. A path from a winning cell, whose D is finite, visits cells with finite D only: a cell's D is its cost plus the chosen
 *      predecessor, and the comparisons choose a finite predecessor where the sum is finite.  So a path never reads a choice from
 *      outside a row's window or from before the reset: stale choices cannot show.
 * The settled positions of consecutive rows come from different paths; they are NOT promised to be monotone.
 *
 * Refused with WC_ERR_INVALID on the host before anything is enqueued, every stream as it was: reserve_lag twice, with max_lag < 1
 * or above 2^30 bytes; set_lag with a bad index, on a stream that was never reset or has rows, with lag < 0 or lag > max_lag
 * (any lag > 0 without a reservation); push_settled_device as push_device, and with a NULL d_settled and rows to write;
 * tail_device with a NULL want or d_tail, or with a wanted stream that has no lag or no rows.
 *
 * A push costs what it did, plus: for a stream with a lag one byte stored per computed cell by the two row kernels; for a settled
 * push one more launch (one wavefront per stream with rows, lane l walks back from pushed rows l, l + 64, ..) and 40 more bytes of
 * descriptor per stream with rows, inside the same single copy.  A tail is one copy of descriptors and one launch. */
#ifndef WORLD_CLASS_ALIGN_LAG_H
#define WORLD_CLASS_ALIGN_LAG_H

#ifdef __cplusplus
extern "C" {
#endif

int wc_align_stream_reserve_lag(wc_align_stream *h, int max_lag);
int wc_align_stream_set_lag(wc_align_stream *h, int stream, int lag);
int wc_align_stream_get_lag(const wc_align_stream *h, int stream); /* -1: bad index */
int wc_align_stream_push_settled_device(wc_align_stream *h, const int *n_rows, const double *d_feat_a, double *d_position, double *d_cost,
                                        double *d_settled);
int wc_align_stream_tail_device(wc_align_stream *h, const int *want, double *d_tail);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_ALIGN_LAG_H */
