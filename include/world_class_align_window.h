/* ---- Alignment streams inside a moving search window (extension) ----
 *
 * Included by world_class_stream.h just below world_class_align_stream.h; kept in a file of its own, with a binding table of its own
 * in the Python mirror (world_class_amd/stream.py: ALIGN_WINDOW_SIGNATURES).
 *
 * An alignment stream (world_class_align_stream.h) walks all m columns of its track for every pushed row.  A stream with a WINDOW
 * walks `width` columns around the place where the voice last was, so that a push costs what the voice can have moved and not what the
 * track is long, and with WC_ALIGN_WINDOW_MONOTONE its position never falls.
 *
 * wc_align_stream_set_window(h, stream, width, back, hop, flags) is host state only; nothing is enqueued.  It is allowed on a stream
 * that is attached (after wc_align_stream_reset) and has received no row yet.  width = 0 (with back = 0, hop = 1, flags = 0) removes
 * the window.  wc_align_stream_reset always returns a stream to no window, so every call sequence without set_window behaves
 * exactly as before.  wc_align_stream_get_window returns the settings; all 0 where no window is set, hop reported as 1.
 *
 * The rule, for a stream with window (width, back, hop, flags) on a track of m rows.  W = min(width, m); i is the row's index since the
 * reset; row i belongs to epoch e = i / hop (integer division), and every row of an epoch uses the same window of columns
 * [lo_e, lo_e + w_e).
 *   Epoch 0:      lo_0 = 0 and w_0 = W; under WC_ALIGN_OPEN_BEGIN w_0 = m: the first hop rows search the whole track (acquisition),
 *                 after that the window tracks.
 *   Epoch e >= 1: w_e = W.  Let p be the position written for row e * hop - 1.  If p is NaN, lo_e = lo_(e-1); otherwise
 *                 lo_e = min(max(lo_(e-1), (int)p - back), m - W).  The window's start never moves back.
 *   Inside the window d(i, j) and D(i, j) are exactly those of world_class_align_stream.h: the same rounding of d, the same row-0
 *   rule restricted to the window (D(0, 0) = d(0, 0); under WC_ALIGN_OPEN_BEGIN D(0, j) = d(0, j)), the same three comparisons.  A
 *   predecessor counts as +inf when it lies outside the matrix, outside row i's window (Dl), or outside row i - 1's window (Du, Dd).
 *   The scan of row i runs by ascending j over the row's window from best = +inf with the strict <.  Under
 *   WC_ALIGN_WINDOW_MONOTONE columns below q cannot win, where q is the last non-NaN position written for this stream, or 0 if there
 *   is none.  When no cell wins d_cost = D(i, lo_e + w_e - 1) and d_position = NaN.
 * Consequences:
 *   1. The results do not depend on how the rows are cut into pushes: epochs are counted on the absolute row index.
 *   2. With width >= m and no monotone flag every hop gives the unwindowed stream bit for bit.
 *   3. No stream's results depend on another stream, windowed or not.
 *   4. A stream whose position went NaN keeps its window; the caller resets it.
 *
 * Refused with WC_ERR_INVALID, the stream as it was: a bad stream index; a stream that was never reset; a stream with rows;
 * width < 0; back < 0; back >= width when width > 0; hop outside 1..64; flags outside {0, WC_ALIGN_WINDOW_MONOTONE}; the monotone flag
 * with width = 0 (and, as "removes the window" says, back != 0 or hop != 1 with width = 0).  get_window returns WC_ERR_INVALID for a
 * bad index or a NULL pointer.
 *
 * wc_align_stream_push_device, create and the allocation are as before, plus 16 bytes of device state per stream (the window of
 * the last row, its position and q).  Streams without a window go through the two launches of world_class_align_stream.h; the
 * streams with a window are left out of those and take one launch of their own (one wavefront per stream with rows: the local
 * costs of the window's columns, then the chain over them), behind the same single copy of the descriptors. */
#ifndef WORLD_CLASS_ALIGN_WINDOW_H
#define WORLD_CLASS_ALIGN_WINDOW_H

#ifdef __cplusplus
extern "C" {
#endif

#define WC_ALIGN_WINDOW_MONOTONE 1
int wc_align_stream_set_window(wc_align_stream *h, int stream, int width, int back, int hop, int flags);
int wc_align_stream_get_window(const wc_align_stream *h, int stream, int *width, int *back, int *hop, int *flags);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_ALIGN_WINDOW_H */
