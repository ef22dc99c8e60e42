/* ---- Feature streams: packed model rows from a live voice, a lag behind (extension) ----
 *
 * wc_pack_model_features_device (world_class_features.h) makes the rows a model reads -- continuous log-F0, the voiced/unvoiced
 * flag, deltas and delta-deltas -- from a whole utterance: the interpolation across an unvoiced gap is not causal, a frame inside a
 * gap needs the gap's far end.  A handle here holds n_streams concurrent streams; each takes rows of F0, coded envelope and coded
 * aperiodicity push by push, exactly the arrays and the packing wc_stream_push_coded_device writes, and emits, `lag` rows behind the
 * newest, the packed rows; a flush emits the last rows.  A header of its own with a binding table of its own in the Python mirror
 * (world_class_amd/feature_stream.py: FEATURE_STREAM_SIGNATURES); tests/feature_stream_rule.py states THE rule in numpy, as the
 * definition and as the recursion of the kernels.
 *
 * Dimensions, the row layout, S = nd + 1 + n_ap static columns, the width orders * S + 1, the formats and every arithmetic
 * expression are those of world_class_features.h; orders is 1, 2 or 3.
 *
 * THE rule.  A stream has a lag L and an lf0_fill, both given at its reset; its rows since the reset are numbered i = 0, 1, ...  A
 * row is one F0 value, nd coded envelope values and n_ap coded aperiodicity values.  P_i is what wc_pack_model_features_device gives
 * for the single utterance made of rows 0 .. i with that lf0_fill.
 *   Push.   Pushed row i with i >= L emits row i - L of P_i.  After T rows a stream that has not ended has emitted
 *           E(T) = max(T - L, 0) rows (wc_feature_stream_emitted: host arithmetic on counts alone); a push that takes it from T0 to
 *           T1 rows writes frames_out = E(T1) - E(T0) rows.
 *   Flush.  With n rows received the flush writes rows E(n) .. n - 1 of P_{n-1}: min(L, n) rows, the whole call's own last rows.
 *           The stream has then ended: rows are refused until the next reset.  A wanted stream with no rows flushes nothing and
 *           ends.
 *   Formats.  The output format is chosen per push and per flush, WC_FEAT_F64 or WC_FEAT_F32; a float is the (float) of the double.
 * Consequences:
 *   1. A stream's concatenated outputs do not depend on how its rows are cut into pushes, pushes of 0 rows included.
 *   2. No stream's outputs depend on another stream.
 *   3. Every emitted row is wc_pack_model_features_device's row on its prefix, bit for bit.  A frame in an unvoiced run whose far end
 *      lies within the prefix is interpolated; a frame whose far end lies beyond the prefix holds the last voiced log-F0, exactly as
 *      the whole call treats a trailing run; before the first voiced row of the prefix every frame is lf0_fill.
 *   4. With L >= n nothing is emitted before the flush, and the flush is the whole call, bit for bit.
 *   5. With L = 0 every row emits itself from the prefix that ends at it; for orders > 1 its successor counts as 0.0, as the whole
 *      call's last row does.
 *   6. A reset forgets everything: nothing from before a reset can show after it.
 *   7. A stream with L >= 1 whose unvoiced runs are all shorter than L (the leading run counts, the trailing run does not) emits,
 *      pushes and flush concatenated, the whole call's rows bit for bit: row t of P_{t+L} reads the continuous log-F0 of frames
 *      t - 1, t and t + 1, and each of those is final once its next voiced frame, if any, lies at or before t + L.
 *   8. The lag is not free: a longer run costs a step in log-F0.  The frames of the run that lie more than L before its far end hold
 *      the last voiced log-F0 (lf0_fill in a leading run); from the frame L before the far end on they are interpolated, so the step
 *      falls at that frame, and that frame's deltas are the deltas of its own prefix.  Its size is the interpolated value there less
 *      the held one: (g - L) / g of the difference of the two logs for a run whose far end lies g frames behind its last voiced
 *      frame.  At 5 ms frames L = 64 covers pauses of 315 ms.
 *
 * Why bounded state suffices.  To form row t of P_j with j = t + L a stream needs the static rows of frames t - 1, t and t + 1, and
 * for each of those frames the greatest voiced index at or before it, which may lie arbitrarily far back, and the least voiced index
 * at or after it but not beyond j, which lies within L + 2 rows.  So a stream carries a ring of its last rows (the log of a voiced
 * F0, taken once on arrival, or a NaN for an unvoiced one; the nd coded envelope values; the n_ap coded aperiodicity values) and one
 * carried record: the index and the log of the last voiced row below the window the next call scans, or "none".  The ring has
 * exactly max_lag + max_rows_per_push + 1 rows: a push from T0 to T1 rows at lag L reads rows T0 - L - 1 .. T1 - 1, the frame before
 * its first emitted frame up to its newest row, and writes rows T0 .. T1 - 1; a flush reads rows n - L - 1 .. n - 1.
 *
 * Layout of a call.  n_rows and want are host arrays of n_streams ints.  d_f0 (one double per row), d_coded_sp (nd doubles per row)
 * and d_coded_ap (n_ap doubles per row; NULL exactly where n_ap is 0) hold stream u's rows at the sum of n_rows[< u] rows: the
 * analysis push's frames_out is this push's n_rows, unchanged.  d_rows is packed stream by stream by frames_out[u], which is filled
 * before the call returns and is 0 for idle and unwanted streams; d_rows holds n_streams x max_frames_per_push rows for a push and
 * n_streams x max_frames_per_flush rows for a flush.  Calls are stream-ordered on wc_set_stream's stream and only enqueue: one copy
 * of descriptors from page-locked staging and two kernels, no device-to-host copy and no synchronisation; a stream with no rows in
 * a push costs no wavefront.  create allocates everything, destroy releases it.
 *
 * Refused with WC_ERR_INVALID (NULL from create), the text in wc_last_error, on the host before anything is enqueued, every stream
 * as it was:
 *   create  shapes the model-feature calls refuse (nd < 1, n_ap < 0, a row width beyond 31 bits), orders outside {1, 2, 3},
 *           n_streams or max_rows_per_push below 1, max_lag < 0, a ring above 2^30 bytes (counted in 64 bits)
 *   any     a NULL handle, a bad stream index
 *   reset   a lag outside 0 .. max_lag, an lf0_fill that is NaN
 *   push    a count that is negative or above max_rows_per_push; rows for a stream that was never reset or has ended; NULL n_rows or
 *           frames_out; NULL arrays with rows to read or to write; exactly one of n_ap == 0 and d_coded_ap == NULL, with rows to
 *           read; a format outside {0, 1}; d_rows overlapping an input
 *   flush   NULL want or frames_out; a wanted stream that was never reset or has ended; NULL d_rows with frames to write; a format
 *           outside {0, 1} */
#ifndef WORLD_CLASS_FEATURE_STREAM_H
#define WORLD_CLASS_FEATURE_STREAM_H

#include "world_class_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* E(rows) = max(rows - lag, 0); -1 for a negative argument.  Pure host arithmetic */
long long wc_feature_stream_emitted(long long rows, int lag);

typedef struct wc_feature_stream wc_feature_stream;

wc_feature_stream *wc_feature_stream_create(int n_streams, int nd, int n_ap, int orders, int max_rows_per_push, int max_lag);
void wc_feature_stream_destroy(wc_feature_stream *h);

/* 0 <= lag <= max_lag; the stream's counts go to zero and it takes rows again */
int wc_feature_stream_reset(wc_feature_stream *h, int stream, int lag, double lf0_fill);

int wc_feature_stream_push_device(wc_feature_stream *h, const int *n_rows, const double *d_f0, const double *d_coded_sp,
                                  const double *d_coded_ap, int out_format, void *d_rows, int *frames_out);
/* want[u] != 0: stream u writes its last min(lag, rows) rows and ends */
int wc_feature_stream_flush_device(wc_feature_stream *h, const int *want, int out_format, void *d_rows, int *frames_out);

int wc_feature_stream_max_frames_per_push(const wc_feature_stream *h);  /* max_rows_per_push */
int wc_feature_stream_max_frames_per_flush(const wc_feature_stream *h); /* max_lag */

long long wc_feature_stream_rows_received(const wc_feature_stream *h, int stream);  /* -1: bad index */
long long wc_feature_stream_frames_emitted(const wc_feature_stream *h, int stream); /* -1: bad index */
int wc_feature_stream_get_lag(const wc_feature_stream *h, int stream);              /* -1: bad index or never reset */

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_FEATURE_STREAM_H */
