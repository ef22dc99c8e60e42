/* ---- MLPG streams: settled statics from a lagged back-substitution (extension) ----
 *
 * wc_mlpg_device (world_class_features.h) solves one banded system per utterance and static column, so a model that predicts means
 * and variances frame by frame could hand nothing to wc_synth_stream_push_coded_device before its utterance had ended.  A handle here
 * holds n_streams concurrent streams; each takes rows of predicted means and variances push by push and emits, `lag` rows behind the
 * newest, the static rows that wc_unpack_model_features_device(orders = 1) and then the synthesis stream take; a flush emits the last
 * rows.  A header of its own with a binding table of its own in the Python mirror (world_class_amd/mlpg_stream.py:
 * MLPG_STREAM_SIGNATURES); tests/mlpg_stream_rule.py states THE rule in numpy, as the definition and as the recursion of the kernels.
 *
 * Dimensions, the row layout, S = nd + 1 + n_ap static columns, the formats and every arithmetic expression are those of
 * world_class_features.h; orders is 2 or 3.  A mean row and a variance row have orders * S + 1 columns, an emitted row S + 1 doubles
 * (the orders == 1 layout).
 *
 * THE rule.  A stream has a lag L, given at its reset; its rows since the reset are numbered i = 0, 1, ...  C_i is what
 * wc_mlpg_device gives for the single utterance made of rows 0 .. i with var_per_frame == 1.
 *   Push.   Pushed row i with i >= L emits static row i - L of C_i.  After T rows a stream that has not ended has emitted
 *           E(T) = max(T - L, 0) frames (wc_mlpg_stream_emitted: host arithmetic on counts alone); a push that takes it from T0 to T1
 *           rows writes frames_out = E(T1) - E(T0) rows.
 *   Flush.  With n rows received the flush writes rows E(n) .. n - 1 of C_{n-1}: min(L, n) rows, the whole call's own last rows.
 *           The stream has then ended: rows are refused until the next reset.  A wanted stream with no rows (or with lag 0) flushes
 *           nothing and ends.
 *   vuv.    The vuv column of an emitted row is the mean row's vuv of that frame, widened exactly; its variance is not read.
 *   Variances.  var_per_frame == 0 in a push means one variance row for every row of every stream in that push: the per-frame rule on
 *           that row repeated (the same quotients 1.0 / v either way, so the same row at every push is
 *           wc_mlpg_device(var_per_frame = 0) on the prefix, bit for bit).  A variance that is NaN or <= 0 in row j of a static column
 *           makes every frame of that column emitted by rows >= j NaN, the flush included; it touches no other column, no other stream
 *           and nothing already emitted.  A variance of +inf drops that observation.  A NaN is a NaN, whatever its payload.
 * Consequences:
 *   1. A stream's concatenated outputs do not depend on how its rows are cut into pushes, pushes of 0 rows included.
 *   2. No stream's outputs depend on another stream.
 *   3. Each emitted row is wc_mlpg_device's on its prefix, bit for bit.
 *   4. With L >= n nothing is emitted before the flush, and the flush is wc_mlpg_device on the whole utterance, bit for bit.
 *   5. With L = 0 every row emits itself from the prefix that ends at it.
 *   6. A reset forgets everything: nothing from before a reset can show after it.
 * The frame a row emits converges geometrically in L to the whole utterance's (DESIGN.md section 10 has the table: at variances
 * (1, 0.1, 0.05) 32 rows of lag are within 2e-5 of max|c| of the whole call's answer, 64 rows within 3e-10).
 *
 * Why bounded state suffices.  In the prefix of T rows a0(t), r(t), a1(t), a2(t), and with them l1, l2, d and z, are those of any
 * longer utterance for the rows t <= T - 2: a0 and r of row t read the precisions of row t + 1, and a2(t) is read by row t + 2 alone.
 * Row T - 1 has its final l1 and l2; its d and z are provisional, formed with the successor's p and q as literal zeros exactly as the
 * whole call forms its last row.  So a stream carries, per static column, what the whole call's sweep carries from one row to the
 * next, taken before its newest row is finished, the converted precisions and weighted means of its last two rows, and a ring of
 * parked l1, l2, final z / d, end-row quotient z_end / d_end and vuv over its last max_lag + max_rows_per_push + 1 rows.  A push
 * finishes the carried row, walks its rows (forward kernel), and for every pushed row that emits makes L + 1 steps of
 * back-substitution down the ring from that row's end quotient (back kernel); the flush is one such walk from row n - 1 that writes
 * every row it passes.
 *
 * Layout of a call.  n_rows and want are host arrays of n_streams ints.  d_mean holds stream u's rows at the sum of n_rows[< u] rows,
 * in in_format (an argument of each push; a float is widened exactly); d_var is packed the same way, or is one row when
 * var_per_frame == 0.  d_static is packed stream by stream by frames_out[u], which is filled before the call returns and is 0 for
 * idle and unwanted streams; d_static holds n_streams x max_frames_per_push rows for a push and n_streams x max_frames_per_flush rows
 * for a flush.  Calls are stream-ordered on wc_set_stream's stream and only enqueue: one copy of descriptors from page-locked
 * staging and two kernels for a push, one kernel for a flush, no device-to-host copy and no synchronisation; a stream with no rows
 * in a push costs no wavefront.  create allocates everything, destroy releases it.
 *
 * Refused with WC_ERR_INVALID (NULL from create), the text in wc_last_error, on the host before anything is enqueued, every stream
 * as it was:
 *   create  shapes the model-feature calls refuse (nd < 1, n_ap < 0, a row width beyond 31 bits), orders outside {2, 3}, n_streams or
 *           max_rows_per_push below 1, max_lag < 0, a ring above 2^30 bytes (counted in 64 bits)
 *   any     a NULL handle, a bad stream index
 *   reset   a lag outside 0 .. max_lag
 *   push    a count that is negative or above max_rows_per_push; rows for a stream that was never reset or has ended; NULL n_rows or
 *           frames_out; NULL arrays with rows to read or frames to write; a format or var_per_frame out of range; d_static
 *           overlapping an input
 *   flush   NULL want or frames_out; a wanted stream that was never reset or has ended; NULL d_static with frames to write */
#ifndef WORLD_CLASS_MLPG_STREAM_H
#define WORLD_CLASS_MLPG_STREAM_H

#include "world_class_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* E(rows) = max(rows - lag, 0); -1 for a negative argument.  Pure host arithmetic */
long long wc_mlpg_stream_emitted(long long rows, int lag);

typedef struct wc_mlpg_stream wc_mlpg_stream;

wc_mlpg_stream *wc_mlpg_stream_create(int n_streams, int nd, int n_ap, int orders, int max_rows_per_push, int max_lag);
void wc_mlpg_stream_destroy(wc_mlpg_stream *h);

/* 0 <= lag <= max_lag; the stream's counts go to zero and it takes rows again */
int wc_mlpg_stream_reset(wc_mlpg_stream *h, int stream, int lag);

int wc_mlpg_stream_push_device(wc_mlpg_stream *h, const int *n_rows, int in_format, const void *d_mean, const void *d_var,
                               int var_per_frame, double *d_static, int *frames_out);
/* want[u] != 0: stream u writes its last min(lag, rows) rows and ends */
int wc_mlpg_stream_flush_device(wc_mlpg_stream *h, const int *want, double *d_static, int *frames_out);

int wc_mlpg_stream_max_frames_per_push(const wc_mlpg_stream *h);  /* max_rows_per_push */
int wc_mlpg_stream_max_frames_per_flush(const wc_mlpg_stream *h); /* max_lag */

long long wc_mlpg_stream_rows_received(const wc_mlpg_stream *h, int stream);  /* -1: bad index */
long long wc_mlpg_stream_frames_emitted(const wc_mlpg_stream *h, int stream); /* -1: bad index */
int wc_mlpg_stream_get_lag(const wc_mlpg_stream *h, int stream);              /* -1: bad index or never reset */

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_MLPG_STREAM_H */
