/* ---- Model features: continuous log-F0, deltas and MLPG on the device (extension) ----
 *
 * The coded rows of world_class_codec.h (mel-cepstrum, band aperiodicity) and the F0 contour are what acoustic models are trained on,
 * after one more step that every recipe repeats on the host: log-F0 interpolated across the unvoiced gaps, a voiced/unvoiced flag,
 * delta and delta-delta features, one row per frame; and on the way back maximum-likelihood parameter generation (MLPG) over the
 * predicted statics and deltas, F0 gated by the flag, the row split again.  The three calls here do that on the device, so that
 * pipeline-coded -> pack -> (model) -> MLPG -> unpack -> coded synthesis never leaves it.  A header of its own with a binding table of
 * its own in the Python mirror (world_class_amd/features.py: FEATURES_SIGNATURES); tests/features_rule.py states THE rule in numpy.
 *
 * Layout.  A packed batch as everywhere in world_class_c.h: n_utt utterances of lengths[u] frames (a host array), device arrays packed
 * in utterance order.  The dimensions are plain integers: nd columns of d_coded_sp per frame, n_ap columns of d_coded_ap per frame
 * (n_ap may be 0, d_coded_ap NULL then), orders in {1, 2, 3}: statics; statics and deltas; statics, deltas and delta-deltas.  A row:
 *   mgc   order k of coefficient c   at column k * nd + c
 *   lf0   order k                    at column orders * nd + k
 *   vuv   (no deltas)                at column orders * (nd + 1)
 *   bap   order k of band b          at column orders * (nd + 1) + 1 + k * n_ap + b
 * width = orders * (nd + 1 + n_ap) + 1.  Rows are double (WC_FEAT_F64) or float (WC_FEAT_F32): a float is the (float) of the double
 * the rule gives, a float input is widened exactly.
 *
 * THE rule of pack, per utterance of n frames (nothing crosses an utterance boundary; every operation in double, rounded on its
 * own, no fma):
 *   frame i is voiced iff 0 < f0[i] <= DBL_MAX (NaN, negatives, 0 and +inf are unvoiced); vuv = 1.0 or 0.0; l(i) = log(f0[i]).
 *   Continuous lf0: with no voiced frame every frame gets lf0_fill.  Otherwise, L(i) the greatest voiced index <= i and R(i) the
 *   least voiced index >= i: a voiced frame gets l(i); a frame before the first voiced frame l(first), one after the last l(last);
 *   a frame in between (1 - a) * l(L) + a * l(R) with a = (double)(i - L) / (double)(R - L).
 *   Deltas of a static column x (a coded coefficient as it is, the continuous lf0, a band), a neighbour outside the utterance
 *   counting as 0.0 (np.correlate(mode="same")):
 *     D x(t)  = 0.5 * (x(t+1) - x(t-1))
 *     DD x(t) = (x(t-1) + x(t+1)) - 2.0 * x(t)
 *   Values that are not finite travel through this arithmetic as they are.
 *
 * THE rule of MLPG, per utterance and static column (mgc coefficient, lf0, band): one system of size n.  p_k(t) = 1.0 / var_k(t) for
 * the orders k = 0, 1, 2 (p_2 = 0 with orders == 2), q_k(t) = p_k(t) == 0 ? 0 : p_k(t) * mean_k(t); outside [0, n) p and q are 0.
 *   a0(t) = (p0(t) + 0.25 * (p1(t-1) + p1(t+1))) + ((p2(t-1) + p2(t+1)) + 4.0 * p2(t))
 *   a1(t) = -2.0 * (p2(t) + p2(t+1))          entry (t, t+1); 0 where t + 1 >= n
 *   a2(t) = p2(t+1) - 0.25 * p1(t+1)          entry (t, t+2); 0 where t + 2 >= n
 *   r(t)  = (q0(t) + 0.5 * (q1(t-1) - q1(t+1))) + ((q2(t-1) + q2(t+1)) - 2.0 * q2(t))
 * L D L^T without pivoting in ascending t, terms with an index below 0 left out:
 *   l2(t) = a2(t-2) / d(t-2)
 *   l1(t) = (a1(t-1) - (l2(t) * d(t-2)) * l1(t-1)) / d(t-1)
 *   d(t)  = (a0(t) - (l2(t) * l2(t)) * d(t-2)) - (l1(t) * l1(t)) * d(t-1)
 *   z(t)  = (r(t) - l2(t) * z(t-2)) - l1(t) * z(t-1)
 * and back in descending t, terms with an index at or beyond n left out:
 *   c(t)  = (z(t) / d(t) - l1(t+1) * c(t+1)) - l2(t+2) * c(t+2)
 * A variance of +inf is a precision of 0: that observation is dropped.  A variance that is NaN or <= 0, anywhere in the variances
 * one (utterance, static column) reads, makes that whole output column NaN and touches nothing else.  The vuv column is copied
 * through; its variance is not read.  The forward sweep parks l1, l2 and z / d, 3 doubles per frame and static column, in
 * per-device scratch that grows on demand and goes with wc_release_scratch().
 *
 * Every call only enqueues, on wc_set_stream's stream; lengths[u] == 0 and n_utt == 0 write nothing.  Refused with WC_ERR_INVALID
 * (the text in wc_last_error), before anything is enqueued or written: nd < 1, n_ap < 0, orders outside the call's set, a format
 * outside {0, 1}, a negative length or count, more than 2^32 - 1 frames in all, NULL lengths, an lf0_fill or vuv_threshold that is
 * NaN; and with frames to do: NULL arrays, exactly one of n_ap == 0 and d_coded_ap == NULL, an output that overlaps an input. */
#ifndef WORLD_CLASS_FEATURES_H
#define WORLD_CLASS_FEATURES_H

#include "world_class_c.h"

#define WC_FEAT_F64 0
#define WC_FEAT_F32 1

#ifdef __cplusplus
extern "C" {
#endif

/* orders * (nd + 1 + n_ap) + 1, or -1 for nd < 1, n_ap < 0, orders outside {1, 2, 3} or a width beyond 2^31 - 1 */
int wc_model_feature_width(int nd, int n_ap, int orders);

/* d_f0: one double per frame; d_coded_sp: nd doubles per frame; d_coded_ap: n_ap doubles per frame; d_rows: rows of out_format */
int wc_pack_model_features_device(int n_utt, const int *lengths, int nd, int n_ap, int orders, const double *d_f0,
                                  const double *d_coded_sp, const double *d_coded_ap, double lf0_fill, int out_format, void *d_rows);

/* orders in {2, 3}.  d_mean: one row of in_format per frame; d_var: the same format, one row per frame (var_per_frame == 1) or one
 * row for the whole batch (var_per_frame == 0: a model's global variances); d_static: rows of double in the orders == 1 layout */
int wc_mlpg_device(int n_utt, const int *lengths, int nd, int n_ap, int orders, int in_format, const void *d_mean, const void *d_var,
                   int var_per_frame, double *d_static);

/* The statics of mgc and bap as doubles, f0 = exp(lf0) where vuv > vuv_threshold and 0.0 elsewhere (a NaN vuv is unvoiced).  Each of
 * the three outputs may be NULL; together they are the arrays wc_synthesis_compute_coded_device takes */
int wc_unpack_model_features_device(long long n_frames, int nd, int n_ap, int orders, int in_format, const void *d_rows,
                                    double vuv_threshold, double *d_f0, double *d_coded_sp, double *d_coded_ap);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_FEATURES_H */
