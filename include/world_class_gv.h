/* ---- Global-variance parameter generation behind MLPG on the device (extension) ----
 *
 * wc_mlpg_device (world_class_features.h) gives the maximum-likelihood trajectory of every static column, and that trajectory is
 * over-smoothed: its variance over the utterance is a fraction of natural speech's.  The companion of MLPG in every HTS-lineage system
 * is parameter generation with a global-variance (GV) term (Toda & Tokuda 2007): a variance-scaling start, then a few Newton-like
 * ascent steps on  w_ml * omega * log-likelihood + w_gv * GV likelihood,  with a per-frame switch that keeps silence out of the
 * statistics.  The two calls here do that on the device behind wc_mlpg_device, so that pack -> (model) -> MLPG -> GV -> unpack -> coded
 * synthesis never leaves it.  A header of its own with a binding table of its own in the Python mirror (world_class_amd/gv.py:
 * GV_SIGNATURES); tests/gv_rule.py states THE rule in numpy on top of tests/features_rule.py.
 *
 * Layout: that of world_class_features.h.  A packed batch of n_utt utterances of lengths[u] frames (a host array); nd, n_ap, orders in
 * {2, 3}, in_format, d_mean, d_var and var_per_frame exactly as wc_mlpg_device takes them; d_static: rows of nd + 2 + n_ap doubles (the
 * orders == 1 layout, vuv at column nd + 1).  The S = nd + 1 + n_ap static columns stand in the order mgc, lf0, bands: d_gv_mean,
 * d_gv_var, d_mean_out and d_var_out are indexed by that order (the vuv column has no entry).  d_mask: one byte per frame of the packed
 * batch, a frame counts ("is masked") where its byte is not 0; NULL: every frame counts.
 *
 * THE rule (every operation in double, rounded on its own, no fma).
 *
 * The sum.  SUM_t x(t) over one utterance has a fixed order: lane l of 64 adds x(l), x(l + 64), ... in ascending t to a partial that
 * starts at +0.0, a term that is not counted adds +0.0; then for off = 32, 16, 8, 4, 2, 1 every partial becomes p[l] + p[l ^ off].
 *
 * Per (utterance of n frames, static column), m(t) the mask, N = (double) the count of masked frames, a0, a1, a2, r the banded system
 * of the MLPG rule of world_class_features.h on the same means and variances:
 *   stat(c):  mean = SUM m·c / N,  d(t) = m(t) ? c(t) - mean : 0,  v = SUM d·d / N
 *   (A c)(t) = ((a2(t-2) * c(t-2) + a1(t-1) * c(t-1)) + a0(t) * c(t)) + (a1(t) * c(t+1) + a2(t) * c(t+2))
 *              a term with an index outside [0, n) counts as +0.0
 *   pv = 1.0 / gv_var,  omega = w_ml / (double)(orders * n)
 * wc_gv_stats_device writes mean and v of stat(c); N == 0 gives NaN by 0.0 / 0.0, for an utterance of length 0 as well.
 * wc_mlpg_gv_device, in this order:
 *   gv_var == +inf (a precision of 0: the column is switched off; its gv_mean is not looked at) leaves the column as it is;
 *   a gv_var that is NaN or <= 0, or a gv_mean that is NaN, <= 0 or +inf, makes the masked frames of that static column NaN in every
 *   utterance and touches nothing else;
 *   N < 2 leaves the column of this utterance as it is;
 *   (mean, d, v) = stat(c); a first v that is not > 0 leaves the column of this utterance as it is.
 * The start:
 *   ratio = sqrt(gv_mean / v)
 *   c(t) = ratio * d(t) + mean                         on masked frames
 * then for it = 1 ... max_iter, with step = step_init:
 *   (mean, d, v) = stat(c);  Ac = A c;  e = v - gv_mean
 *   J = omega * SUM_t c(t) * (r(t) - 0.5 * Ac(t)) - (0.5 * w_gv) * ((e * e) * pv)
 *   if it > 1:  if J < J_prev: step = step * 0.5;  if J > J_prev: step = step * 1.2          (a NaN J changes nothing)
 *   h(t) = omega * a0(t) + (w_gv * (2.0 / (N * N))) * (((N - 1.0) * pv) * e + (2.0 * pv) * (d(t) * d(t)))
 *   g(t) = (omega * (r(t) - Ac(t)) - ((w_gv * (2.0 / N)) * (pv * e)) * d(t)) / h(t)
 *   c(t) = c(t) + step * g(t)                          on masked frames;  J_prev = J
 * h is minus the diagonal of J's Hessian, g the Newton-like ascent direction; every g of one step is formed from the c before it.
 * max_iter == 0 is the closed-form variance-scaling post-filter alone: d_mean and d_var are not read then and may be NULL.  The vuv
 * column is never touched, unmasked frames are never written, values that are not finite travel through this arithmetic, and every
 * loop is bounded by n and max_iter.
 *
 * Both calls only enqueue, on wc_set_stream's stream.  wc_mlpg_gv_device forms a0, a1, a2 and r once per call, 4 doubles per frame
 * and static column (6 where an utterance is too long for the on-chip copy of its trajectory), in the per-device scratch of the model
 * features, which grows on demand and goes with wc_release_scratch().  Refused with WC_ERR_INVALID (the text in wc_last_error), before
 * anything is enqueued or written: the shape and format refusals of wc_mlpg_device (nd < 1, n_ap < 0, orders outside {2, 3}, a format
 * outside {0, 1}, var_per_frame outside {0, 1}, a negative length or count, more than 2^32 - 1 frames, NULL lengths); max_iter < 0 or
 * > 64; a w_ml, w_gv or step_init that is NaN, negative or infinite; w_ml == 0; with frames to do (for wc_gv_stats_device: with
 * utterances to do) a NULL array other than d_mask; d_static overlapping any input; the two outputs of wc_gv_stats_device overlapping
 * each other or d_static. */
#ifndef WORLD_CLASS_GV_H
#define WORLD_CLASS_GV_H

#include "world_class_features.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per utterance and static column, over the frames whose mask byte is not 0 (d_mask NULL: every frame):
 * d_mean_out, d_var_out: n_utt * S doubles */
int wc_gv_stats_device(int n_utt, const int *lengths, int nd, int n_ap, const double *d_static, const unsigned char *d_mask,
                       double *d_mean_out, double *d_var_out);

/* d_static: wc_mlpg_device's output on the same d_mean / d_var, refined in place.  d_gv_mean, d_gv_var: S doubles each,
 * the mean and the variance of the utterance-level variance of each static column over the training data */
int wc_mlpg_gv_device(int n_utt, const int *lengths, int nd, int n_ap, int orders, int in_format, const void *d_mean, const void *d_var,
                      int var_per_frame, const double *d_gv_mean, const double *d_gv_var, const unsigned char *d_mask, double w_ml,
                      double w_gv, double step_init, int max_iter, double *d_static);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_GV_H */
