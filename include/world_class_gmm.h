/* ---- Joint-density GMM conversion in front of MLPG on the device (extension) ----
 *
 * The headers of the model features write their chain as  pack -> (model) -> MLPG -> GV -> unpack -> coded synthesis.  This one is a
 * model for the brackets: joint-density Gaussian-mixture conversion (Toda, Black & Tokuda 2007), the companion of MLPG and GV in the
 * literature those calls were built from.  A mixture over joint source/target rows [x; y] is evaluated frame by frame, the most likely
 * mixture of every frame is chosen, and that mixture's conditional mean and conditional variance of y given x are written as per-frame
 * means and variances, which wc_mlpg_device(..., var_per_frame = 1) takes.  The call is stateless per frame, so the same call stands
 * between a feature stream and an MLPG stream.  Training (EM) happens elsewhere.  A header of its own with a binding table of its own
 * in the Python mirror (world_class_amd/gmm.py: GMM_SIGNATURES); tests/gmm_rule.py states THE rule in numpy and Python floats.
 *
 * Layout.  The source vector of frame t is columns [col_in, col_in + dx) of input row t, whose width is ld_in elements of in_format
 * (WC_FEAT_F64 / WC_FEAT_F32).  The outputs go to columns [col_out, col_out + dy) of row t of d_mean and d_var, whose width is ld_out
 * elements of out_format; every other column of those rows is left exactly as it was.  The mgc block of a packed model row is
 * contiguous (orders * nd columns from 0), so it converts in place in MLPG's layout and the caller fills the lf0, vuv and band columns
 * as it likes.  d_best: n_frames ints; d_loglik: n_frames * n_mix doubles, ll(m) of frame t at t * n_mix + m, for callers that want
 * posteriors.  Each of the four outputs may be NULL.
 *
 * THE rule of create.  It runs on the host, per mixture.  Every operation is in double, rounded on its own, with no fma.
 * D = dx + dy; Sxx (dx x dx), Syx (dy x dx) and Syy (dy x dy) are the blocks of the mixture's covariance, of which only the lower
 * triangle (column <= row) is read; mux and muy the two parts of its mean; w its weight.
 *   Cholesky, row by row.  For i ascending and j = 0..i:  s = Sxx(i,j), then s = s - L(i,k) * L(j,k) for k = 0..j-1 ascending.
 *                          Then L(i,j) = s / L(j,j) for j < i, and L(i,i) = sqrt(s).
 *   W = L^-1, column by column.  W(j,j) = 1.0 / L(j,j).  For i > j:  s = L(i,j) * W(j,j), then s = s + L(i,k) * W(k,j) for
 *                          k = j+1..i-1 ascending, and W(i,j) = -s / L(i,i).
 *   B = Syx W^T.           B(j,k) is the sum of Syx(j,i) * W(k,i) over i = 0..k, ascending.  The sum starts at its first product.
 *   cvar(j).               s = Syy(j,j), then s = s - B(j,k) * B(j,k) for k ascending.
 *   c.                     c = (log(w) - ld) - (0.5 * (double)dx) * 1.8378770664093453, where ld = log L(0,0) and then
 *                          ld = ld + log L(i,i) ascending.  log is the C library's.
 *
 * THE rule of convert.  It runs per frame, with the same arithmetic conventions.  A float input is widened exactly.  A float output
 * is the (float) of the double.
 *   For every mixture m:   d(k) = x(k) - mux_m(k).
 *                          z(i) is the sum of W_m(i,k) * d(k) over k = 0..i, ascending, starting at its first product.
 *                          q is the sum of z(i) * z(i) over i, ascending, in the same form.
 *                          ll(m) = c_m - 0.5 * q.
 *   best is the least m whose ll(m) is not NaN and is >= every other ll that is not NaN.
 *   mean(j) = muy_best(j) + s, where s is the sum of B_best(j,k) * z_best(k) over k ascending, starting at its first product.
 *   var(j) = cvar_best(j).
 *   If every ll is NaN:    best = -1, mean(j) = 0.0, var(j) = +inf.
 * A NaN in the source vector makes every ll NaN.  So does an infinity wherever the rule's arithmetic turns it into one: where it
 * meets a W_m(i,k) that is 0.0, or an infinity of the other sign in the same sum, in every mixture.  MLPG's rule drops an observation
 * whose variance is +inf, so a frame the model cannot judge drops out of the generation instead of poisoning its column.  An infinity
 * that the arithmetic carries through as ll = -inf is judged like any other number, as the rule says.  A NaN in d_loglik is a NaN: its
 * sign and payload are no part of the rule.  Every loop is bounded by n_mix, dx and dy.  Whichever way a call is cut into launches,
 * each ll(t, m) is computed by this one sequence of operations: the result never depends on the launch shape, nor on the pushes a
 * caller cuts its frames into.
 *
 * wc_gmm_convert_device only enqueues, on wc_set_stream's stream.  The handle lives on the device that is current at create and is
 * read-only afterwards: several host threads may convert with one handle on their own streams.  Where d_loglik is NULL and a best
 * mixture is asked for, the table of ll stands in the per-device scratch of the model features (at most 256 MiB of it: a longer call
 * is cut into launches), which grows on demand, is handed from stream to stream and goes with wc_release_scratch().
 *
 * Refusals.  Create returns NULL, convert returns WC_ERR_INVALID; the text is in wc_last_error.  Every refusal happens before
 * anything is allocated, enqueued or written.  Create refuses: n_mix outside 1..1024; dx or dy outside 1..192; a NULL array; a weight
 * that is not finite or not > 0; a non-finite value among the means and the covariance entries read; a Cholesky s on the diagonal, or
 * a cvar, that is not > 0 or not finite (the text names the mixture and the row).  Weights need not sum to 1.  Convert refuses: a NULL
 * handle; n_frames < 0 or > 2^32 - 1; a format outside {0, 1}; a negative column; ld_in < col_in + dx; ld_out < col_out + dy; with
 * frames to do, a NULL d_rows_in, or all four outputs NULL; any output overlapping the input or another output.  n_frames == 0 writes
 * nothing. */
#ifndef WORLD_CLASS_GMM_H
#define WORLD_CLASS_GMM_H

#include "world_class_features.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wc_gmm wc_gmm;

/* joint model on host arrays, D = dx + dy: h_weight n_mix; h_mean n_mix * D ([x; y]);
 * h_cov n_mix * D * D row-major, of which only the lower triangle (column <= row) is read */
wc_gmm *wc_gmm_create(int n_mix, int dx, int dy, const double *h_weight, const double *h_mean, const double *h_cov);
void wc_gmm_destroy(wc_gmm *g);

/* what create prepared, back on the host; each pointer may be NULL:
 * c n_mix; W n_mix*dx*dx (upper part 0.0); B n_mix*dy*dx; cvar n_mix*dy */
int wc_gmm_prepared_host(const wc_gmm *g, double *h_c, double *h_W, double *h_B, double *h_cvar);

int wc_gmm_convert_device(const wc_gmm *g, long long n_frames,
                          int in_format, const void *d_rows_in, int ld_in, int col_in,
                          int out_format, void *d_mean, void *d_var, int ld_out, int col_out,
                          int *d_best, double *d_loglik);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_GMM_H */
