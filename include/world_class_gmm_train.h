/* ---- Training the joint-density GMM on the device: expectation-maximisation over joint rows (extension) ----
 *
 * world_class_gmm.h converts with a mixture over joint source/target rows [x; y]; this header produces one.  Two speakers' parallel
 * utterances, coded, aligned and brought onto one time line, stand in device memory as joint rows; a trainer handle holds a model
 * (the three arrays wc_gmm_create takes), evaluates the posteriors of every frame under it (E-step), sums the sufficient statistics of
 * every mixture on the device, and re-estimates the model from them on the host (M-step).  wc_gmm_trainer_model_host hands the
 * model out in exactly the layout wc_gmm_create reads.  A header of its own with a binding table of its own in the Python mirror
 * (world_class_amd/gmm_train.py: GMM_TRAIN_SIGNATURES); tests/gmm_train_rule.py states THE rule in numpy and Python floats.
 *
 * Layout.  D = dx + dy.  The joint vector z_t of frame t is columns [col, col + D) of row t of d_rows, whose width is ld elements of
 * format (WC_FEAT_F64 / WC_FEAT_F32; a float is widened exactly).  d_mask follows the convention of world_class_gv.h: a frame counts
 * where its byte is not 0, and NULL means every frame counts.  d_post: n_frames * n_mix doubles, the posterior of mixture m at
 * t * n_mix + m; d_frame_ll: n_frames doubles.  h_N: n_mix; h_S1: n_mix * D; h_S2: n_mix * D(D+1)/2, the lower triangles packed row
 * by row, S2_m(i, j) at m * D(D+1)/2 + i(i+1)/2 + j.  accumulate may be called many times between updates, one utterance per call for
 * example.
 *
 * THE rule.  Every operation is in double, rounded on its own, with no fma.
 *   Joint preparation.     Per mixture, the Cholesky factor, W = L^-1 and c of THE rule of create in world_class_gmm.h, operation for
 *                          operation, applied to the whole D x D covariance: that rule with dx := D and Sxx := the joint covariance.
 *   ll.                    ll(t, m) is THE rule of convert on the joint row with that W, mux := mean and c.
 *   Posteriors, per frame, mixtures ascending.  top is the greatest ll that is not NaN.  A frame whose mask byte is 0 is masked.  A
 *                          frame that is not masked and has no finite top is dropped and counted.  Masked and dropped frames have
 *                          gamma(m) = 0.0 for every m and frame_ll = 0.0, and the statistics do not read their rows.  Every other
 *                          frame is live:  e(m) = exp(ll(m) - top), and 0.0 where ll(m) is NaN;  s is the sum of e(m) over m ascending,
 *                          starting at its first term;  gamma(m) = e(m) / s;  frame_ll = top + log(s).  exp and log are the device
 *                          library's: they are the one place where the device and a host restatement may differ.
 *   Statistics.            With d(i) = z_t(i) - mean_m(i), centred on the model in force (which keeps the covariance from
 *                          cancelling), and g = gamma(t, m) * d(i):  N_m sums gamma(t, m);  S1_m(i) sums g;  S2_m(i, j), j <= i, sums
 *                          g * d(j);  LL sums frame_ll.  The frames of one call are cut into segments of 1024 from the call's first
 *                          frame.  Within a segment every sum runs over the live frames ascending and starts at its first term; an
 *                          empty sum is +0.0.  Segment sums are folded into the totals ascending, total = total + partial.  Totals
 *                          start at +0.0 after create, update and reset.  n_live and n_dropped count the frames.
 *   Update, on the host, per mixture.  A mixture with !(N_m >= min_occupancy) is starved: it keeps its weight, mean and covariance.
 *                          Otherwise  w = N_m / (double)n_live,  delta(i) = S1(i) / N_m,  mean(i) = mean(i) + delta(i),
 *                          cov(i, j) = S2(i, j) / N_m - delta(i) * delta(j) for j <= i.  The diagonal is raised to h_var_floor[i]
 *                          where it is below it (NULL: no floor).  The upper triangle is mirrored.  A mixture whose new mean or
 *                          covariance holds a value that is not finite, or whose new covariance fails the joint Cholesky, keeps
 *                          its three old values and is counted in n_kept.  loglik = LL: the likelihood under the model the
 *                          statistics were taken with.  Weights need not sum to 1.
 * The result depends neither on the launch shape nor on how many segments a launch takes.  A corpus accumulated in calls whose
 * lengths are multiples of 1024 equals the one call bit for bit; any other cut equals the rule for that cut.  Every loop is bounded
 * by n_mix, D and the segment.  No atomics and no matrix instructions: their order of accumulation is no part of any rule here.
 *
 * posterior_device and accumulate_device only enqueue, on wc_set_stream's stream; posterior_device hands out exactly what the E-step
 * of accumulate uses and leaves the statistics alone.  The tables of ll and gamma and the segment sums stand in the per-device scratch
 * of the model features (about 256 MiB of it at the most unless set_segments_per_launch says otherwise: a longer call is cut into
 * launches of whole segments), which goes with wc_release_scratch().  stats_host, update and set_model wait for the device.  A handle
 * belongs to one host thread at a time; two handles may be driven from two threads.
 *
 * Refusals.  Create returns NULL, the other calls WC_ERR_INVALID; the text is in wc_last_error.  Every refusal happens before
 * anything is allocated, enqueued or written.  Create refuses n_mix outside 1..1024, dx or dy < 1, D outside 2..192.  set_model
 * refuses what wc_gmm_create refuses, on the joint matrix (the text names the mixture and the row).  Refused elsewhere: a NULL handle;
 * accumulate, posterior, update or model_host before a model is set; a format outside {0, 1}; a negative column; ld < col + D; a NULL
 * d_rows with frames to do; n_frames < 0 or > 2^32 - 1; both outputs of posterior NULL, or an output overlapping the other, the rows
 * or the mask; min_occupancy not finite or < 1; a floor that is negative or not finite; update with n_live == 0; g < 0.
 * n_frames == 0 does nothing. */
#ifndef WORLD_CLASS_GMM_TRAIN_H
#define WORLD_CLASS_GMM_TRAIN_H

#include "world_class_gmm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wc_gmm_trainer wc_gmm_trainer;
typedef struct {
	double loglik;
	long long n_live, n_dropped;
	int n_starved, n_kept; /* set by update; 0 from stats_host */
} wc_gmm_train_info;

wc_gmm_trainer *wc_gmm_trainer_create(int n_mix, int dx, int dy);
void wc_gmm_trainer_destroy(wc_gmm_trainer *t);

/* the arrays of wc_gmm_create: h_weight n_mix; h_mean n_mix * D; h_cov n_mix * D * D row-major, lower triangle read.  model_host
 * writes both triangles; each of its pointers may be NULL */
int wc_gmm_trainer_set_model(wc_gmm_trainer *t, const double *h_weight, const double *h_mean, const double *h_cov);
int wc_gmm_trainer_model_host(const wc_gmm_trainer *t, double *h_weight, double *h_mean, double *h_cov);

/* the E-step alone; one of d_post and d_frame_ll may be NULL */
int wc_gmm_trainer_posterior_device(wc_gmm_trainer *t, long long n_frames, int format, const void *d_rows, int ld, int col,
                                    const unsigned char *d_mask, double *d_post, double *d_frame_ll);
/* the E-step and the statistics, added to the handle's totals */
int wc_gmm_trainer_accumulate_device(wc_gmm_trainer *t, long long n_frames, int format, const void *d_rows, int ld, int col,
                                     const unsigned char *d_mask);
/* the totals; each pointer may be NULL */
int wc_gmm_trainer_stats_host(wc_gmm_trainer *t, double *h_N, double *h_S1, double *h_S2, wc_gmm_train_info *info);
/* the M-step; clears the statistics; h_var_floor: D values or NULL; info may be NULL */
int wc_gmm_trainer_update(wc_gmm_trainer *t, double min_occupancy, const double *h_var_floor, wc_gmm_train_info *info);
int wc_gmm_trainer_reset_stats(wc_gmm_trainer *t);
/* g segments of 1024 frames per launch; 0: chosen from the scratch budget.  Never changes a result */
int wc_gmm_trainer_set_segments_per_launch(wc_gmm_trainer *t, int g);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_GMM_TRAIN_H */
