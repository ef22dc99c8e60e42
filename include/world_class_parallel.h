/* ---- Parallel-corpus joint rows: path gather, speech mask, distortion along the path (extension) ----
 *
 * world_class_gmm_train.h starts from "two speakers' parallel utterances, coded, aligned and brought onto one time line, stand in
 * device memory as joint rows"; the three calls of this header put them there.  The alignment (wc_align_features[_ex]_device) writes a
 * path of (i, j) cells and a path length per pair, both in device memory; wc_joint_rows_device gathers both speakers' rows along that
 * path into rows [x; y] with a mask byte per row, wc_speech_mask_device makes the mask that keeps silence out of the training, and
 * wc_path_distortion_device sums the local distance along the path.  Nothing is read back: two speakers' waveforms reach a trained
 * wc_gmm with no device-to-host copy except the M-step's statistics.  A header of its own with a binding table of its own in the Python
 * mirror (world_class_amd/parallel.py: PARALLEL_SIGNATURES); tests/parallel_rule.py states THE rule in numpy and Python floats.
 *
 * Conventions shared by the three calls.
 *   Pairs.        Pair u has a = a_length[u] rows of A and b = b_length[u] rows of B (host arrays).
 *   Row packing.  A's rows are packed pair after pair; pair u's first row is A_u = sum_{v<u} a_length[v].  B's rows are packed likewise
 *                 from B_u.
 *   Paths.        d_path and d_path_length are exactly what the two alignment calls write: pair u owns the slots 0 <= s < cap_u =
 *                 a + b - 1; slot s is entry P_u + s, with P_u = sum_{v<u} cap_v; an entry is two int32 values (i, j).
 *   Path length.  With K = d_path_length[u], K' = K if 0 <= K <= cap_u, else K' = 0.
 *   Slot states.  A slot is on the path iff s < K', 0 <= i < a and 0 <= j < b.  A slot is live iff it is on the path, A's mask byte of
 *                 frame A_u + i is not 0 and B's mask byte of frame B_u + j is not 0; a NULL mask means every frame counts (the
 *                 convention of world_class_gv.h).  A path the caller wrote itself may hold anything: an entry that is not on the path
 *                 is never used as an index.
 *   Rows.         A row vector is columns [col, col + d) of a row of ld elements of format (WC_FEAT_F64 / WC_FEAT_F32), as in
 *                 world_class_gmm.h.  A float read is widened exactly; a float written is the (float) of the double; same format to
 *                 same format copies the bits.
 *
 * wc_joint_rows_device.  The output has sum_u cap_u rows: one row and one mask byte per slot, so the host never needs K.  A slot on the
 * path: columns [col_out, col_out + dx) are A's vector of frame i, columns [col_out + dx, col_out + dx + dy) are B's vector of frame
 * j, and the mask byte is 1 if the slot is live, else 0.  A slot not on the path: those dx + dy columns are +0.0 and the mask byte is
 * 0.  Every other column of every output row is left exactly as it was.  d_joint_mask may be NULL; d_joint may not.  The rows and the
 * mask are what wc_gmm_trainer_accumulate_device(t, sum cap, out_format, d_joint, ld_out, col_out, d_joint_mask) takes.  A pair whose
 * alignment was not finite has K = 0, so it contributes nothing.
 *
 * wc_speech_mask_device.  The rule runs per utterance, on the one column col: c0 of the coded envelope, which is column 0 of a packed
 * model row.  top is the greatest value of the column that is finite.  Frame t gets 1 iff its value v is finite, v >= top - margin (one
 * rounded subtraction) and v >= floor; otherwise it gets 0.  With no finite value in the utterance every byte is 0.  margin = +inf and
 * floor = -inf are allowed and switch that test off.  Nothing crosses an utterance boundary.  A maximum is exact, so the launch shape
 * cannot change a byte.
 *   The unit of margin.  margin is in the column's own units.  The codec writes (wc_codec.hip, code_sp_kernel)
 *       out[i] = (re * w.x - im * w.y) / normalization
 *   and at i = 0 re is the plain sum of the fft_size / 2 mel-spaced samples of ln(power spectrum), im = 0, w.x = (2 / sqrt(fft_size)) /
 *   sqrt(2) and normalization = sqrt(fft_size / 2), so c0 = sum * 2 / fft_size: the mean of the natural log of the power over the mel
 *   axis, whatever fft_size is.  One decibel of frame power multiplies every sample of the power spectrum by 10^(1/10) and so adds
 *   ln(10) / 10 = 0.23025850929940458 to c0.  One decibel is ln(10) / 10 units of c0: margin = 40 dB is 9.210340371976184.
 *
 * wc_path_distortion_device.  Cell distance: e(s) = sqrt(sum_c (x_c - y_c)^2) over the dims columns ascending from 0.0, every
 * difference, product and sum rounded on its own, no fma, the square root correctly rounded: the local cost of
 * wc_align_features_device, word for word.  d_count[u] is the number of live slots.  d_sum[u] is the sum of e(s) over the live slots in
 * ascending s; the sum starts at its first term and is +0.0 for none.  The sum is strictly sequential on purpose: a path has a few
 * thousand cells and a batch has many pairs, so the parallelism is across pairs and across the cells' distances, not inside the sum.
 * d_cell is optional and packed like d_path: e(s) for slots on the path, whether live or not, and +0.0 for the others.  Values that are
 * not finite travel through as they are.  The value of d_sum does not depend on the launch shape.
 *   What the order buys.  With step pattern 0, NULL masks, ld = dims_of_align, col = dim_begin and dims = dim_end - dim_begin, d_sum[u]
 *   equals the alignment's d_cost[u] bit for bit at every length, because D(i, j) = d(i, j) + best is this very chain of additions.
 *   As mel-cepstral distortion: mcd_db = (10 / ln 10) * sqrt(2) * sum / count, on the host (the mirror's mcd_db).
 *
 * The three calls only enqueue, on wc_set_stream's stream.  They return WC_OK or WC_ERR_INVALID, with the text in wc_last_error, and
 * refuse before anything is enqueued or written.  Refused: n_pairs / n_utt < 0; a length below 1 for a pair; a negative utterance
 * length; a format outside {0, 1}; a negative column; dx, dy or dims < 1; dx + dy > 384; an ld smaller than col plus the width read or
 * written; more than 2^31 - 1 slots, or 2^32 - 1 frames, in all; margin or floor NaN; margin < 0.  With work to do also: a NULL length
 * array, input, path, path length or required output; all three outputs of the distortion call NULL; an output that overlaps an input
 * or another output.  n_pairs == 0 / n_utt == 0 write nothing.  No atomics; every loop is bounded by arguments the host validated,
 * and every index read from the path is bounded by the on-path test: a path of garbage costs nothing but masked rows.  The call's
 * descriptors, and the distances where d_cell is NULL, stand in a buffer per device and stream that grows on demand. */
#ifndef WORLD_CLASS_PARALLEL_H
#define WORLD_CLASS_PARALLEL_H

#include "world_class_gmm_train.h"

#ifdef __cplusplus
extern "C" {
#endif

int wc_joint_rows_device(int n_pairs, const int *a_length, const int *b_length,
                         int a_format, const void *d_rows_a, int ld_a, int col_a, int dx,
                         int b_format, const void *d_rows_b, int ld_b, int col_b, int dy,
                         const int *d_path_length, const int *d_path,
                         const unsigned char *d_mask_a, const unsigned char *d_mask_b,
                         int out_format, void *d_joint, int ld_out, int col_out, unsigned char *d_joint_mask);

int wc_speech_mask_device(int n_utt, const int *lengths, int format, const void *d_rows, int ld, int col,
                          double margin, double floor, unsigned char *d_mask);

int wc_path_distortion_device(int n_pairs, const int *a_length, const int *b_length,
                              int a_format, const void *d_rows_a, int ld_a, int col_a,
                              int b_format, const void *d_rows_b, int ld_b, int col_b, int dims,
                              const int *d_path_length, const int *d_path,
                              const unsigned char *d_mask_a, const unsigned char *d_mask_b,
                              double *d_sum, long long *d_count, double *d_cell);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_PARALLEL_H */
