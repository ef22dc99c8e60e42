/* ---- Warping: signals resampled along positions read on the device (extension) ----
 *
 * world_class_vresample.h places output n at the arithmetic position n * step, the step set on the host.  Here every output has a
 * position of its own, read from device memory: a time map from wc_align_features_device carried onto the waveform itself, a vibrato
 * or wow-and-flutter curve, a speed glide, reverse playback.  The calls run on a wc_vresampler and use its table; a header of its own
 * with a binding table of its own in the Python mirror (world_class_amd/warp.py: WARP_SIGNATURES).
 *
 * Positions.  A position is a signed 64-bit integer pos = q * 2^32 + f: q = pos >> 32 (an arithmetic shift: the floor), f the low 32
 * bits -- the pair (q, f) of world_class_vresample.h.  Output n of an utterance is THE rule of that header at (q, f) of d_pos[n]: the
 * same table, segment and nu, every tap added by ascending j from 0.0, every product and every sum rounded (no fma), x outside [0, N)
 * read as +0.0.  Nothing is required of the positions: they may repeat, fall or jump.  The cut-off is the handle's, fixed by its
 * step_max; positions that advance by more than step_max per output alias, and that is the caller's affair.  An output with q < -K or
 * q > N - 1 + K has every tap outside the signal: by the rule it is +0.0, and no address is formed for it.  WC_WARP_NO_POSITION lies
 * before every signal, so it is such an output and needs no case of its own.
 *
 * The map rule.  A frame-level time map of L >= 1 doubles (d_b_on_a of wc_align_features_device, a d_position of retime or morph, the
 * settled positions of an alignment stream) becomes sample positions: for output n, every operation in double and rounded, no fma,
 *   t = (double)n / out_per_entry
 *   t >= L - 1:  v = map[L - 1]                                                    (the end is held)
 *   otherwise:   i = floor(t), w = t - i, v = (w == 0) ? map[i] : map[i] + w * (map[i + 1] - map[i])
 *   p = v * in_per_unit
 *   pos = (p is finite and -2^30 <= p < 2^30) ? (long long)floor(p * 4294967296.0) : WC_WARP_NO_POSITION
 * With map = d_b_on_a, out_per_entry = A's hop in samples and in_per_unit = B's hop in samples the warp gives B's waveform on A's
 * timing.  A NaN in a map (an unsettled row) becomes silence at the outputs that read it and touches no other.
 *
 * Refused with WC_ERR_INVALID (a negative result), the text in wc_last_error; every refusal comes before the first enqueue. */
#ifndef WORLD_CLASS_WARP_H
#define WORLD_CLASS_WARP_H

#include <limits.h>

#include "world_class_vresample.h"

#define WC_WARP_NO_POSITION LLONG_MIN

#ifdef __cplusplus
extern "C" {
#endif

/* ---- pure host functions: no handle, no device ---- */
/* How wc_warp_device cuts the work, for tests and tools; the plan arguments and *tile_outputs, *segment_min and *plain_block are
 * wc_vresample_tiling's.  A tile whose live outputs (-K <= q <= N - 1 + K) span q_max - q_min + 2K + 1 <= *span_max input samples is
 * a near tile: it holds that span in local memory.  Any other tile is a far tile and reads its inputs from global memory.  Where
 * *tile_outputs is 0, *span_max is what the shortest tile would have needed. */
int wc_warp_tiling(unsigned long long step_min, unsigned long long step_max, int zeros, double rolloff, int phase_bits, int degree,
                   int *tile_outputs, int *span_max, int *segment_min, int *plain_block);
/* (long long)floor((double)(map_length - 1) * out_per_entry) + 1: the outputs up to the map's last entry.  Refused: map_length < 1,
 * an out_per_entry that is not finite and positive, a result of 2^62 and more */
long long wc_warp_map_out_length(int map_length, double out_per_entry);
/* the map rule for outputs 0 .. n_out - 1.  Refused: NULL arrays, map_length < 1, n_out < 0, an out_per_entry or in_per_unit that is
 * not finite and positive */
int wc_warp_map_positions(const double *map, int map_length, double out_per_entry, double in_per_unit, long long n_out, long long *pos);

/* ---- on the device ----
 * Both calls only enqueue, on wc_set_stream's stream; their records go up through the handle's page-locked staging, as
 * wc_vresample_device's do.  n_utt utterances packed like every batch here: utterance u's input at the sum of x_length[< u], its
 * positions and its outputs at the sum of out_length[< u]; x_length and out_length are host arrays.  out_length[u] == 0 is allowed.
 * Formats as in wc_vresample_device.  Refused: NULL arrays, n_utt < 1, an x_length below 1, an out_length below 0, a batch whose
 * packed output exceeds 2^31 - 1 samples, a format out of range. */
int wc_warp_device(wc_vresampler *r, int n_utt, const void *d_x, int in_format, const int *x_length, const long long *d_pos,
                   const int *out_length, void *d_y, int out_format);
/* The map rule on the device, bit for bit wc_warp_map_positions: n_utt maps packed by map_length, their positions by out_length.
 * Refused: NULL arrays, n_utt < 1, a map_length below 1, an out_length below 0, packed positions above 2^31 - 1, an out_per_entry or
 * in_per_unit that is not finite and positive. */
int wc_warp_map_positions_device(wc_vresampler *r, int n_utt, const double *d_map, const int *map_length, double out_per_entry,
                                 double in_per_unit, const int *out_length, long long *d_pos);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_WARP_H */
