/* world_class_io.h -- the data formats on either side of the hot path,
 * exported by the same libworldclass_hip.so as world_class_c.h.
 *
 *   - the reference's WAV reader / writer (reference tools/audioio.hpp:22-47, tools/audioio.cpp:116-253) and its
 *     F0 / spectral-envelope / aperiodicity parameter files (reference tools/parameterio.hpp:24-121,
 *     tools/parameterio.cpp:60-244): SAME function names, argument meaning, file bytes and return values, so a caller
 *     of the reference's tools links against this library unchanged.  Host code only (no GPU needed).
 *     Where the reference prints a message and returns, these do the same (message on stderr, also kept for
 *     wc_last_error()).
 *   - device-side sample conversion, so that PCM travels over PCIe as int16 (4x fewer bytes than double) and is
 *     expanded / quantised on the GPU with exactly wavread's / wavwrite's arithmetic;
 *   - the demo's parameter modification (reference test/test.cpp:201-243: F0 scaling, spectral stretching) as a
 *     device kernel between analysis and synthesis, no host round trip.
 */
#ifndef WORLD_CLASS_IO_H
#define WORLD_CLASS_IO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference tools/audioio.hpp --------------------------------------------------------------------------- */
/* 16-bit mono PCM; nbit is ignored exactly as in the reference (tools/audioio.cpp:116-165).
 * sample = clamp(int(x * 32767), -32768, 32767), the conversion truncating toward zero. */
void wavwrite(const double *x, int x_length, int fs, int nbit, const char *filename);
/* number of samples; 0 if the file cannot be opened, -1 on a header the reference rejects
 * (tools/audioio.cpp:167-207) */
int GetAudioLength(const char *filename);
/* x[i] = signed little-endian sample / 2^(nbit-1) for nbit = 8, 16, 24 or 32 (tools/audioio.cpp:209-253); outputs
 * are left untouched when the header is rejected */
void wavread(const char *filename, int *fs, int *nbit, double *x);

/* ---- reference tools/parameterio.hpp ------------------------------------------------------------------------ */
void WriteF0(const char *filename, int f0_length, double frame_period, const double *temporal_positions, const double *f0,
			 int text_flag);
int ReadF0(const char *filename, double *temporal_positions, double *f0);
double GetHeaderInformation(const char *filename, const char *parameter);
void WriteSpectralEnvelope(const char *filename, int fs, int f0_length, double frame_period, int fft_size,
						   int number_of_dimensions, const double *const *spectrogram);
int ReadSpectralEnvelope(const char *filename, double **spectrogram);
void WriteAperiodicity(const char *filename, int fs, int f0_length, double frame_period, int fft_size, int number_of_dimensions,
					   const double *const *aperiodicity);
int ReadAperiodicity(const char *filename, double **aperiodicity);

/* ---- extensions (wc_ prefix): raw PCM access and device-side conversion -------------------------------------- */
/* The 16-bit samples of a WAV file as stored (no scaling); returns the number of samples read (<= capacity),
 * 0 / -1 like GetAudioLength, -2 if the file is not 16-bit. */
int wc_wavread_pcm16(const char *filename, int *fs, int16_t *pcm, int capacity);
/* d_x[i] = d_pcm[i] / 32768.0 (wavread's scaling) on the current device / stream; pointers are device pointers */
int wc_pcm16_to_double_device(const int16_t *d_pcm, long long n, double *d_x);
/* d_x[i] = (double)d_f[i]: 32-bit float samples (the other common in-memory format) widened on the device, exactly */
int wc_float_to_double_device(const float *d_f, long long n, double *d_x);
/* d_pcm[i] = wavwrite's quantisation of d_y[i] */
int wc_double_to_pcm16_device(const double *d_y, long long n, int16_t *d_pcm);

/* ---- parameter modification (reference test/test.cpp:201-243) on device-resident parameters ------------------ */
/* f0[i] *= f0_scale for n_frames frames (pass 1.0 to leave it), then, if spectral_ratio != 0, every row of d_sp
 * (n_frames rows of fft_size/2+1 doubles, packed like the batch layout of world_class_c.h) is stretched:
 * log -> interp1 from the axis ratio * k * fs / fft_size onto k * fs / fft_size -> exp, and for ratio < 1 the
 * bins from int(fft_size / 2.0 * ratio) upward repeat the bin just below. */
int wc_modify_parameters_device(int fs, int fft_size, long long n_frames, double *d_f0, double *d_sp, double f0_scale,
								double spectral_ratio);
/* The same with a scale and a ratio per frame (a packed batch or a push of many streams holds many speakers, and a shift may
 * change over time): d_f0_scale and d_spectral_ratio are device arrays of n_frames doubles.  f0[i] *= d_f0_scale[i] (a plain
 * product: NaN in, NaN out); row i of d_sp is, bit for bit, what the call above writes with spectral_ratio =
 * d_spectral_ratio[i].  Any of d_f0, d_sp, d_f0_scale, d_spectral_ratio may be NULL: that part is left alone.  The values live
 * on the device, so the host cannot refuse them; per frame: 0 leaves the row as it is, a finite ratio >= 2.0 / fft_size is
 * stretched (below that the fill for ratio < 1 would read bin -1), anything else -- negative, NaN, infinite, 0 < ratio <
 * 2.0 / fft_size -- turns that frame's row into NaN and touches no other frame.  Stream-ordered, enqueue-only.
 * n_frames <= 0xffffffff. */
int wc_modify_parameters_frames_device(int fs, int fft_size, long long n_frames, double *d_f0, double *d_sp,
									   const double *d_f0_scale, const double *d_spectral_ratio);

/* ---- time-scale modification ----------------------------------------------------------------------------------- */
/* The frames of a packed batch resampled along a time map, out of place.  Utterance u has in_length[u] source frames and gets
 * out_length[u] output frames (host arrays; the device arrays are packed in utterance order, source frames for the inputs, output
 * frames for d_position, d_f0_scale, d_spectral_ratio and the outputs).  d_position[k] is output frame k's place in source
 * frames, counted from its utterance's first frame; with n source frames:
 *   not finite: F0 and both rows of that frame are NaN, no other frame is touched;
 *   else p = min(max(position, 0), n - 1) (the end frames are held), i = floor(p), a = p - i;
 *   a == 0: source frame i, bit for bit;  a > 0: row = (1 - a) * row[i] + a * row[i + 1] for sp and ap (the interpolation of
 *   reference src/synthesis.cpp:346-393), F0 = (1 - a) * f0[i] + a * f0[i + 1] between two voiced frames, 0 between two unvoiced
 *   ones, and next to one voiced frame that frame's F0 while it is the nearer one (a < 0.5 for i, a > 0.5 for i + 1), else 0:
 *   voiced exactly where Synthesis' interpolated voicing is (:200-204).
 * Then, per OUTPUT frame, f0 *= d_f0_scale[k] and the row of sp stretched by d_spectral_ratio[k] with the rules and the bits of
 * wc_modify_parameters_frames_device (0 leaves the row, an invalid ratio makes it NaN); either array may be NULL.  The positions
 * need not be monotone and out_length has no relation to in_length.  Each of the pairs (d_f0_in, d_f0_out), (d_sp_in, d_sp_out),
 * (d_ap_in, d_ap_out) may be NULL together: that part is skipped.  Refused (WC_ERR_INVALID, nothing written): fft_size other than
 * 512 / 1024 / 2048 / 4096, fs <= 0, n_utt < 0, a negative length, out_length[u] > 0 with in_length[u] < 1, more than 2^32 - 1
 * frames in all on either side, NULL lengths or positions with frames to write, one half of a pair NULL, an output equal to its
 * input.  out_length[u] == 0 and n_utt == 0 write nothing.  Stream-ordered, enqueue-only. */
int wc_retime_parameters_device(int fs, int fft_size, int n_utt, const int *in_length, const double *d_f0_in, const double *d_sp_in,
								const double *d_ap_in, const int *out_length, const double *d_position, const double *d_f0_scale,
								const double *d_spectral_ratio, double *d_f0_out, double *d_sp_out, double *d_ap_out);

/* ---- voice morphing --------------------------------------------------------------------------------------------------- */
/* Two parameter sets blended along two time maps, out of place.  Pair u has a_length[u] source frames of A, b_length[u] of B and
 * gets out_length[u] output frames (host arrays; the device arrays are packed in pair order as for wc_retime_parameters_device:
 * source frames of A for A's inputs, source frames of B for B's, output frames for d_position_a, d_position_b, d_weight,
 * d_f0_weight, d_ratio_a, d_ratio_b and the outputs).  Output frame k has pa = d_position_a[k], pb = d_position_b[k], w =
 * d_weight[k] and wf = d_f0_weight[k] (NULL: wf = w):
 *   pa, pb or w not finite: F0 and both rows of that frame are NaN, no other frame is touched; only wf not finite: only that
 *   frame's F0 is NaN;
 *   A_k = the frame (F0, sp row, ap row) wc_retime_parameters_device forms from A at pa without scale or ratio, B_k the same from B
 *   at pb: the end frames are held, a whole position copies, otherwise two products and one sum, F0 voiced where Synthesis'
 *   interpolated voicing is -- that rule and its bits;
 *   ap: w == 0: A_k's row, w == 1: B_k's row, both bit for bit; else (1 - w) * apA + w * apB (two products and one sum, each
 *   rounded; what a weight outside [0, 1] puts outside [0, 1] is left to Synthesis' own clamp, as in retime);
 *   sp: la(b) is the log envelope of A_k at bin b: log(spA[b]) where d_ratio_a is NULL or 0 for this frame; with a valid ratio the
 *   value whose exp wc_modify_parameters_frames_device writes for that row and ratio (log -> interp1 from the stretched axis; for
 *   a ratio below 1 the bins from cut = int(fft_size / 2.0 * ratio) upward repeat the value of bin cut - 1); lb(b) the same for B
 *   with d_ratio_b.  An invalid ratio of EITHER source (negative, NaN, infinite, 0 < ratio < 2.0 / fft_size) makes the sp row NaN
 *   whatever the weight; F0 and ap of that frame are unaffected, as in retime.  w == 0: the row wc_retime_parameters_device writes
 *   for A with that ratio, w == 1: the same for B, both bit for bit; else sp[b] = exp((1 - w) * la(b) + w * lb(b)) (two products,
 *   one sum, one exp);
 *   F0, with fA, fB the retimed values: wf == 0: fA, wf == 1: fB, both bit for bit; both voiced: exp((1 - wf) * log fA + wf *
 *   log fB); neither: 0; only A voiced: fA while wf < 0.5, else 0; only B voiced: fB while wf > 0.5, else 0 -- the nearer-source
 *   rule of retime across the two voices: F0 never glides towards 0 Hz.
 * Weights need not lie in [0, 1] (extrapolation), positions need not be monotone, out_length has no relation to the source
 * lengths.  Each of the triples (d_f0_a, d_f0_b, d_f0_out), (d_sp_a, d_sp_b, d_sp_out), (d_ap_a, d_ap_b, d_ap_out) may be NULL
 * together: that part is skipped.  Refused (WC_ERR_INVALID, nothing written): fft_size other than 512 / 1024 / 2048 / 4096, fs <=
 * 0, n_pairs < 0, a negative length, out_length[u] > 0 with a_length[u] < 1 or b_length[u] < 1, more than 2^32 - 1 frames in all
 * on any side, NULL lengths, positions or weight with frames to write, a triple that is only partly NULL, an output equal to one
 * of its inputs.  out_length[u] == 0 and n_pairs == 0 write nothing.  Stream-ordered, enqueue-only. */
int wc_morph_parameters_device(int fs, int fft_size, int n_pairs, const int *a_length, const double *d_f0_a, const double *d_sp_a,
							   const double *d_ap_a, const int *b_length, const double *d_f0_b, const double *d_sp_b,
							   const double *d_ap_b, const int *out_length, const double *d_position_a, const double *d_position_b,
							   const double *d_weight, const double *d_f0_weight, const double *d_ratio_a, const double *d_ratio_b,
							   double *d_f0_out, double *d_sp_out, double *d_ap_out);

/* ---- feature alignment ------------------------------------------------------------------------------------------------ */
/* Dynamic time warping of a packed batch of pairs of feature sequences: where the time maps of the two calls above come from.  Pair
 * u has n = a_length[u] rows of A and m = b_length[u] rows of B (host arrays); a row holds dims doubles, the rows are packed pair
 * after pair (the layout of d_coded_sp everywhere).  Only the coefficients dim_begin <= c < dim_end are compared (dim_begin = 1
 * leaves out the energy coefficient).
 *   Local cost: d(i, j) = sqrt(sum_c (a[i][c] - b[j][c])^2), the sum over ascending c from 0.0, every difference, product and sum
 *   rounded on its own, the square root correctly rounded.
 *   Band: band == 0 allows every cell; band >= 1, with L = max(n, m) - 1, allows cell (i, j) iff |i * (m - 1) - j * (n - 1)| <=
 *   band * L in 64-bit integers (a Sakoe-Chiba band around the straight line between the corners; both corners and a connected path
 *   are always inside).
 *   Accumulation: D(0, 0) = d(0, 0); D(i, j) = d(i, j) + best of Dd = D(i - 1, j - 1), Du = D(i - 1, j), Dl = D(i, j - 1), a
 *   predecessor outside the matrix or the band counting as +inf, chosen by exactly these comparisons: the diagonal if Dd <= Du &&
 *   Dd <= Dl, else up if Du <= Dl, else left (they fix the tie-break and what NaN and inf do).
 *   Path: the recorded choices followed back from (n - 1, m - 1) to (0, 0); K cells, max(n, m) <= K <= n + m - 1.
 * Outputs (device arrays; each of d_path, d_b_on_a, d_a_on_b may be NULL): d_cost[u] = D(n - 1, m - 1); d_path_length[u] = K;
 * d_path: pair u's cells as (i, j) int32 pairs in forward order from entry sum_{v<u} (a_length[v] + b_length[v] - 1) on, only the
 * first K entries written; d_b_on_a, packed like A's frames: for frame i (jmin(i) + jmax(i)) * 0.5 over the path's cells in row i;
 * d_a_on_b the mirror image, packed like B's frames.  Both maps are exact half-integers and non-decreasing, and they are the
 * d_position arguments above: B at A's timing is wc_retime_parameters_device with out_length = a_length and d_position = d_b_on_a;
 * a morph on A's timeline takes d_position_a = 0, 1, ... and d_position_b = d_b_on_a.
 * A total cost that is not finite: d_cost[u] is written as it is, d_path_length[u] = 0, that pair's maps are NaN and its path
 * region is not written; no other pair is affected.
 * Refused (WC_ERR_INVALID, nothing written, nothing enqueued): n_pairs < 0, a length below 1, dims < 1, dim_begin < 0, dim_end >
 * dims, dim_begin >= dim_end, band < 0, NULL lengths, inputs, d_cost or d_path_length with pairs to do, and more than 2^28 stored
 * cells in all.  A pair stores n * W cells, W the widest row its band can have: W = m at band 0 (all n * m cells), W = min(m,
 * 2 * band * L / (n - 1) + 1) under a band -- the allowed cells, rounded up to whole rows.  The call's scratch is 9 bytes per
 * stored cell plus 8 bytes per possible path entry, 2.3 GB at the cap; it is one buffer per device that grows on demand, is shared
 * by the calls on that device (a call on another stream waits on the device for the one before it) and goes with
 * wc_release_scratch().  n_pairs == 0 writes nothing.  Stream-ordered, enqueue-only. */
int wc_align_features_device(int n_pairs, const int *a_length, const double *d_feat_a, const int *b_length, const double *d_feat_b,
							 int dims, int dim_begin, int dim_end, int band, double *d_cost, int *d_path_length, int *d_path,
							 double *d_b_on_a, double *d_a_on_b);

/* The same alignment under a wider rule: ends that need not be the corners, a step pattern that limits the slope, and the path's
 * own timeline.  Packing, the local cost d(i, j) and its rounding, the band predicate, the three comparisons, what a total that is
 * not finite does, the scratch and the stream order are those of wc_align_features_device; with step_pattern == 0, flags == 0 and
 * d_span, d_timeline_a, d_timeline_b NULL every output equals that call's byte for byte.  ok(i, j) below means inside the matrix
 * and inside the band; a term whose cells are not all ok is +inf.
 *   Steps: step_pattern == 0 has Dd = D(i - 1, j - 1), Du = D(i - 1, j), Dl = D(i, j - 1).  step_pattern == 1 keeps the slope between
 *   1/2 and 2: Dd = D(i - 1, j - 1), Du = D(i - 2, j - 1) + d(i - 1, j) (needs ok(i - 2, j - 1) and ok(i - 1, j)), Dl = D(i - 1, j - 2) +
 *   d(i, j - 1) (needs ok(i - 1, j - 2) and ok(i, j - 1)), each one rounded sum with the D operand first.  D(i, j) = d(i, j) + best, the
 *   diagonal if Dd <= Du && Dd <= Dl, else up if Du <= Dl, else left.  The path holds the intermediate cell: the choice up at (i, j)
 *   puts (i - 1, j) and then (i - 2, j - 1) behind it, the choice left (i, j - 1) and then (i - 1, j - 2), so a path still steps by one
 *   in each index and K <= n + m - 1.  With both ends closed the total is finite only if max(n, m) - 1 <= 2 * (min(n, m) - 1).
 *   Start: D(0, 0) = d(0, 0).  With WC_ALIGN_OPEN_BEGIN D(0, j) = d(0, j) for every ok (0, j) (row 0 takes no step) and the backtrack
 *   stops at the first cell it meets in row 0; without it, at (0, 0).
 *   End: with WC_ALIGN_OPEN_END the ok cells of row n - 1 are scanned by ascending j from best = +inf and j is taken when D(n - 1, j)
 *   < best: the lowest column of the minimum wins, NaN and +inf never do.  d_cost[u] is that D and the backtrack starts there.  If
 *   no cell wins the pair ends at (n - 1, m - 1) like a closed one, and its total is then not finite.  A is always matched whole; a
 *   caller who wants B whole inside A swaps the arguments.
 *   Maps: d_b_on_a as above (every row is on the path).  With j_first and j_last the columns of the path's first and last cell,
 *   d_a_on_b[j] is as above for j_first <= j <= j_last, 0.0 for j < j_first and (double)(n - 1) for j > j_last: the end frames are
 *   held, as wc_retime_parameters_device holds them for positions outside.
 * Further outputs (device arrays, each may be NULL on its own): d_span, two int32 per pair, (j_first, j_last), or (-1, -1) where the
 * total is not finite.  d_timeline_a, d_timeline_b: doubles packed like d_path (pair u from entry sum_{v<u} (a_length[v] +
 * b_length[v] - 1) on); entry k < K is (double)i_k and (double)j_k of the path's cell k; nothing is written behind K and nothing at
 * all where the total is not finite.  They are d_position_a and d_position_b of wc_morph_parameters_device with out_length = K:
 * the caller reads d_path_length back for that.
 * Refused (WC_ERR_INVALID, nothing written, nothing enqueued): what wc_align_features_device refuses; step_pattern outside {0, 1};
 * flags outside 0..3; flags != 0 with band != 0 (the band lies around the line between the corners and has no meaning for an open
 * end); under step_pattern == 1 more than 2^27 stored cells in all (it keeps d and D side by side: 17 bytes per stored cell, which
 * keeps the scratch within the 2.3 GB above; step_pattern 0 keeps 2^28).  The count is made on the host before the device is
 * touched.  Stream-ordered, enqueue-only. */
#define WC_ALIGN_OPEN_BEGIN 1 /* the path may start at any cell (0, j) */
#define WC_ALIGN_OPEN_END 2   /* the path may end at any cell (n - 1, j) */
int wc_align_features_ex_device(int n_pairs, const int *a_length, const double *d_feat_a, const int *b_length, const double *d_feat_b,
								int dims, int dim_begin, int dim_end, int band, int step_pattern, int flags, double *d_cost,
								int *d_path_length, int *d_path, double *d_b_on_a, double *d_a_on_b, int *d_span, double *d_timeline_a,
								double *d_timeline_b);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_IO_H */
