/* ---- Coded track-morph streams: wc_track_morph with its tracks, its ring and its live rows held as coded features (extension) ----
 *
 * A header of its own that includes world_class_stream.h and world_class_codec.h; world_class_stream.h does not include it.  Its
 * binding table in the Python mirror is TRACK_MORPH_CODED_SIGNATURES (world_class_amd/stream.py).
 *
 * wc_track_morph (world_class_track_morph.h) morphs a live voice with a resident track at positions it reads in device memory, and
 * is the one link of the live chain (analysis stream -> coded rows -> alignment stream -> track morph -> synthesis stream) that
 * takes full rows: 2 * (fft_size/2 + 1) + 1 doubles per track row and ring slot, where everything in front of it lives on
 * number_of_dimensions + GetNumberOfAperiodicities(fs) coded doubles per frame.  wc_track_morph_coded is that handle with coded
 * tracks, a coded ring and coded inputs: the two device arrays of coded track rows that went to wc_align_stream_set_track_device
 * and the coded live rows that go to wc_align_stream_push_settled_device go to this handle as they are.  Its OUTPUTS stay full
 * rows (F0, sp row, ap row of fft_size/2+1), which is what wc_synth_stream_push_device takes: the morph aligns formants on the
 * envelope itself, so there is no blend in the cepstral domain.
 *
 * Layout.  A coded sp row is number_of_dimensions doubles (nd; fixed at create), a coded ap row is n_ap = GetNumberOfAperiodicities(fs)
 * doubles, as wc_code_features_device writes them.  d_coded_sp_* / d_coded_ap_* hold them row after row, the rows of a push packed
 * stream by stream by n_a[u] exactly as wc_track_morph_push_device packs its full rows; d_f0_*, d_position_b, d_tail and the three
 * outputs are those of wc_track_morph.  Coded rows need 8-byte alignment only.
 *
 * The rule is wc_track_morph's, unchanged, with the coded arrays in the place of the full ones: tracks (n_tracks slots of
 * max_track_frames rows; wc_track_morph_coded_set_track_device copies m coded rows and their F0 into a slot, stream-ordered, refused
 * while a stream that has received rows is attached), wc_track_morph_coded_reset(h, stream, track, delay) with the delay D, 0 <= D <=
 * max_delay, the weight / F0 weight / ratios per stream that take effect at the next call, and per pushed row i since the reset:
 *   i <  D   the row forms nothing and its entry of d_position_b is not read;
 *   i >= D   the row forms output frame t = i - D from A's row t and the track at the entry of row i.
 * frames_out[u] = max(n + n_a[u] - D, 0) - max(n - D, 0) from counts alone; no host code looks at a position.  The flush takes
 * d_tail as wc_align_stream_tail_device writes it (K = min(D + 1, n) doubles per wanted stream), forms the last min(D, n) frames and
 * ends the stream.  The outputs hold n_streams x max_frames_per_push rows (a push) / n_streams x max_delay rows (the flush).
 *
 * Bit identity.  Every formed frame equals, bit for bit, the frame a wc_track_morph handle of the same shape forms whose track is
 * wc_decode_features_device (world_class_codec.h) of the coded track, whose live rows are wc_decode_features_device of the coded
 * live rows, and which sees the same counts, positions, delays, weights and ratios.  By that handle's contract the frame is
 * therefore frame t of wc_morph_parameters_device on the decoded pair -- with its clamp of the position to [0, m - 1], its frame
 * that is NaN throughout for a position that is not finite, positions that fall, jump or repeat, and no dependence on other streams
 * or on how the rows are cut into pushes.  This holds at every fft_size because the library's one decoder decodes
 * (wc::decode_features_enqueue: the one-wavefront kernel at 2048, the two workgroup kernels at 512 / 1024 / 4096), and a row's
 * decoded bits depend on that row alone.
 *
 * A push or flush with frames to form enqueues, on the caller's stream (wc_set_stream) and in this order: the one asynchronous copy
 * of the records (48 bytes per stream, 16 per formed frame, 8 per kept row, out of a pair of page-locked staging buffers);
 * track_gather_coded_kernel, which reads each frame's position, places it in the track and copies the three coded rows the frame
 * needs -- A's row t, track rows i and j, all inside the arrays whatever the position holds -- into slots 3g, 3g + 1, 3g + 2 of the
 * handle's scratch, and copies the rows to keep into their ring slots; the decoder over the 3 x frames scratch slots; and
 * track_morph_coded_kernel, wc_track_morph's blend on the decoded slots (its variant without shared memory while no stream that
 * forms frames has a ratio).  A push that only keeps rows enqueues the copy and the gather alone.  No call makes a device-to-host
 * copy or synchronises; wc_track_morph_coded_create builds the decoding plan of (fs, fft_size), so no push is the first use that
 * may wait for the device.  A handle is driven on one stream at a time.
 *
 * The ring is wc_track_morph's: slot number % cap, cap = max_delay + min(max_delay, max_frames_per_push), so a push never writes a
 * slot the state before it needs and a push that fails on the device leaves the host state and the kept rows of the last good push.
 *
 * Memory.  wc_track_morph_coded_create allocates everything, every device array once and exactly, each rounded up to 256 bytes
 * (A(x) below).  With bins = fft_size/2 + 1, T = n_tracks x max_track_frames, S = n_streams x cap, F = n_streams x
 * max(max_frames_per_push, max_delay):
 *   tracks    A(8 T) + A(8 T nd) + A(8 T n_ap)
 *   ring      A(8 S) + A(8 S nd) + A(8 S n_ap)                        (nothing when max_delay = 0)
 *   scratch   A(24 F nd) + A(24 F n_ap) + 2 A(24 F bins)              (3 F slots: the coded rows and both decoded rows)
 *   records   A(48 n_streams + 16 F + 8 n_streams min(max_delay, max_frames_per_push))
 * wc_track_morph_coded_device_bytes returns their sum; the records' two page-locked staging buffers are host memory.  A track row
 * or ring slot is 1 + nd + n_ap doubles instead of 1 + 2 bins: 64 instead of 1027 at 24 kHz / fft 1024 / nd = 60, 66 instead of
 * 2051 at 48 kHz / fft 2048 / nd = 60.  The scratch is now the large item and grows with the rows a CALL may form, not with what is
 * resident: 512 streams x 50 rows per push at fft 1024, nd = 60 is 76 800 slots of 1 089 doubles = 669 MB (638 MiB); the same
 * streams at 1 row per push and max_delay = 20 are 30 720 slots = 268 MB, at max_delay = 1 they are 13 MB.
 *
 * Refused with WC_ERR_INVALID on the host before anything is enqueued, every stream, setting and kept row as it was: all that
 * wc_track_morph refuses -- a bad stream or track index; a count that is negative or above max_frames_per_push; rows for a stream
 * that is not attached or has ended; NULL arrays with rows to read, positions to read or frames to write; a NULL n_a, want or
 * frames_out; a delay out of range; a reset onto a slot that has not been set; set_track_device with m out of range, a NULL array
 * or a stream with rows attached; a weight or F0 weight that is not finite; a ratio that is neither 0 nor finite and >= 2.0 /
 * fft_size; a flush with a wanted stream that is not attached, has ended, has D = 0 or has no rows.  wc_track_morph_coded_create
 * returns NULL for what wc_track_morph_create refuses (fft_size outside 512 / 1024 / 2048 / 4096, fs <= 0, a count below 1,
 * max_delay < 0, sizes past 2^31 - 1 rows, here also 3 F) and for what the decoder refuses: number_of_dimensions outside
 * 1 .. fft_size/2, fs below 12 kHz (no aperiodicity band). */
#ifndef WORLD_CLASS_TRACK_MORPH_CODED_H
#define WORLD_CLASS_TRACK_MORPH_CODED_H

#include "world_class_stream.h"
#include "world_class_codec.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wc_track_morph_coded wc_track_morph_coded;
wc_track_morph_coded *wc_track_morph_coded_create(int fs, int fft_size, int number_of_dimensions, int n_streams, int n_tracks,
                                                  int max_track_frames, int max_frames_per_push, int max_delay);
void wc_track_morph_coded_destroy(wc_track_morph_coded *h);
int wc_track_morph_coded_set_track_device(wc_track_morph_coded *h, int track, int m, const double *d_f0_b, const double *d_coded_sp_b,
                                          const double *d_coded_ap_b);
int wc_track_morph_coded_reset(wc_track_morph_coded *h, int stream, int track, int delay);
int wc_track_morph_coded_set_weight(wc_track_morph_coded *h, int stream, double weight, double f0_weight);
int wc_track_morph_coded_set_ratios(wc_track_morph_coded *h, int stream, double ratio_a, double ratio_b);
int wc_track_morph_coded_push_device(wc_track_morph_coded *h, const int *n_a, const double *d_f0_a, const double *d_coded_sp_a,
                                     const double *d_coded_ap_a, const double *d_position_b, double *d_f0_out, double *d_sp_out,
                                     double *d_ap_out, int *frames_out);
int wc_track_morph_coded_flush_device(wc_track_morph_coded *h, const int *want, const double *d_tail, double *d_f0_out, double *d_sp_out,
                                      double *d_ap_out, int *frames_out);
/* rows of A received / frames formed so far; -1 for a bad index */
long long wc_track_morph_coded_frames_received(const wc_track_morph_coded *h, int stream);
long long wc_track_morph_coded_frames_formed(const wc_track_morph_coded *h, int stream);
int wc_track_morph_coded_pending(const wc_track_morph_coded *h, int stream); /* rows of A kept, not yet formed; -1 for a bad index */
int wc_track_morph_coded_get_delay(const wc_track_morph_coded *h, int stream); /* -1: bad index */
int wc_track_morph_coded_track_length(const wc_track_morph_coded *h, int track);
/* what create allocated on the device: tracks + ring + scratch + records (the formula above); -1 for a NULL handle */
long long wc_track_morph_coded_device_bytes(const wc_track_morph_coded *h);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_TRACK_MORPH_CODED_H */
