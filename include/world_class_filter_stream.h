/* ---- Filter streams: frame filtering push by push, the whole call's bits (extension) ----
 *
 * Frame filtering (world_class_filter.h) shapes a waveform by one gain row per frame without the vocoder, and needs the whole utterance.
 * A filter stream takes the samples and the rows of a live voice as they arrive and commits outputs as soon as the rule allows it.  It
 * is the last member of the live chain: analysis stream (coded push) -> feature stream -> GMM conversion -> MLPG stream -> filter
 * stream (coded push), where a synthesis stream would stand.  A header of its own with a binding table of its own in the Python mirror
 * (world_class_amd/filter_stream.py: FILTER_STREAM_SIGNATURES); tests/filter_stream_rule.py states THE rule in numpy on
 * tests/filter_rule.py.
 *
 * Notation.  c_t, a_t, N, h, S, the kinds and the rows are those of world_class_filter.h.  Stream u has received n samples and F rows
 * since its reset.
 *
 * THE rule.
 *   Segments done.  T(n, F) is the largest T with 0 <= T <= F and c_T <= n (wc_filter_stream_segments_done).  Segment t is done when
 *               row t is in and every sample below c_{t+1} is in.  A stream never holds a row before the flush: it cannot know that no
 *               further row comes.
 *   Committed.  C(T) = T ? c_{T-1} + 1 : 0, which is a_T (wc_filter_stream_committed).  T and C are host arithmetic on counts alone.
 *   A push      gives stream u n_samples[u] samples and n_rows[u] rows.  Either count may be 0; rows may run ahead of samples, and
 *               samples ahead of rows.  It computes segments T_before .. T_after - 1, writes y[C_before .. C_after), and
 *               samples_out[u] = C_after - C_before is filled before the call returns.
 *   The flush   is a flag per stream in the push (flush may be NULL: no stream is flushed).  It takes that push's samples and rows
 *               first.  It then computes the remaining segments T .. S - 1 as the whole call does at n_total = n:
 *               b_t = min(n - 1, c_{t+1} - 1) and row min(t, F - 1); the last row is held, and rows from S on are not read.  It writes
 *               y[C .. n).  Afterwards the stream has ended until its reset; a flush flag for a stream that has ended does nothing.  A
 *               flush with n > 0 and F == 0 is refused.  A flush with n == 0 writes nothing.
 *   Bit identity.  For any cut into pushes, the concatenated outputs, flush included, equal one whole call on (x[0..n), rows[0..F),
 *               kind), bit for bit: wc_frame_filter_run_device for a plain-push stream, wc_frame_filter_run_coded_device for a
 *               coded-push stream.  A row with a value that is not finite turns the N samples from its a_t into NaN and nothing else,
 *               across push borders too.  No stream's outputs depend on another stream or on the launch shape.
 *   Latency.    With its rows in, a stream is at most 2 ceil(h) - 2 samples behind its newest sample: 78 at hop 40, 1022 at hop 512,
 *               128 at the tie hop 64.49999999999999.
 *
 * State per stream.  The whole call forms y[k] from 0.0 by adding r_t[k - a_t] with t ascending.  The stream carries a tail of N partial
 * sums behind C: the sums over the done segments, in that same order.  Later segments add onto the tail, so the additions and their
 * order are the whole call's.  It also carries a window of pending samples x[a_T .. n) and a window of pending rows T .. F - 1 (and,
 * beside them, the last row a done segment used: the row a flush holds when no row is pending).  Capacities are fixed at create:
 * max_pending_samples and max_pending_rows.  A push is accepted if, for every stream, pending-before plus pushed fits both; the new
 * window is assembled before any segment is consumed.  So samples_out[u] <= max_pending_samples, and d_y holds n_streams x
 * max_pending_samples doubles, packed by samples_out.  With max_pending_samples >= 2 ceil(h) a stream whose sample window is full is
 * waiting for rows, so a push of rows alone is accepted and no state is a dead end.  Tails and windows are kept in pairs: a push reads
 * one and writes the other, and a refused or failed push leaves every stream as it was.  Counters are 64-bit on the host; a push that
 * would take a stream past 2^31 - 1 samples is refused (the rule's lengths are int).  A reset clears the tail: a stream after a reset
 * behaves as a fresh one.  A stream is fresh at create.
 *
 * Layout.  d_x is packed by n_samples, d_rows (fft_size/2+1 doubles per row, of the handle's kind) and the coded rows
 * (number_of_dimensions doubles per row) by n_rows, d_y by samples_out.  The coded push forms d = to - from as the batch's coded call
 * does, decodes the pushed rows into the handle's scratch and runs the plain path: the pending rows are kept decoded.  Its handle's
 * kind must be WC_FILTER_POWER.
 *
 * A push only enqueues, on wc_set_stream's stream: one asynchronous copy of the records and a number of launches that does not depend on
 * the number of streams; no device-to-host copy and no synchronisation.  The handle lives on the device that is current at create; one
 * handle serves one call at a time (a call on another stream waits, on the device, for the handle's last call), and two host threads
 * on two handles run side by side.  Scratch: the response rows of a push (segments of this push x fft_size doubles) and, for the coded
 * push, the difference and the decoded rows of the push.  It lives in the handle, grows on demand and goes with it.
 *
 * Refusals.  Create returns NULL, the others WC_ERR_INVALID; the text is in wc_last_error.  Each happens before anything is enqueued,
 * and every stream stays as it was.  Create refuses: everything wc_frame_filter_create refuses; a kind outside {0, 1}; n_streams < 1;
 * max_pending_samples < 2 ceil(h); max_pending_rows < 1; byte counts that leave 63 bits.  A push refuses: a NULL handle, n_samples,
 * n_rows or samples_out; a negative count; a count that does not fit the windows; samples or rows for a stream that has ended; NULL
 * arrays with work to do; d_y overlapping any input; a flush with n > 0 and F == 0; the 2^31 - 1 limit.  The coded push also refuses:
 * number_of_dimensions outside 1 .. fft_size/2; a NULL d_coded_to; a handle whose kind is WC_FILTER_LOG.  The counters return -1 for a
 * bad index, and so do the two host functions for arguments create would refuse. */
#ifndef WORLD_CLASS_FILTER_STREAM_H
#define WORLD_CLASS_FILTER_STREAM_H

#include "world_class_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wc_filter_stream wc_filter_stream;

/* T and C of the rule; pure host */
long long wc_filter_stream_segments_done(int fs, double frame_period_ms, long long n, long long rows);
long long wc_filter_stream_committed(int fs, double frame_period_ms, long long segments_done);

wc_filter_stream *wc_filter_stream_create(int fs, int fft_size, double frame_period_ms, int kind, int n_streams,
                                          int max_pending_samples, int max_pending_rows);
void wc_filter_stream_destroy(wc_filter_stream *h);
int wc_filter_stream_reset(wc_filter_stream *h, int stream);

int wc_filter_stream_push_device(wc_filter_stream *h, const int *n_samples, const double *d_x, const int *n_rows,
                                 const double *d_rows, const int *flush, double *d_y, int *samples_out);
int wc_filter_stream_push_coded_device(wc_filter_stream *h, const int *n_samples, const double *d_x, const int *n_rows,
                                       const double *d_coded_to, const double *d_coded_from, int number_of_dimensions,
                                       int skip_energy, const int *flush, double *d_y, int *samples_out);

long long wc_filter_stream_samples_received(const wc_filter_stream *h, int stream);
long long wc_filter_stream_rows_received(const wc_filter_stream *h, int stream);
long long wc_filter_stream_segments_done_of(const wc_filter_stream *h, int stream);
long long wc_filter_stream_samples_committed(const wc_filter_stream *h, int stream);
int wc_filter_stream_pending_samples(const wc_filter_stream *h, int stream);
int wc_filter_stream_pending_rows(const wc_filter_stream *h, int stream);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_FILTER_STREAM_H */
