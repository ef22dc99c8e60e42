// Host-side internals shared by the C-ABI translation units: per-device state (stream, twiddle
// table, RNG draw table), grow-only device buffers, error reporting, kernel timing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/world_class_c.h"
#include "wc_stage_plan.hpp"  // UttDesc, the batch layout, the draw range

namespace wc {

void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

#define WC_HIP(expr)                                                                              \
	do {                                                                                          \
		hipError_t _e = (expr);                                                                   \
		if (_e != hipSuccess)                                                                     \
			return ::wc::fail(WC_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));  \
	} while (0)

// Grow-only device buffer.
struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	int reserve(size_t bytes);  // 0 on success
	void release();
	template <class T> T *as() const { return static_cast<T *>(p); }
};

// Pinned host staging buffer (grow-only).
struct HostBuf {
	void *p = nullptr;
	size_t cap = 0;
	hipEvent_t ev = nullptr;  // recorded after the async copies that read this buffer
	int reserve(size_t bytes);  // also waits until earlier async copies out of the buffer are done
	int mark(hipStream_t s);    // call after enqueueing the copies that read the buffer
	void release();
	template <class T> T *as() const { return static_cast<T *>(p); }
};

// The records of a stream handle's call and their way to the device: one device buffer and two page-locked stagings that take turns --
// a pair, so that a call waits for the copy of the call before the last only.  A call that has something to upload waits for the
// staging whose turn it is and takes its pointer (begin), writes its records there, and sends the used prefix up with one asynchronous
// copy (upload), which records the staging's event and hands the turn to the other one.  Nothing reads "the staging of this call"
// through the pair behind upload: the caller keeps the pointer begin gave it.
struct RecPair {
	DevBuf d;
	HostBuf h[2];
	int parity = 0;  // whose turn it is
	int reserve(size_t bytes) { return d.reserve(bytes) || h[0].reserve(bytes) || h[1].reserve(bytes); }  // 0 on success
	void release() { d.release(); h[0].release(); h[1].release(); }
	// nullptr on failure (the error is set); with a byte count, this call's staging and the device buffer grow to it first
	template <class T> T *begin(size_t bytes = 0) { return h[parity].reserve(bytes) || d.reserve(bytes) ? nullptr : h[parity].as<T>(); }
	template <class T> int upload(hipStream_t s, size_t bytes, const T **on_device) {
		HostBuf &hb = h[parity];
		WC_HIP(hipMemcpyAsync(d.p, hb.p, bytes, hipMemcpyHostToDevice, s));
		if (int rc = hb.mark(s)) return rc;
		parity = 1 - parity;
		*on_device = d.as<T>();
		return WC_OK;
	}
};

// host arrays <-> one packed device array: page-locked staging and its device twin (wc_batch.hip)
struct Staging {
	HostBuf h;
	DevBuf d;
};

// Per-device shared state.
struct Device {
	int id = 0;
	hipStream_t stream = nullptr;  // library-owned non-blocking stream: created once, never replaced
	// the stream this thread's calls enqueue on: the calling thread's wc_set_stream() stream, else `stream`
	hipStream_t active() const;
	// waits for everything on the device (handles are destroyed / the RNG table is replaced behind it: work that uses
	// their buffers may sit on the library stream, on a caller's stream or on the pipeline's side streams)
	void quiesce() const;
	// One public call at a time per device: the calls of several host threads that drive handles on the same device
	// are serialised (they share the RNG draw table, the timing events and the noise-stream position).
	std::recursive_mutex mu;
	double2 *twiddle = nullptr;  // kTwiddleN entries, e^{+2 pi i k / kTwiddleN}
	// RNG draw table: raw 12-step sums (uint32) of the reference's randn() for stream positions
	// [rng_base, rng_base + rng_count)
	DevBuf rng_table;
	uint64_t rng_base = 0, rng_count = 0;
	int ensure_rng(uint64_t first, uint64_t last_exclusive);  // makes [first, last) available
	// timing
	bool timing = false;
	int time_tag = -1;  // >= 0: events are keyed "name#tag" (the pipeline runs each kernel once per utterance group)
	std::map<std::string, std::pair<hipEvent_t, hipEvent_t>> events;
	int time_begin(const char *name, hipStream_t s = nullptr);  // nullptr = active()
	int time_end(const char *name, hipStream_t s = nullptr);
	// Staging of the host-pointer batch calls (wc_*_compute_batch): samples, time axis, contour, two row matrices, waveform.
	// Owned by the device, used under its call lock by whichever host thread calls, grown on demand and kept between calls
	// (a 64 x 10 s batch at 48 kHz holds ~1 GB of device and ~1 GB of page-locked memory per row matrix).  Released when the
	// last stage handle on the device is destroyed and by wc_release_scratch() -- never tied to a host thread's lifetime.
	Staging batch[6];
	// Scratch of wc_align_features_device (wc_align.hip): local costs / accumulated costs, choices and the backward path of one
	// call.  One buffer per device, used under the call lock; a call on another stream than the last one waits (on the device) for
	// align_done, recorded behind the last call's kernels.  Grown on demand, released with the batch staging.
	DevBuf align_scratch;
	hipEvent_t align_done = nullptr;
	hipStream_t align_last = nullptr;
	// Scratch of the model-feature calls (wc_features.hip): pack's continuous lf0 and gap ends, MLPG's parked l1, l2 and z / d.  Kept
	// and handed from stream to stream like align_scratch.
	DevBuf features_scratch;
	hipEvent_t features_done = nullptr;
	hipStream_t features_last = nullptr;
	int live_handles = 0;  // stage handles alive on this device (under mu)
	void handle_born();
	void handle_gone();  // the last one takes the batch staging with it
	void release_batch_staging();
};

Device *current_device();  // creates the state on first use; nullptr + error on failure
// RAII: a handle that creates a helper handle of its own on first use (a twin, a pipeline group) does so on ITS device, whatever the
// calling thread's wc_set_device says (thread-local; the compute entry points run a handle on its own device anyway)
struct OnDeviceOf {
	int prev;
	explicit OnDeviceOf(const Device *d);
	~OnDeviceOf();
};
// process-wide noise-stream position of the host-pointer calls (atomic: handles on different devices share it)
uint64_t global_rng_position();
void set_global_rng_position(uint64_t position);
// RAII: serialises the public calls on one device
struct DeviceLock {
	std::unique_lock<std::recursive_mutex> lk;
	explicit DeviceLock(Device *d) : lk(d->mu) {}
};

// host-side RNG jump-ahead (GF(2) linear algebra on the xorshift128 state)
void rng_state_at(uint64_t position, uint32_t state[4]);

// device entry points implemented in the .hip files
int launch_rng_fill(Device *dev, uint32_t *table, uint64_t first, uint64_t count);

// Frame filtering's segments (wc_filter.hip), which the batch and the filter streams (wc_filter_stream.hip) place by the same record.
// One per utterance -- for a stream: per stream that a push touches -- and one more behind the last whose seg_off is the call's segment
// count.  t0 is the number of the record's first segment (the batch: 0).  x_off and row_off lead to the sample a_t0 and to row t0: n
// and f_len count from there, and so do the segment's own offsets.  A segment past f_len reads row f_len - 1, the held one; with
// f_len == 0 that is the row in front of row_off.
struct FfUtt {
	long long x_off, row_off, seg_off;
	int n, f_len, S, t0;
};
struct FfArgs {
	const double *x, *gain;
	double *rows, *y;
	const FfUtt *utts;
	const double2 *tw;
	long long total_seg;
	double fp_ms;
	int n_utt, fs, kind;
};
// the response rows of a.total_seg segments into a.rows, enqueued on s: the one-wavefront kernel at fft_size 1024 / 2048 unless block
// is set, the workgroup-per-segment kernel otherwise (arguments already checked)
int filter_segments_launch(Device *dev, hipStream_t s, int fft_size, bool block, const FfArgs &a);
// the coded call's d = to - from over total values in rows of nd (from == nullptr: d = to; skip_energy: d[0] of a row is 0.0)
int filter_difference_launch(hipStream_t s, const double *d_to, const double *d_from, double *d_diff, long long total, int nd, int skip_energy);

}  // namespace wc
