// Device helpers that the two sample-rate converters share (wc_resample.hip, wc_vresample.hip): the format loads and stores, the
// search of a block's record and the first half of a stream's push.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wc_pcm16.hpp"

namespace wc {
namespace {

constexpr int kPlainBlock = 256;

// one stream's new samples (resample_widen_kernel)
struct RsPush {
	long long c_off;      // first new sample in the packed chunk
	long long cur_off;    // the stream's buffer of this push, in doubles from the buffers' base
	long long other_off;  // the buffer of the next push
	int n_new;
	int block0;
};

template <int FMT> __device__ __forceinline__ double rs_load(const void *x, long long i);
template <> __device__ __forceinline__ double rs_load<0>(const void *x, long long i) { return static_cast<const double *>(x)[i]; }
template <> __device__ __forceinline__ double rs_load<1>(const void *x, long long i) { return pcm16_to_double(static_cast<const int16_t *>(x)[i]); }
template <> __device__ __forceinline__ double rs_load<2>(const void *x, long long i) { return static_cast<double>(static_cast<const float *>(x)[i]); }

__device__ __forceinline__ void rs_store(void *y, int out_format, long long i, double v) {
	if (out_format == 0) static_cast<double *>(y)[i] = v;
	else static_cast<int16_t *>(y)[i] = static_cast<int16_t>(pcm16_of(v));
}

// the record of block b: the last one whose block0 is not above b (block0 ascends, rec[0].block0 == 0)
template <class T> __device__ __forceinline__ int rs_find(const T *rec, int n, int b) {
	int lo = 0, hi = n - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (rec[mid].block0 <= b) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

// A stream's push, first half: the new samples widened behind the 2K of history in the buffer of this push, and the last 2K of
// (history, new samples) to the head of the other buffer.  Nothing that is read here is written here.
template <int FMT> __global__ __launch_bounds__(kPlainBlock) void resample_widen_kernel(const RsPush *push, int n_push, const void *chunk, double *buf, int hist) {
	const RsPush w = push[rs_find(push, n_push, (int)blockIdx.x)];
	const long long k = ((long long)blockIdx.x - w.block0) * kPlainBlock + threadIdx.x;
	if (k < w.n_new) {
		buf[w.cur_off + hist + k] = rs_load<FMT>(chunk, w.c_off + k);
	} else if (k < (long long)w.n_new + hist) {
		const long long b = k - w.n_new, s = w.n_new + b;
		buf[w.other_off + b] = s < hist ? buf[w.cur_off + s] : rs_load<FMT>(chunk, w.c_off + s - hist);
	}
}

}  // namespace
}  // namespace wc
