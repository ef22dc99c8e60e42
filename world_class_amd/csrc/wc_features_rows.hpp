// What the translation units of the model features share (wc_features.hip, wc_mlpg_stream.hip, wc_feature_stream.hip): which F0
// counts as voiced, where a static column stands in a row of include/world_class_features.h, and the host's test of two byte ranges.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

namespace wc {

// a frame is voiced iff 0 < f0 <= DBL_MAX: NaN, negatives, 0 and +inf are unvoiced
__device__ __forceinline__ bool ft_voiced(double f) { return f > 0.0 && f <= DBL_MAX; }

// the static column c < S = nd + 1 + n_ap of a row: where its order 0 stands, and the step from one order to the next
__device__ __forceinline__ void ft_column(int c, int nd, int n_ap, int orders, int *col0, int *cstep) {
	if (c < nd) { *col0 = c; *cstep = nd; }
	else if (c == nd) { *col0 = orders * nd; *cstep = 1; }
	else { *col0 = orders * (nd + 1) + 1 + (c - nd - 1); *cstep = n_ap; }
}

// whether two device ranges share a byte; a NULL or empty range shares none
inline bool overlap(const void *a, unsigned long long a_bytes, const void *b, unsigned long long b_bytes) {
	if (!a || !b || !a_bytes || !b_bytes) return false;
	const unsigned long long x = (unsigned long long)(uintptr_t)a, y = (unsigned long long)(uintptr_t)b;
	return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace wc
