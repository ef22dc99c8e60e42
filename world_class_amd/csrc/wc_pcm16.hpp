// The sample conversions at the int16 boundary, stated once for wc_io.hip (wavwrite, wc_*_pcm16_*_device) and wc_resample.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

namespace wc {

// wavwrite's sample conversion: static_cast<int>(x * 32767) on the reference's platform (x86 cvttsd2si: NaN and
// out-of-range values become INT_MIN), then clamp to int16
__host__ __device__ inline int pcm16_of(double x) {
	const double v = x * 32767;
	int iv;
	if (!(v > -2147483649.0 && v < 2147483648.0)) iv = INT_MIN;
	else iv = static_cast<int>(v);
	return iv < -32768 ? -32768 : (iv > 32767 ? 32767 : iv);
}

// wavread's: the sample over 32768
__host__ __device__ inline double pcm16_to_double(int16_t p) { return static_cast<double>(p) / 32768.0; }

}  // namespace wc
