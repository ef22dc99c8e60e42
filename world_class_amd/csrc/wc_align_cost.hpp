// The local costs of feature alignment, shared by the whole-utterance calls (wc_align.hip) and the alignment streams
// (wc_align_stream.hip): the pair descriptors, the band's row ranges and align_cost_kernel.  One kernel for both, so that the
// rounding of d(i, j) -- ascending c from 0.0; difference, product and sum rounded apart (-ffp-contract=off); the correctly rounded
// root -- cannot drift apart between a stream's rows and the call they are held against.
// al_cell_costs is the same arithmetic per cell for the one caller whose columns are decided on the device (the windowed streams).
#pragma once
#include <hip/hip_runtime.h>

namespace wc {

constexpr int AL_TILE = 32;                   // rows of A and rows of B per workgroup of the cost pass
constexpr int AL_KC = 32;                     // coefficients per trip through LDS
constexpr int AL_CHUNK = 8;                   // cells a lane of the accumulation loads ahead of its chain

struct AlPair {
	long long a_off, b_off;  // first row of A / of B in the packed arrays (also first frame of the maps)
	long long cell_off;      // first stored cell
	long long path_off;      // first path entry
	long long tile_off;      // first workgroup of the cost pass
	long long B;             // band * L, or -1: every cell is allowed
	int n, m;                // rows of A / of B
	int W;                   // stored cells per row
	int tiles_j;             // cost tiles per block of 32 rows
};

struct AlArgs {
	const AlPair *pairs;
	int n_pairs, dims, dim_begin, dim_end;
	const double *fa, *fb;
	double *cells;           // d(i, j), then D(i, j) in place
	unsigned char *choice;   // 0 diagonal, 1 up, 2 left
	int2 *back;              // the path backwards
	double *cost;
	int *path_length;
	int2 *path;
	double *b_on_a, *a_on_b;
};

// the allowed columns [lo, hi] of row i: |i * (m - 1) - j * (n - 1)| <= B in 64-bit integers, solved for j
__device__ __forceinline__ void al_row(const AlPair &u, int i, int &lo, int &hi) {
	if (u.B < 0 || u.n == 1) {
		lo = 0; hi = u.m - 1;
		return;
	}
	const long long q = u.n - 1, x = (long long)i * (u.m - 1);
	const long long l = x - u.B, h = (x + u.B) / q;
	lo = l <= 0 ? 0 : (int)((l + q - 1) / q);
	hi = h > u.m - 1 ? u.m - 1 : (int)h;
}

// d(i, j) of N cells by one lane, for a caller that cannot go through the kernel below (the windowed alignment streams, whose columns
// are decided on the device): a[k] and b[k] point at the two rows of cell k.  Per cell it is the kernel's arithmetic: ascending c from
// 0.0, the difference, the product and the sum rounded apart, the correctly rounded root; the N chains only hide each other's loads.
template <int N>
__device__ __forceinline__ void al_cell_costs(const double *const (&a)[N], const double *const (&b)[N], int dim_begin, int dim_end,
                                              double (&out)[N]) {
	double acc[N];
#pragma unroll
	for (int k = 0; k < N; ++k) acc[k] = 0.0;
	for (int c = dim_begin; c < dim_end; ++c) {
#pragma unroll
		for (int k = 0; k < N; ++k) {
			const double d = a[k][c] - b[k][c];
			acc[k] = acc[k] + d * d;
		}
	}
#pragma unroll
	for (int k = 0; k < N; ++k) out[k] = __dsqrt_rn(acc[k]);
}

static __global__ __launch_bounds__(256) void align_cost_kernel(AlArgs A) {
	__shared__ double sa[AL_TILE][AL_KC + 1], sb[AL_TILE][AL_KC + 1];
	const int tid = threadIdx.x;
	const long long g = blockIdx.x;
	int plo = 0, phi = A.n_pairs;
	while (phi - plo > 1) {
		const int mid = (plo + phi) >> 1;
		if (A.pairs[mid].tile_off <= g) plo = mid;
		else phi = mid;
	}
	const AlPair u = A.pairs[plo];
	const long long t = g - u.tile_off;
	const int i0 = (int)(t / u.tiles_j) * AL_TILE;
	if (i0 >= u.n) return;
	const int i_last = min(i0 + AL_TILE - 1, u.n - 1);
	int lo0, hi0, lo1, hi1;
	al_row(u, i0, lo0, hi0);
	al_row(u, i_last, lo1, hi1);
	const long long j0l = (long long)lo0 + (t % u.tiles_j) * AL_TILE;
	if (j0l > hi1) return;  // (the whole workgroup: lo and hi do not fall with i)
	const int j0 = (int)j0l;
	const int tx = tid & (AL_TILE - 1), ty = tid >> 5;
	double acc[4] = {0.0, 0.0, 0.0, 0.0};
	for (int c0 = A.dim_begin; c0 < A.dim_end; c0 += AL_KC) {
		const int kc = min(AL_KC, A.dim_end - c0);
		for (int e = tid; e < AL_TILE * AL_KC; e += 256) {
			const int r = e >> 5, c = e & (AL_KC - 1);
			const bool in = c < kc;
			sa[r][c] = in && i0 + r < u.n ? A.fa[(u.a_off + i0 + r) * A.dims + c0 + c] : 0.0;
			sb[r][c] = in && j0 + r < u.m ? A.fb[(u.b_off + j0 + r) * A.dims + c0 + c] : 0.0;
		}
		__syncthreads();
		for (int c = 0; c < kc; ++c) {
			const double b = sb[tx][c];
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const double d = sa[ty + 8 * k][c] - b;
				acc[k] = acc[k] + d * d;
			}
		}
		__syncthreads();
	}
	const int j = j0 + tx;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const int i = i0 + ty + 8 * k;
		if (i >= u.n || j >= u.m) continue;
		int lo, hi;
		al_row(u, i, lo, hi);
		if (j < lo || j > hi) continue;
		A.cells[u.cell_off + (long long)i * u.W + (j - lo)] = __dsqrt_rn(acc[k]);
	}
}

}  // namespace wc
