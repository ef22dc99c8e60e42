// gmm_ll_kernel, the table of ll(t, m) of THE rule of convert (include/world_class_gmm.h), for the two translation units that evaluate
// a mixture: wc_gmm.hip on the source part of a joint model, wc_gmm_train.hip on the whole joint vector (a GmmDev of width D).  What
// the kernel does and why stands at the head of wc_gmm.hip.  Everything here has internal linkage: each translation unit owns its
// instantiations, so a hipFuncSetAttribute on one is of no concern to the other.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kTile = 64, kPitch = kTile + 1, kRows = 16, kWaves = 8;
static_assert(kRows == 16, "gmm_q cuts the rest of the rows into blocks of 16, 8 and 4");

struct GmmDev {
	const double *Wt;   // [m][k][i]: W_m(i,k), 0.0 where i < k
	const double *Bt;   // [m][k][j]: B_m(j,k)
	const double *mux, *muy, *c, *cvar;
	int n_mix, dx, dy;
};

// rows i0 .. i0 + R - 1 of z for this lane's frame, and their squares added to q in ascending i; xl: the lane's column of the tile
// (x(k) at xl[k * kPitch])
template <int R>
__device__ __forceinline__ double gmm_rows(const double *__restrict__ Wm, const double *__restrict__ mu, const double *xl, int dx, int i0, double q) {
	double z[R];
	const double *w = Wm + i0;
	double dk = xl[0] - mu[0];
#pragma unroll
	for (int r = 0; r < R; ++r) z[r] = w[r] * dk;
#pragma unroll 2
	for (int k = 1; k <= i0; ++k) {  // columns 1 .. i0 reach all R rows
		w += dx;
		dk = xl[k * kPitch] - mu[k];
#pragma unroll
		for (int r = 0; r < R; ++r) z[r] = z[r] + w[r] * dk;
	}
	// the triangle: column i0 + j reaches rows i0 + j .. i0 + R - 1.  (Rows at and past dx read what lies behind them and are dropped.)
#pragma unroll
	for (int j = 1; j < R; ++j) {
		if (i0 + j < dx) {
			w = Wm + (size_t)(i0 + j) * dx + i0;
			dk = xl[(i0 + j) * kPitch] - mu[i0 + j];
#pragma unroll
			for (int r = j; r < R; ++r) z[r] = z[r] + w[r] * dk;
		}
	}
#pragma unroll
	for (int r = 0; r < R; ++r)
		if (i0 + r < dx) q = i0 + r == 0 ? z[r] * z[r] : q + z[r] * z[r];
	return q;
}

// q of one mixture: blocks of kRows rows, the rest in the narrowest block that holds it
__device__ __forceinline__ double gmm_q(const double *__restrict__ Wm, const double *__restrict__ mu, const double *xl, int dx) {
	double q = 0.0;
	int i0 = 0;
	for (; i0 + kRows <= dx; i0 += kRows) q = gmm_rows<kRows>(Wm, mu, xl, dx, i0, q);
	const int rest = dx - i0;
	if (rest > 8) q = gmm_rows<kRows>(Wm, mu, xl, dx, i0, q);
	else if (rest > 4) q = gmm_rows<8>(Wm, mu, xl, dx, i0, q);
	else if (rest > 0) q = gmm_rows<4>(Wm, mu, xl, dx, i0, q);
	return q;
}

// table: ll of frame t0 at its start
template <class T>
__global__ __launch_bounds__(kTile * kWaves) void gmm_ll_kernel(GmmDev g, long long t0, long long n_end, const T *__restrict__ rows, int ld_in,
																  int col_in, int per, double *__restrict__ table) {
	extern __shared__ __attribute__((aligned(16))) double gmm_x[];  // dx * kPitch
	const int tid = threadIdx.x, dx = g.dx;
	const long long tbase = t0 + (long long)blockIdx.x * kTile;
	for (int idx = tid; idx < kTile * dx; idx += kTile * kWaves) {
		const int ff = idx / dx, col = idx - ff * dx;
		const long long t = tbase + ff;
		gmm_x[col * kPitch + ff] = t < n_end ? (double)rows[(size_t)t * ld_in + col_in + col] : 0.0;
	}
	__syncthreads();
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
	const int m_begin = blockIdx.y * per, m_end = m_begin + per < g.n_mix ? m_begin + per : g.n_mix;
	const long long t = tbase + lane;
	const double *xl = gmm_x + lane;
	for (int m = m_begin + wave; m < m_end; m += kWaves) {
		const double q = gmm_q(g.Wt + (size_t)m * dx * dx, g.mux + (size_t)m * dx, xl, dx);
		const double ll = g.c[m] - 0.5 * q;
		if (t < n_end) table[(size_t)(t - t0) * g.n_mix + m] = ll;
	}
}

size_t gmm_lds_bytes_of(int dx) { return (size_t)dx * kPitch * sizeof(double); }

// the launch of gmm_ll_kernel over frames [t0, t0 + nc) of a call of n_end frames: the mixtures are cut into shares of whole eights
// (a wavefront each) where the tiles alone leave compute units idle
template <class T>
void gmm_ll_launch(const GmmDev &dv, int cus, hipStream_t s, long long t0, long long nc, long long n_end, const T *rows, int ld_in, int col_in,
				   double *table) {
	const int n_mix = dv.n_mix;
	const long long tiles = (nc + kTile - 1) / kTile, want = 4ll * cus;
	long long split = (want + tiles - 1) / tiles;
	const long long most = (n_mix + kWaves - 1) / kWaves;
	split = split < 1 ? 1 : (split > most ? most : split);
	const int per = (int)(((n_mix + split - 1) / split + kWaves - 1) / kWaves * kWaves);
	const dim3 grid((unsigned)tiles, (unsigned)((n_mix + per - 1) / per));
	hipLaunchKernelGGL(gmm_ll_kernel<T>, grid, dim3(kTile * kWaves), gmm_lds_bytes_of(dv.dx), s, dv, t0, n_end, rows, ld_in, col_in, per, table);
}

}  // namespace
