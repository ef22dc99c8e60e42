// Feature alignment (include/world_class_io.h: wc_align_features_device): dynamic time warping of a packed batch of pairs of
// feature sequences to the time maps that retime and morph take.  Three launches for the whole batch, all bounded by lengths the
// host wrote into the descriptors:
//
//   align_cost_kernel   fully parallel: a workgroup of 256 fills a tile of 32 rows of A x 32 rows of B with the local costs
//     d(i, j).  The coefficients go through LDS 32 at a time (any dims), a lane holds four cells and adds to each in ascending c, one
//     dependent chain per cell (difference, product, sum: rounded apart, -ffp-contract=off), then the correctly rounded root.  Under a
//     band a pair stores W cells per row, W the widest row the band can have, row i from its first allowed column lo(i) on; the
//     tiles of a block of 32 rows start at that block's first allowed column, so the grid grows with the stored cells, not with
//     n * m, and a tile wholly outside the band leaves at once.
//   align_accumulate_kernel   one 64-lane wavefront per pair, no barrier, no LDS.  Lane l owns the strip of ceil(m / 64) columns
//     from l * ceil(m / 64) and works on row s - l at step s, so lane l - 1 has finished that row's strip to the left one step
//     before: it hands D at its strip's right edge to lane l through one cross-lane move per step (the value of the step before is
//     the diagonal neighbour).  Within a strip the lane walks left to right, eight cells per round: the eight local costs and the
//     eight D of the row above (which this lane wrote itself one step earlier -- D overwrites d in place) are loaded together, then
//     the dependent chain of three comparisons and one sum per cell runs on registers.  One byte per cell records the choice.
//   align_path_kernel   one wavefront per pair: lane 0 follows the choices back from (n - 1, m - 1), at most n + m - 1 steps,
//     writes the cells backwards into scratch and each row's / column's (min + max) * 0.5 as it leaves it; then all lanes turn the
//     K cells into forward order.  A total that is not finite writes NaN maps and K = 0 instead.
//
//   The descriptors go up through page-locked staging kept per (device, stream); the scratch is the device's (Device::align_scratch).
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

#include "../../include/world_class_c.h"
#include "../../include/world_class_io.h"
#include "wc_stages.hpp"

using namespace wc;

namespace {

constexpr int AL_TILE = 32;                   // rows of A and rows of B per workgroup of the cost pass
constexpr int AL_KC = 32;                     // coefficients per trip through LDS
constexpr int AL_CHUNK = 8;                   // cells a lane of the accumulation loads ahead of its chain
constexpr long long kAlignMaxCells = 1ll << 28;  // stored cells per call (world_class_io.h)

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

__global__ __launch_bounds__(256) void align_cost_kernel(AlArgs A) {
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

__global__ __launch_bounds__(64) void align_accumulate_kernel(AlArgs A) {
	const AlPair u = A.pairs[blockIdx.x];
	const int lane = threadIdx.x;
	const double inf = __builtin_inf();
	const int cw = (u.m + 63) / 64;
	const int lanes = (u.m + cw - 1) / cw;  // lanes with a strip
	const long long c0l = (long long)lane * cw;
	const int c0 = c0l < u.m ? (int)c0l : u.m, c1 = min(c0 + cw, u.m);  // this lane's columns [c0, c1)
	double edge = inf;     // D at the strip's right edge in the row this lane did last
	double in_prev = inf;  // what came from the left one step ago: D(i - 1, c0 - 1)
	const long long steps = (long long)u.n + lanes - 1;
	for (long long s = 0; s < steps; ++s) {
		double in = __shfl_up(edge, 1);  // D(i, c0 - 1): lane - 1 did row i one step ago
		if (lane == 0) in = inf;
		const long long il = s - lane;
		if (il < 0 || il >= u.n || c0 >= c1) continue;  // (every lane is back at the move above: the trip count is the wavefront's)
		const int i = (int)il;
		int lo, hi, ulo = 1, uhi = 0;  // allowed columns of this row and of the row above
		al_row(u, i, lo, hi);
		if (i > 0) al_row(u, i - 1, ulo, uhi);
		const int js = max(c0, lo), je = min(c1 - 1, hi);
		double *row = A.cells + u.cell_off + (long long)i * u.W - lo;
		const double *up_row = i > 0 ? A.cells + u.cell_off + (long long)(i - 1) * u.W - ulo : row;  // (read only where ulo <= j <= uhi)
		unsigned char *__restrict__ ch = A.choice + u.cell_off + (long long)i * u.W - lo;
		double left = in, diag = in_prev;
		if (js > c0) {  // the strip's first columns lie outside the band
			left = inf;
			diag = js - 1 >= ulo && js - 1 <= uhi ? up_row[js - 1] : inf;
		}
		for (int j = js; j <= je; j += AL_CHUNK) {
			double d[AL_CHUNK], up[AL_CHUNK];
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				const int jj = j + k;
				const bool in_row = jj <= je;
				d[k] = in_row ? row[jj] : 0.0;
				up[k] = in_row && jj >= ulo && jj <= uhi ? up_row[jj] : inf;
			}
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				const int jj = j + k;
				if (jj <= je) {
					const double Dd = diag, Du = up[k], Dl = left;
					double best;
					unsigned char c;
					if (Dd <= Du && Dd <= Dl) { best = Dd; c = 0; }
					else if (Du <= Dl) { best = Du; c = 1; }
					else { best = Dl; c = 2; }
					const double D = (i == 0 && jj == 0) ? d[k] : d[k] + best;
					row[jj] = D;
					ch[jj] = c;
					diag = Du;
					left = D;
				}
			}
		}
		edge = je == c1 - 1 && js <= je ? left : inf;
		in_prev = in;
	}
}

__global__ __launch_bounds__(64) void align_path_kernel(AlArgs A) {
	const int p = blockIdx.x;
	const AlPair u = A.pairs[p];
	const int lane = threadIdx.x;
	int lo, hi;
	al_row(u, u.n - 1, lo, hi);
	const double total = A.cells[u.cell_off + (long long)(u.n - 1) * u.W + (u.m - 1 - lo)];
	if (lane == 0) A.cost[p] = total;
	if (!(fabs(total) < __builtin_inf())) {
		if (lane == 0) A.path_length[p] = 0;
		const double nan = __builtin_nan("");
		if (A.b_on_a)
			for (int i = lane; i < u.n; i += 64) A.b_on_a[u.a_off + i] = nan;
		if (A.a_on_b)
			for (int j = lane; j < u.m; j += 64) A.a_on_b[u.b_off + j] = nan;
		return;
	}
	int K = 0;
	if (lane == 0) {
		int i = u.n - 1, j = u.m - 1;
		int jmax = j, imax = i;  // the first column met in row i / the first row met in column j
		const long long most = (long long)u.n + u.m - 1;
		for (long long k = 0; k < most; ++k) {
			A.back[u.path_off + k] = make_int2(i, j);
			K = (int)k + 1;
			if (i == 0 && j == 0) break;
			al_row(u, i, lo, hi);
			if (j < lo || j > hi) break;  // (a finite total never leads here)
			const unsigned char c = A.choice[u.cell_off + (long long)i * u.W + (j - lo)];
			const int ni = (c != 2 && i > 0) ? i - 1 : i, nj = (c != 1 && j > 0) ? j - 1 : j;
			if (ni == i && nj == j) break;
			if (ni != i) {
				if (A.b_on_a) A.b_on_a[u.a_off + i] = (double)(j + jmax) * 0.5;
				jmax = nj;
			}
			if (nj != j) {
				if (A.a_on_b) A.a_on_b[u.b_off + j] = (double)(i + imax) * 0.5;
				imax = ni;
			}
			i = ni; j = nj;
		}
		if (A.b_on_a) A.b_on_a[u.a_off + i] = (double)(j + jmax) * 0.5;
		if (A.a_on_b) A.a_on_b[u.b_off + j] = (double)(i + imax) * 0.5;
		A.path_length[p] = K;
	}
	if (!A.path) return;
	K = __shfl(K, 0);
	__threadfence();  // lane 0's cells, before the other lanes read them
	for (int k = lane; k < K; k += 64) A.path[u.path_off + k] = A.back[u.path_off + (K - 1 - k)];
}

// descriptor staging per (device, stream), as for retime and morph
std::mutex g_stage_mu;
std::map<std::pair<int, hipStream_t>, Staging *> g_stage;

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

extern "C" int wc_align_features_device(int n_pairs, const int *a_length, const double *d_feat_a, const int *b_length, const double *d_feat_b,
										int dims, int dim_begin, int dim_end, int band, double *d_cost, int *d_path_length, int *d_path,
										double *d_b_on_a, double *d_a_on_b) {
	if (n_pairs < 0) return fail(WC_ERR_INVALID, "align: negative n_pairs");
	if (dims < 1) return fail(WC_ERR_INVALID, "align: dims must be at least 1");
	if (dim_begin < 0 || dim_end > dims || dim_begin >= dim_end) return fail(WC_ERR_INVALID, "align: need 0 <= dim_begin < dim_end <= dims");
	if (band < 0) return fail(WC_ERR_INVALID, "align: negative band");
	if (n_pairs == 0) return WC_OK;
	if (!a_length || !b_length) return fail(WC_ERR_INVALID, "align: null length array");
	if (!d_feat_a || !d_feat_b || !d_cost || !d_path_length) return fail(WC_ERR_INVALID, "align: null features, d_cost or d_path_length");
	long long cells = 0, entries = 0, tiles = 0;
	for (int u = 0; u < n_pairs; ++u) {
		const long long n = a_length[u], m = b_length[u];
		if (n < 1 || m < 1) return fail(WC_ERR_INVALID, "align: a length below 1");
		long long W = m;
		if (band >= 1 && band < (n > m ? n : m) && n > 1) {
			const long long L = (n > m ? n : m) - 1;
			const __int128 w = (__int128)2 * band * L / (n - 1) + 1;  // (band and L may both be near 2^31)
			if (w < W) W = (long long)w;
		}
		cells += n * W;  // (n, m < 2^31 and W <= m: one term stays below 2^62, and the sum is checked term by term)
		if (cells > kAlignMaxCells) return fail(WC_ERR_INVALID, "align: more than 2^28 stored cells in one call");
		entries += n + m - 1;
	}
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	Staging *st;
	{
		std::lock_guard<std::mutex> g(g_stage_mu);
		Staging *&slot = g_stage[{dev->id, s}];
		if (!slot) slot = new Staging();
		st = slot;
	}
	int rc;
	const size_t bytes = sizeof(AlPair) * (size_t)n_pairs;
	if ((rc = st->h.reserve(bytes))) return rc;
	if ((rc = st->d.reserve(bytes))) return rc;
	AlPair *h = st->h.as<AlPair>();
	long long fa = 0, fb = 0, co = 0, po = 0;
	for (int u = 0; u < n_pairs; ++u) {
		const long long n = a_length[u], m = b_length[u], L = (n > m ? n : m) - 1;
		AlPair &q = h[u];
		q.a_off = fa; q.b_off = fb; q.cell_off = co; q.path_off = po; q.tile_off = tiles;
		q.n = (int)n; q.m = (int)m;
		// a band of max(n, m) or more allows every cell (|i * (m - 1) - j * (n - 1)| <= (n - 1) * (m - 1) <= band * L)
		q.B = band >= 1 && band <= L ? band * L : -1;
		long long W = m, span = m;
		if (q.B >= 0 && n > 1) {
			const long long w = 2 * q.B / (n - 1) + 1;
			if (w < W) W = w;
			// the columns a block of 32 rows can touch: its widest row plus what the band's edge moves over 31 rows
			const long long sp = W + (AL_TILE - 1) * ((m - 1 + n - 2) / (n - 1)) + 2;
			if (sp < span) span = sp;
		}
		q.W = (int)W;
		q.tiles_j = (int)((span + AL_TILE - 1) / AL_TILE);
		tiles += (n + AL_TILE - 1) / AL_TILE * q.tiles_j;
		fa += n; fb += m; co += n * W; po += n + m - 1;
	}
	if (tiles > 0x7fffffffll) return fail(WC_ERR_INVALID, "align: more than 2^31 - 1 cost tiles in one call");
	// scratch: cells (doubles), the backward path (int2), choices (bytes)
	const size_t cells_bytes = (size_t)cells * sizeof(double), back_bytes = (size_t)entries * sizeof(int2);
	const size_t need = cells_bytes + back_bytes + round_up((size_t)cells, 8);
	if (need > dev->align_scratch.cap) {
		dev->quiesce();  // an earlier call's kernels may still use the buffer that is about to go
		if ((rc = dev->align_scratch.reserve(need))) return rc;
	}
	if (!dev->align_done) WC_HIP(hipEventCreateWithFlags(&dev->align_done, hipEventDisableTiming));
	else if (dev->align_last != s) WC_HIP(hipStreamWaitEvent(s, dev->align_done, 0));
	WC_HIP(hipMemcpyAsync(st->d.p, h, bytes, hipMemcpyHostToDevice, s));
	if ((rc = st->h.mark(s))) return rc;
	AlArgs a;
	a.pairs = st->d.as<AlPair>();
	a.n_pairs = n_pairs; a.dims = dims; a.dim_begin = dim_begin; a.dim_end = dim_end;
	a.fa = d_feat_a; a.fb = d_feat_b;
	char *base = dev->align_scratch.as<char>();
	a.cells = reinterpret_cast<double *>(base);
	a.back = reinterpret_cast<int2 *>(base + cells_bytes);
	a.choice = reinterpret_cast<unsigned char *>(base + cells_bytes + back_bytes);
	a.cost = d_cost; a.path_length = d_path_length; a.path = reinterpret_cast<int2 *>(d_path);
	a.b_on_a = d_b_on_a; a.a_on_b = d_a_on_b;
	if ((rc = dev->time_begin("align_cost_kernel", s))) return rc;
	hipLaunchKernelGGL(align_cost_kernel, dim3((unsigned)tiles), dim3(256), 0, s, a);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("align_cost_kernel", s))) return rc;
	if ((rc = dev->time_begin("align_accumulate_kernel", s))) return rc;
	hipLaunchKernelGGL(align_accumulate_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, a);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("align_accumulate_kernel", s))) return rc;
	if ((rc = dev->time_begin("align_path_kernel", s))) return rc;
	hipLaunchKernelGGL(align_path_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, a);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("align_path_kernel", s))) return rc;
	WC_HIP(hipEventRecord(dev->align_done, s));
	dev->align_last = s;
	return WC_OK;
}
