// Feature alignment (include/world_class_io.h: wc_align_features_device): dynamic time warping of a packed batch of pairs of
// feature sequences to the time maps that retime and morph take.  Three launches for the whole batch, all bounded by lengths the
// host wrote into the descriptors:
//
//   align_cost_kernel   (wc_align_cost.hpp, shared with the alignment streams)  fully parallel: a workgroup of 256 fills a tile of 32 rows of A x 32 rows of B with the local costs
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
// wc_align_features_ex_device runs the same three launches under its wider rule (open ends, the slope-limited step pattern 1,
// the span and the path's timelines), and wc_align_features_device is that call at pattern 0 without flags:
//   align_accumulate_kernel<true>   the kernel above with D(0, j) = d(0, j) in row 0 (an open beginning).
//   align_accumulate_slope_kernel   step pattern 1 on the same plan.  Every term of a cell lies in the two rows above it or in d,
//     so D gets an array of its own beside the read-only d, and a strip is at least two columns wide: what lane l needs of columns
//     c0 - 1 and c0 - 2 is the last two D of lane l - 1's strip, handed over by two cross-lane moves per step and kept for two
//     steps.  No lane reads from memory a D that another lane wrote.
//   align_path_kernel   under an open end all 64 lanes scan row n - 1 for the lowest column of the least D first; the backtrack
//     stops in row 0 under an open beginning and adds the intermediate cell of a two-cell step; the forward pass writes the
//     timelines beside the path, and all lanes fill a_on_b outside the span.
//
//   The descriptors go up through page-locked staging kept per (device, stream); the scratch is the device's (Device::align_scratch).
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

#include "../../include/world_class_c.h"
#include "../../include/world_class_io.h"
#include "wc_align_cost.hpp"
#include "wc_stages.hpp"

using namespace wc;

namespace {

constexpr long long kAlignMaxCells = 1ll << 28;  // stored cells per call (world_class_io.h)
constexpr long long kAlignMaxCellsSlope = 1ll << 27;  // the same under step pattern 1, which keeps d and D side by side

// what the extended call adds (the kernels of the plain call see it as pattern 0, no flags, no further outputs)
struct AlEx {
	double *acc;             // D(i, j) of step pattern 1, laid out like cells
	const double *D;         // where the path kernel finds D: cells (pattern 0) or acc
	int pattern, flags;
	int *span;
	double *timeline_a, *timeline_b;
};

// OPEN_BEGIN: every allowed cell of row 0 starts a path, D(0, j) = d(0, j)
template <bool OPEN_BEGIN>
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
					const double D = (i == 0 && (OPEN_BEGIN || jj == 0)) ? d[k] : d[k] + best;
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

// Step pattern 1 (slope between 1/2 and 2): Dd = D(i - 1, j - 1), Du = D(i - 2, j - 1) + d(i - 1, j), Dl = D(i - 1, j - 2) + d(i, j - 1).
// d stays in A.cells, D goes to X.acc.  A lane's strip is at least two columns wide, so columns c0 - 1 and c0 - 2 both belong to
// lane - 1, which hands the last two D of the row it just did over at every step; this lane keeps them for the two steps in which
// that row is its row above and its row two above.  Whether a term counts is decided from the rows' column ranges alone, so a
// value that was handed over or loaded for a cell outside them is never used.
__global__ __launch_bounds__(64) void align_accumulate_slope_kernel(AlArgs A, AlEx X) {
	const AlPair u = A.pairs[blockIdx.x];
	const int lane = threadIdx.x;
	const double inf = __builtin_inf();
	const bool open_begin = (X.flags & WC_ALIGN_OPEN_BEGIN) != 0;
	const int cw = max(2, (u.m + 63) / 64);
	const int lanes = (u.m + cw - 1) / cw;  // lanes with a strip
	const long long c0l = (long long)lane * cw;
	const int c0 = c0l < u.m ? (int)c0l : u.m, c1 = min(c0 + cw, u.m);  // this lane's columns [c0, c1)
	double e1 = inf, e2 = inf;  // D at columns c1 - 1 and c1 - 2 in the row this lane did last
	double in1_p = inf, in1_pp = inf, in2_p = inf;  // from the left: D(i - 1, c0 - 1), D(i - 2, c0 - 1), D(i - 1, c0 - 2)
	const long long steps = (long long)u.n + lanes - 1;
	for (long long s = 0; s < steps; ++s) {
		const double in1 = __shfl_up(e1, 1), in2 = __shfl_up(e2, 1);  // D(i, c0 - 1), D(i, c0 - 2): lane - 1 did row i one step ago
		const long long il = s - lane;
		if (il < 0 || il >= u.n || c0 >= c1) continue;  // (every lane is back at the moves above: the trip count is the wavefront's)
		const int i = (int)il;
		int lo0, hi0, lo1 = 1, hi1 = 0, lo2 = 1, hi2 = 0;  // allowed columns of this row, of the row above and of the one above that
		al_row(u, i, lo0, hi0);
		if (i > 0) al_row(u, i - 1, lo1, hi1);
		if (i > 1) al_row(u, i - 2, lo2, hi2);
		const int js = max(c0, lo0), je = min(c1 - 1, hi0);
		const long long r0 = u.cell_off + (long long)i * u.W - lo0;
		const long long r1 = i > 0 ? u.cell_off + (long long)(i - 1) * u.W - lo1 : r0;  // (read only where lo1 <= j <= hi1)
		const long long r2 = i > 1 ? u.cell_off + (long long)(i - 2) * u.W - lo2 : r0;
		const double *d0 = A.cells + r0, *d1 = A.cells + r1;
		double *D0 = X.acc + r0;
		const double *D1 = X.acc + r1, *D2 = X.acc + r2;
		unsigned char *__restrict__ ch = A.choice + r0;
		// what lies left of the strip's first allowed cell: D(i - 1, js - 1), D(i - 1, js - 2), D(i - 2, js - 1), d(i, js - 1)
		double p1 = in1_p, p2 = in2_p, q1 = in1_pp;
		if (js > c0 && js <= je) {  // the strip's first columns lie outside the band: this lane's own columns come before js
			p1 = js - 1 >= lo1 && js - 1 <= hi1 ? D1[js - 1] : inf;
			q1 = js - 1 >= lo2 && js - 1 <= hi2 ? D2[js - 1] : inf;
			p2 = js - 2 < c0 ? in1_p : (js - 2 >= lo1 && js - 2 <= hi1 ? D1[js - 2] : inf);
		}
		double pd0 = js <= je && js - 1 >= lo0 ? d0[js - 1] : inf;
		e1 = inf; e2 = inf;
		for (int j = js; j <= je; j += AL_CHUNK) {
			double a0[AL_CHUNK], a1[AL_CHUNK], b1[AL_CHUNK], b2[AL_CHUNK];
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				const int jj = j + k;
				const bool in_row = jj <= je;
				const bool in1r = in_row && jj >= lo1 && jj <= hi1;
				a0[k] = in_row ? d0[jj] : 0.0;
				a1[k] = in1r ? d1[jj] : inf;
				b1[k] = in1r ? D1[jj] : inf;
				b2[k] = in_row && jj >= lo2 && jj <= hi2 ? D2[jj] : inf;
			}
#pragma unroll
			for (int k = 0; k < AL_CHUNK; ++k) {
				const int jj = j + k;
				if (jj <= je) {
					const bool vd = jj - 1 >= lo1 && jj - 1 <= hi1;
					const bool vu = jj - 1 >= lo2 && jj - 1 <= hi2 && jj >= lo1 && jj <= hi1;
					const bool vl = jj - 2 >= lo1 && jj - 2 <= hi1 && jj - 1 >= lo0;  // (jj - 1 < jj <= hi0)
					const double Dd = vd ? p1 : inf;
					const double Du = vu ? q1 + a1[k] : inf;
					const double Dl = vl ? p2 + pd0 : inf;
					double best;
					unsigned char c;
					if (Dd <= Du && Dd <= Dl) { best = Dd; c = 0; }
					else if (Du <= Dl) { best = Du; c = 1; }
					else { best = Dl; c = 2; }
					const double D = (i == 0 && (open_begin || jj == 0)) ? a0[k] : a0[k] + best;
					D0[jj] = D;
					ch[jj] = c;
					p2 = p1; p1 = b1[k]; q1 = b2[k]; pd0 = a0[k];
					e2 = e1; e1 = D;
				}
			}
		}
		if (je != c1 - 1) {  // the band ends inside the strip: column c1 - 1 was not done, column c1 - 2 only if it is the last one done
			e2 = js <= je && je == c1 - 2 ? e1 : inf;
			e1 = inf;
		}
		in1_pp = in1_p; in1_p = in1; in2_p = in2;
	}
}

__global__ __launch_bounds__(64) void align_path_kernel(AlArgs A, AlEx X) {
	const int p = blockIdx.x;
	const AlPair u = A.pairs[p];
	const int lane = threadIdx.x;
	const double inf = __builtin_inf();
	int lo, hi;
	al_row(u, u.n - 1, lo, hi);
	const double *last = X.D + u.cell_off + (long long)(u.n - 1) * u.W - lo;
	int j_end = u.m - 1;
	if (X.flags & WC_ALIGN_OPEN_END) {  // the lowest column of the least D of row n - 1; NaN and +inf never win
		const int none = 0x7fffffff;
		double best = inf;
		int bj = none;
		for (long long j = (long long)lo + lane; j <= hi; j += 64) {
			const double v = last[j];
			if (v < best) { best = v; bj = (int)j; }
		}
		for (int o = 32; o > 0; o >>= 1) {
			const double ov = __shfl_xor(best, o);
			const int oj = __shfl_xor(bj, o);
			if (ov < best || (ov == best && oj < bj)) { best = ov; bj = oj; }
		}
		if (bj != none) j_end = bj;
	}
	const double total = last[j_end];
	if (lane == 0) A.cost[p] = total;
	if (!(fabs(total) < inf)) {
		if (lane == 0) {
			A.path_length[p] = 0;
			if (X.span) X.span[2 * p] = X.span[2 * p + 1] = -1;
		}
		const double nan = __builtin_nan("");
		if (A.b_on_a)
			for (int i = lane; i < u.n; i += 64) A.b_on_a[u.a_off + i] = nan;
		if (A.a_on_b)
			for (int j = lane; j < u.m; j += 64) A.a_on_b[u.b_off + j] = nan;
		return;
	}
	int K = 0, j_first = 0;
	if (lane == 0) {
		int i = u.n - 1, j = j_end;
		int jmax = j, imax = i;  // the first column met in row i / the first row met in column j
		const bool open_begin = (X.flags & WC_ALIGN_OPEN_BEGIN) != 0;
		const long long most = (long long)u.n + u.m - 1;
		// one cell back: the map entry of the row and of the column that the path leaves
		auto go = [&](int ni, int nj) {
			if (ni != i) {
				if (A.b_on_a) A.b_on_a[u.a_off + i] = (double)(j + jmax) * 0.5;
				jmax = nj;
			}
			if (nj != j) {
				if (A.a_on_b) A.a_on_b[u.b_off + j] = (double)(i + imax) * 0.5;
				imax = ni;
			}
			i = ni; j = nj;
		};
		long long k = 0;
		while (k < most) {
			A.back[u.path_off + k++] = make_int2(i, j);
			if (i == 0 && (j == 0 || open_begin)) break;
			al_row(u, i, lo, hi);
			if (j < lo || j > hi) break;  // (a finite total never leads here)
			const unsigned char c = A.choice[u.cell_off + (long long)i * u.W + (j - lo)];
			if (X.pattern == 0) {
				const int ni = (c != 2 && i > 0) ? i - 1 : i, nj = (c != 1 && j > 0) ? j - 1 : j;
				if (ni == i && nj == j) break;
				go(ni, nj);
			} else {
				const int mi = c == 2 ? i : i - 1, mj = c == 1 ? j : j - 1;  // the cell behind (i, j); the step ends one diagonal further
				if (c == 0) {
					if (mi < 0 || mj < 0) break;
					go(mi, mj);
				} else {
					if (mi < 1 || mj < 1 || k >= most) break;
					go(mi, mj);
					A.back[u.path_off + k++] = make_int2(i, j);
					go(i - 1, j - 1);
				}
			}
		}
		K = (int)k;
		if (A.b_on_a) A.b_on_a[u.a_off + i] = (double)(j + jmax) * 0.5;
		if (A.a_on_b) A.a_on_b[u.b_off + j] = (double)(i + imax) * 0.5;
		A.path_length[p] = K;
		j_first = j;
		if (X.span) {
			X.span[2 * p] = j_first;
			X.span[2 * p + 1] = j_end;
		}
	}
	K = __shfl(K, 0);
	j_first = __shfl(j_first, 0);
	if (A.a_on_b) {  // outside the span the end frames are held
		for (int j = lane; j < j_first; j += 64) A.a_on_b[u.b_off + j] = 0.0;
		for (long long j = (long long)j_end + 1 + lane; j < u.m; j += 64) A.a_on_b[u.b_off + j] = (double)(u.n - 1);
	}
	if (!A.path && !X.timeline_a && !X.timeline_b) return;
	__threadfence();  // lane 0's cells, before the other lanes read them
	for (int k = lane; k < K; k += 64) {
		const int2 c = A.back[u.path_off + (K - 1 - k)];
		if (A.path) A.path[u.path_off + k] = c;
		if (X.timeline_a) X.timeline_a[u.path_off + k] = (double)c.x;
		if (X.timeline_b) X.timeline_b[u.path_off + k] = (double)c.y;
	}
}

// descriptor staging per (device, stream), as for retime and morph
std::mutex g_stage_mu;
std::map<std::pair<int, hipStream_t>, Staging *> g_stage;

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

extern "C" int wc_align_features_ex_device(int n_pairs, const int *a_length, const double *d_feat_a, const int *b_length,
										   const double *d_feat_b, int dims, int dim_begin, int dim_end, int band, int step_pattern, int flags,
										   double *d_cost, int *d_path_length, int *d_path, double *d_b_on_a, double *d_a_on_b, int *d_span,
										   double *d_timeline_a, double *d_timeline_b) {
	if (n_pairs < 0) return fail(WC_ERR_INVALID, "align: negative n_pairs");
	if (dims < 1) return fail(WC_ERR_INVALID, "align: dims must be at least 1");
	if (dim_begin < 0 || dim_end > dims || dim_begin >= dim_end) return fail(WC_ERR_INVALID, "align: need 0 <= dim_begin < dim_end <= dims");
	if (band < 0) return fail(WC_ERR_INVALID, "align: negative band");
	if (step_pattern != 0 && step_pattern != 1) return fail(WC_ERR_INVALID, "align: step_pattern must be 0 or 1");
	if (flags < 0 || flags > (WC_ALIGN_OPEN_BEGIN | WC_ALIGN_OPEN_END)) return fail(WC_ERR_INVALID, "align: unknown flags");
	if (flags != 0 && band != 0) return fail(WC_ERR_INVALID, "align: a band has no meaning under an open end");
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
		if (step_pattern == 1 && cells > kAlignMaxCellsSlope)
			return fail(WC_ERR_INVALID, "align: more than 2^27 stored cells in one call under step pattern 1");
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
	// scratch: cells (doubles), under step pattern 1 as many again for D, the backward path (int2), choices (bytes)
	const size_t cells_bytes = (size_t)cells * sizeof(double), back_bytes = (size_t)entries * sizeof(int2);
	const size_t acc_bytes = step_pattern == 1 ? cells_bytes : 0;
	const size_t need = cells_bytes + acc_bytes + back_bytes + round_up((size_t)cells, 8);
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
	a.back = reinterpret_cast<int2 *>(base + cells_bytes + acc_bytes);
	a.choice = reinterpret_cast<unsigned char *>(base + cells_bytes + acc_bytes + back_bytes);
	a.cost = d_cost; a.path_length = d_path_length; a.path = reinterpret_cast<int2 *>(d_path);
	a.b_on_a = d_b_on_a; a.a_on_b = d_a_on_b;
	AlEx x;
	x.acc = reinterpret_cast<double *>(base + cells_bytes);
	x.D = step_pattern == 1 ? x.acc : a.cells;
	x.pattern = step_pattern; x.flags = flags;
	x.span = d_span; x.timeline_a = d_timeline_a; x.timeline_b = d_timeline_b;
	if ((rc = dev->time_begin("align_cost_kernel", s))) return rc;
	hipLaunchKernelGGL(align_cost_kernel, dim3((unsigned)tiles), dim3(256), 0, s, a);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("align_cost_kernel", s))) return rc;
	const char *acc_name = step_pattern == 1 ? "align_accumulate_slope_kernel" : "align_accumulate_kernel";
	if ((rc = dev->time_begin(acc_name, s))) return rc;
	if (step_pattern == 1) hipLaunchKernelGGL(align_accumulate_slope_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, a, x);
	else if (flags & WC_ALIGN_OPEN_BEGIN) hipLaunchKernelGGL(align_accumulate_kernel<true>, dim3((unsigned)n_pairs), dim3(64), 0, s, a);
	else hipLaunchKernelGGL(align_accumulate_kernel<false>, dim3((unsigned)n_pairs), dim3(64), 0, s, a);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end(acc_name, s))) return rc;
	if ((rc = dev->time_begin("align_path_kernel", s))) return rc;
	hipLaunchKernelGGL(align_path_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, a, x);
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("align_path_kernel", s))) return rc;
	WC_HIP(hipEventRecord(dev->align_done, s));
	dev->align_last = s;
	return WC_OK;
}

extern "C" int wc_align_features_device(int n_pairs, const int *a_length, const double *d_feat_a, const int *b_length, const double *d_feat_b,
										int dims, int dim_begin, int dim_end, int band, double *d_cost, int *d_path_length, int *d_path,
										double *d_b_on_a, double *d_a_on_b) {
	return wc_align_features_ex_device(n_pairs, a_length, d_feat_a, b_length, d_feat_b, dims, dim_begin, dim_end, band, 0, 0, d_cost,
									   d_path_length, d_path, d_b_on_a, d_a_on_b, nullptr, nullptr, nullptr);
}
