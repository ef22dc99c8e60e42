// Parallel-corpus joint rows (include/world_class_parallel.h): the gather along an alignment path, the speech mask, the distortion.
//
//   par_joint_kernel  the gather, bound by memory.  The lanes of a wavefront lie on neighbouring columns of one output row; where
//                     D = dx + dy is small a wavefront holds 64 / G rows, G the smallest power of two that holds D.  The first lane
//                     of a row's group reads the pair, the path length, the path entry and the two mask bytes, once per row, writes
//                     the row's mask byte and hands (i, j, on) to its group through the wavefront; the group then walks the D
//                     columns, neighbouring lanes on neighbouring columns of A's row, B's row and the output row.
//   par_mask_kernel   one wavefront per utterance: the greatest finite value of the column (a maximum is exact, so the order of the
//                     butterfly is no part of the rule), then the bytes.
//   par_cell_kernel   one lane per slot: e(s) by the chain of wc_align_cost.hpp (ascending c from 0.0; difference, product and sum
//                     rounded apart; the correctly rounded root), into d_cell or into scratch.
//   par_sum_kernel    one wavefront per pair: 64 slots' states and distances are read side by side, then the live ones are added
//                     one after the other in ascending s -- every lane carries the same chain, so the sum is strictly sequential
//                     whatever the launch shape.
// No atomics.  Every loop is bounded by arguments the host validated (wc_parallel_plan.hpp); an index read from the path is used only
// behind the on-path test.  The tree is built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <map>
#include <mutex>

#include "../../include/world_class_parallel.h"
#include "wc_internal.hpp"
#include "wc_parallel_plan.hpp"

using namespace wc;

namespace {

struct ParPath {
	const ParPair *pairs;
	int n_pairs;
	long long slots;
	const int *path_length, *path;
	const unsigned char *mask_a, *mask_b;
};

struct ParSlot {
	int i, j;
	bool on, live;
};

// the pair that owns slot g: the last one whose p_off <= g
__device__ __forceinline__ int par_find(const ParPath &P, long long g) {
	int lo = 0, hi = P.n_pairs;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (P.pairs[mid].p_off <= g) lo = mid;
		else hi = mid;
	}
	return lo;
}

// K' of the header
__device__ __forceinline__ int par_length(const ParPair &u, int K) { return K >= 0 && (long long)K <= (long long)u.a + u.b - 1 ? K : 0; }

// the state of slot s < cap of pair u, whose usable path length is Kp
__device__ __forceinline__ ParSlot par_slot(const ParPath &P, const ParPair &u, long long s, int Kp) {
	ParSlot r = {0, 0, false, false};
	if (s >= Kp) return r;
	const int i = P.path[2 * (u.p_off + s)], j = P.path[2 * (u.p_off + s) + 1];
	if (i < 0 || i >= u.a || j < 0 || j >= u.b) return r;
	r.i = i;
	r.j = j;
	r.on = true;
	r.live = (!P.mask_a || P.mask_a[u.a_off + i]) && (!P.mask_b || P.mask_b[u.b_off + j]);
	return r;
}

struct ParJointK {
	ParPath P;
	const void *rows_a, *rows_b;
	void *out;
	unsigned char *out_mask;
	int ld_a, col_a, dx, ld_b, col_b, dy, ld_o, col_o;
	int lanes_log2;  // G = 1 << lanes_log2 lanes of one row
};

template <class TA, class TB, class TO>
__global__ __launch_bounds__(256) void par_joint_kernel(ParJointK k) {
	const int tid = threadIdx.x, G = 1 << k.lanes_log2, sub = tid & (G - 1);
	const long long row = (long long)blockIdx.x * (256 >> k.lanes_log2) + (tid >> k.lanes_log2);
	const bool valid = row < k.P.slots;
	ParPair u = {0, 0, 0, 1, 1};
	int i = 0, j = 0, on = 0;
	if (valid && sub == 0) {
		const int p = par_find(k.P, row);
		u = k.P.pairs[p];
		const ParSlot st = par_slot(k.P, u, row - u.p_off, par_length(u, k.P.path_length[p]));
		i = st.i;
		j = st.j;
		on = st.on;
		if (k.out_mask) k.out_mask[row] = st.live ? 1 : 0;
	}
	// the group's first lane hands the row's state on (every lane of the wavefront is here: a group never straddles two wavefronts)
	const int first = (tid & 63) & ~(G - 1);
	const long long ra = __shfl(on ? u.a_off + i : 0ll, first, 64), rb = __shfl(on ? u.b_off + j : 0ll, first, 64);
	on = __shfl(on, first, 64);
	if (!valid) return;
	const int D = k.dx + k.dy;
	TO *o = static_cast<TO *>(k.out) + (size_t)row * k.ld_o + k.col_o;
	if (!on) {
		for (int c = sub; c < D; c += G) o[c] = (TO)0;
		return;
	}
	const TA *xa = static_cast<const TA *>(k.rows_a) + (size_t)ra * k.ld_a + k.col_a;
	const TB *xb = static_cast<const TB *>(k.rows_b) + (size_t)rb * k.ld_b + k.col_b;
	for (int c = sub; c < D; c += G) o[c] = c < k.dx ? (TO)xa[c] : (TO)xb[c - k.dx];
}

template <class T>
__global__ __launch_bounds__(64) void par_mask_kernel(const ParUtt *__restrict__ utt, const T *__restrict__ rows, int ld, int col, double margin,
													  double floor, unsigned char *__restrict__ mask) {
	const ParUtt u = utt[blockIdx.x];
	const unsigned lane = threadIdx.x, n = (unsigned)u.n;  // (unsigned frame indices: t + 64 may pass 2^31 - 1)
	const T *c = rows + (size_t)u.f_off * ld + col;
	double top = -INFINITY;  // below every finite value: it stays where the utterance has none
	for (unsigned t = lane; t < n; t += 64) {
		const double v = (double)c[(size_t)t * ld];
		if (fabs(v) <= DBL_MAX && v > top) top = v;
	}
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const double other = __shfl_xor(top, off, 64);
		if (other > top) top = other;
	}
	const bool none = top == -INFINITY;
	const double least = top - margin;
	unsigned char *m = mask + u.f_off;
	for (unsigned t = lane; t < n; t += 64) {
		const double v = (double)c[(size_t)t * ld];
		m[t] = !none && fabs(v) <= DBL_MAX && v >= least && v >= floor ? 1 : 0;
	}
}

struct ParDistK {
	ParPath P;
	const void *rows_a, *rows_b;
	int ld_a, col_a, ld_b, col_b, dims;
	double *cell;  // d_cell, or the scratch that stands in for it
	double *sum;
	long long *count;
};

template <class TA, class TB>
__global__ __launch_bounds__(256) void par_cell_kernel(ParDistK k) {
	const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
	if (g >= k.P.slots) return;
	const int p = par_find(k.P, g);
	const ParPair u = k.P.pairs[p];
	const ParSlot st = par_slot(k.P, u, g - u.p_off, par_length(u, k.P.path_length[p]));
	double e = 0.0;
	if (st.on) {
		const TA *xa = static_cast<const TA *>(k.rows_a) + (size_t)(u.a_off + st.i) * k.ld_a + k.col_a;
		const TB *xb = static_cast<const TB *>(k.rows_b) + (size_t)(u.b_off + st.j) * k.ld_b + k.col_b;
		double acc = 0.0;
		for (int c = 0; c < k.dims; ++c) {
			const double d = (double)xa[c] - (double)xb[c];
			acc = acc + d * d;
		}
		e = __dsqrt_rn(acc);
	}
	k.cell[g] = e;
}

__global__ __launch_bounds__(64) void par_sum_kernel(ParDistK k) {
	const int p = blockIdx.x, lane = threadIdx.x;
	const ParPair u = k.P.pairs[p];
	const int Kp = par_length(u, k.P.path_length[p]);
	double sum = 0.0;
	long long count = 0;
	for (long long base = 0; base < Kp; base += 64) {
		const long long s = base + lane;
		const bool live = par_slot(k.P, u, s, Kp).live;  // (false at and behind Kp)
		const double e = live ? k.cell[u.p_off + s] : 0.0;
		unsigned long long todo = __ballot(live);  // the same in every lane: the loop below does not diverge
		while (todo) {
			const int src = __ffsll((long long)todo) - 1;
			todo &= todo - 1;
			const double v = __shfl(e, src, 64);
			sum = count ? sum + v : v;  // the sum starts at its first term
			++count;
		}
	}
	if (lane == 0) {
		if (k.sum) k.sum[p] = sum;
		if (k.count) k.count[p] = count;
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// the descriptors' way up and the distances' scratch, per (device, stream): a call on a stream follows the one before it on that stream
struct ParStage {
	HostBuf h;
	DevBuf d, cells;
};
std::mutex g_par_mu;
std::map<std::pair<int, hipStream_t>, ParStage *> g_par;

ParStage *par_stage(Device *dev, hipStream_t s) {
	std::lock_guard<std::mutex> g(g_par_mu);
	ParStage *&slot = g_par[{dev->id, s}];
	if (!slot) slot = new ParStage();
	return slot;
}

// a buffer that must grow is let go only behind the kernels that may still read it
int par_reserve(Device *dev, DevBuf *b, size_t bytes) {
	if (bytes <= b->cap) return WC_OK;
	dev->quiesce();
	return b->reserve(bytes);
}

template <class Rec>
int par_upload(Device *dev, hipStream_t s, ParStage *st, const std::vector<Rec> &recs, const Rec **on_device) {
	const size_t bytes = sizeof(Rec) * recs.size();
	int rc;
	if ((rc = st->h.reserve(bytes))) return rc;
	if ((rc = par_reserve(dev, &st->d, bytes))) return rc;
	std::copy(recs.begin(), recs.end(), st->h.as<Rec>());
	WC_HIP(hipMemcpyAsync(st->d.p, st->h.p, bytes, hipMemcpyHostToDevice, s));
	if ((rc = st->h.mark(s))) return rc;
	*on_device = st->d.as<Rec>();
	return WC_OK;
}

int par_refuse(const char *who, const std::string &why) { return fail(WC_ERR_INVALID, std::string(who) + ": " + why); }

template <class TA, class TB>
void par_joint_launch(int out_format, unsigned blocks, hipStream_t s, const ParJointK &k) {
	if (out_format == WC_FEAT_F32) hipLaunchKernelGGL((par_joint_kernel<TA, TB, float>), dim3(blocks), dim3(256), 0, s, k);
	else hipLaunchKernelGGL((par_joint_kernel<TA, TB, double>), dim3(blocks), dim3(256), 0, s, k);
}

}  // namespace

extern "C" {

int wc_joint_rows_device(int n_pairs, const int *a_length, const int *b_length, int a_format, const void *d_rows_a, int ld_a, int col_a, int dx,
						 int b_format, const void *d_rows_b, int ld_b, int col_b, int dy, const int *d_path_length, const int *d_path,
						 const unsigned char *d_mask_a, const unsigned char *d_mask_b, int out_format, void *d_joint, int ld_out, int col_out,
						 unsigned char *d_joint_mask) {
	const char *who = "joint rows";
	const long long D = (long long)dx + dy;
	const ParJointArgs g = {n_pairs, a_length, b_length, {a_format, ld_a, col_a, dx}, {b_format, ld_b, col_b, dy},
							{out_format, ld_out, col_out, dx >= 1 && dy >= 1 && D <= kParMaxJoint ? (int)D : 1},
							d_rows_a, d_rows_b, d_path_length, d_path, d_mask_a, d_mask_b, d_joint, d_joint_mask};
	ParCounts counts;
	std::vector<ParPair> pairs;
	std::string why;
	if (!par_joint_plan(g, &counts, &pairs, &why)) return par_refuse(who, why);
	if (n_pairs == 0) return WC_OK;
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	ParStage *st = par_stage(dev, s);
	int rc;
	ParJointK k = {};
	if ((rc = par_upload(dev, s, st, pairs, &k.P.pairs))) return rc;
	k.P.n_pairs = n_pairs;
	k.P.slots = counts.slots;
	k.P.path_length = d_path_length;
	k.P.path = d_path;
	k.P.mask_a = d_mask_a;
	k.P.mask_b = d_mask_b;
	k.rows_a = d_rows_a; k.rows_b = d_rows_b; k.out = d_joint; k.out_mask = d_joint_mask;
	k.ld_a = ld_a; k.col_a = col_a; k.dx = dx; k.ld_b = ld_b; k.col_b = col_b; k.dy = dy; k.ld_o = ld_out; k.col_o = col_out;
	const int G = par_row_lanes((int)D);
	while ((1 << k.lanes_log2) < G) ++k.lanes_log2;
	const long long per_block = 256 / G;
	const unsigned blocks = (unsigned)((counts.slots + per_block - 1) / per_block);
	if ((rc = dev->time_begin("par_joint_kernel", s))) return rc;
	if (a_format == WC_FEAT_F32) {
		if (b_format == WC_FEAT_F32) par_joint_launch<float, float>(out_format, blocks, s, k);
		else par_joint_launch<float, double>(out_format, blocks, s, k);
	} else {
		if (b_format == WC_FEAT_F32) par_joint_launch<double, float>(out_format, blocks, s, k);
		else par_joint_launch<double, double>(out_format, blocks, s, k);
	}
	WC_HIP(hipGetLastError());
	return dev->time_end("par_joint_kernel", s);
}

int wc_speech_mask_device(int n_utt, const int *lengths, int format, const void *d_rows, int ld, int col, double margin, double floor,
						  unsigned char *d_mask) {
	const char *who = "speech mask";
	long long frames = 0;
	std::vector<ParUtt> utts;
	std::string why;
	if (!par_mask_plan(n_utt, lengths, ParRows{format, ld, col, 1}, d_rows, margin, floor, d_mask, &frames, &utts, &why)) return par_refuse(who, why);
	if (frames == 0) return WC_OK;
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	ParStage *st = par_stage(dev, s);
	int rc;
	const ParUtt *d_utt = nullptr;
	if ((rc = par_upload(dev, s, st, utts, &d_utt))) return rc;
	if ((rc = dev->time_begin("par_mask_kernel", s))) return rc;
	if (format == WC_FEAT_F32)
		hipLaunchKernelGGL(par_mask_kernel<float>, dim3((unsigned)n_utt), dim3(64), 0, s, d_utt, static_cast<const float *>(d_rows), ld, col, margin,
						   floor, d_mask);
	else
		hipLaunchKernelGGL(par_mask_kernel<double>, dim3((unsigned)n_utt), dim3(64), 0, s, d_utt, static_cast<const double *>(d_rows), ld, col, margin,
						   floor, d_mask);
	WC_HIP(hipGetLastError());
	return dev->time_end("par_mask_kernel", s);
}

int wc_path_distortion_device(int n_pairs, const int *a_length, const int *b_length, int a_format, const void *d_rows_a, int ld_a, int col_a,
							  int b_format, const void *d_rows_b, int ld_b, int col_b, int dims, const int *d_path_length, const int *d_path,
							  const unsigned char *d_mask_a, const unsigned char *d_mask_b, double *d_sum, long long *d_count, double *d_cell) {
	const char *who = "path distortion";
	const ParDistArgs g = {n_pairs, a_length, b_length, {a_format, ld_a, col_a, dims}, {b_format, ld_b, col_b, dims},
						   d_rows_a, d_rows_b, d_path_length, d_path, d_mask_a, d_mask_b, d_sum, d_count, d_cell};
	ParCounts counts;
	std::vector<ParPair> pairs;
	std::string why;
	if (!par_dist_plan(g, &counts, &pairs, &why)) return par_refuse(who, why);
	if (n_pairs == 0) return WC_OK;
	Device *dev = current_device();
	if (!dev) return WC_ERR_DEVICE;
	DeviceLock lock(dev);
	hipStream_t s = dev->active();
	ParStage *st = par_stage(dev, s);
	int rc;
	ParDistK k = {};
	if ((rc = par_upload(dev, s, st, pairs, &k.P.pairs))) return rc;
	if (!d_cell && (rc = par_reserve(dev, &st->cells, sizeof(double) * (size_t)counts.slots))) return rc;
	k.P.n_pairs = n_pairs;
	k.P.slots = counts.slots;
	k.P.path_length = d_path_length;
	k.P.path = d_path;
	k.P.mask_a = d_mask_a;
	k.P.mask_b = d_mask_b;
	k.rows_a = d_rows_a; k.rows_b = d_rows_b;
	k.ld_a = ld_a; k.col_a = col_a; k.ld_b = ld_b; k.col_b = col_b; k.dims = dims;
	k.cell = d_cell ? d_cell : st->cells.as<double>();
	k.sum = d_sum;
	k.count = d_count;
	const unsigned blocks = (unsigned)((counts.slots + 255) / 256);
	if ((rc = dev->time_begin("par_cell_kernel", s))) return rc;
	if (a_format == WC_FEAT_F32) {
		if (b_format == WC_FEAT_F32) hipLaunchKernelGGL((par_cell_kernel<float, float>), dim3(blocks), dim3(256), 0, s, k);
		else hipLaunchKernelGGL((par_cell_kernel<float, double>), dim3(blocks), dim3(256), 0, s, k);
	} else {
		if (b_format == WC_FEAT_F32) hipLaunchKernelGGL((par_cell_kernel<double, float>), dim3(blocks), dim3(256), 0, s, k);
		else hipLaunchKernelGGL((par_cell_kernel<double, double>), dim3(blocks), dim3(256), 0, s, k);
	}
	WC_HIP(hipGetLastError());
	if ((rc = dev->time_end("par_cell_kernel", s))) return rc;
	if (!d_sum && !d_count) return WC_OK;
	if ((rc = dev->time_begin("par_sum_kernel", s))) return rc;
	hipLaunchKernelGGL(par_sum_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, k);
	WC_HIP(hipGetLastError());
	return dev->time_end("par_sum_kernel", s);
}

}  // extern "C"
