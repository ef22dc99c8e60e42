// The host half of include/world_class_gmm_train.h in plain C++: the joint preparation, the M-step of THE rule operation for operation
// (the tree is built with -ffp-contract=off, on the host side as well), and how a launch is cut.  No device code and no HIP call.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "wc_gmm_plan.hpp"

namespace wc {

constexpr int kGmmSegment = 1024;                       // frames of one segment of THE rule
constexpr size_t kGmmTrainScratch = (size_t)256 << 20;  // what a launch's tables and segment sums take at the most, unless set
constexpr int kGmmTrainMaxSegments = 1 << 14;           // segments of one launch at the most (2^24 frames)

// a model as wc_gmm_create takes it, and what the joint preparation made of it
struct GmmTrainModel {
	int n_mix = 0, D = 0;
	bool set = false;
	std::vector<double> weight, mean, cov;  // n_mix; n_mix * D; n_mix * D * D, both triangles
	std::vector<double> W, c;               // n_mix * D * D row-major, upper part 0.0; n_mix
};

// the doubles of one mixture's statistics: N, S1, the lower triangle of S2
inline size_t gmm_train_width(int D) { return 1 + (size_t)D + (size_t)D * (D + 1) / 2; }

// the scratch of a launch of g segments: two tables (ll, gamma), frame_ll, the segment sums (LL, two counts), the partial statistics, the
// frames' states
inline size_t gmm_train_scratch_bytes(int n_mix, int D, long long g) {
	const size_t frames = (size_t)g * kGmmSegment;
	return frames * (2 * (size_t)n_mix + 1) * sizeof(double) + (size_t)g * (sizeof(double) + 2 * sizeof(long long)) +
		   (size_t)g * n_mix * gmm_train_width(D) * sizeof(double) + frames;
}

// segments per launch: what was set, else what the budget holds, and one at the least
inline int gmm_train_segments(int n_mix, int D, int set) {
	long long g = set > 0 ? set : (long long)(kGmmTrainScratch / gmm_train_scratch_bytes(n_mix, D, 1));
	g = g < 1 ? 1 : g;
	return (int)(g > kGmmTrainMaxSegments ? kGmmTrainMaxSegments : g);
}

// the joint preparation of one mixture: W (D x D, upper part left as it is) and *c; L is D * D of room -> the failing row or -1
inline long gmm_train_factor(int D, double w, const double *cov, double *L, double *W, double *c) {
	const long bad = gmm_factor((size_t)D, cov, (size_t)D, L, W);
	if (bad < 0) *c = gmm_constant((size_t)D, w, L);
	return bad;
}

// set_model: create's refusals on the joint matrix, then the preparation of every mixture; *mdl is written only where all of it holds
inline bool gmm_train_set_model(int n_mix, int D, const double *weight, const double *mean, const double *cov, GmmTrainModel *mdl, std::string *why) {
	const auto no = [&](const std::string &text) { *why = text; return false; };
	if (!weight || !mean || !cov) return no("null array");
	const size_t N = (size_t)D;
	const auto at = [](int m, size_t row) { return "mixture " + std::to_string(m) + ", row " + std::to_string(row); };
	for (int m = 0; m < n_mix; ++m) {
		if (!(weight[m] > 0.0) || !gmm_finite(weight[m])) return no("mixture " + std::to_string(m) + ": a weight that is not finite or not > 0");
		for (size_t i = 0; i < N; ++i) {
			if (!gmm_finite(mean[m * N + i])) return no(at(m, i) + ": a mean that is not finite");
			for (size_t j = 0; j <= i; ++j)
				if (!gmm_finite(cov[(m * N + i) * N + j])) return no(at(m, i) + ": a covariance entry that is not finite");
		}
	}
	std::vector<double> L(N * N), W((size_t)n_mix * N * N, 0.0), c((size_t)n_mix, 0.0);
	for (int m = 0; m < n_mix; ++m) {
		const long bad = gmm_train_factor(D, weight[m], cov + (size_t)m * N * N, L.data(), W.data() + (size_t)m * N * N, &c[m]);
		if (bad >= 0) return no(at(m, (size_t)bad) + ": the joint covariance is not positive definite (a Cholesky diagonal that is not > 0 or not finite)");
	}
	mdl->n_mix = n_mix; mdl->D = D;
	mdl->weight.assign(weight, weight + n_mix);
	mdl->mean.assign(mean, mean + (size_t)n_mix * N);
	mdl->cov.assign((size_t)n_mix * N * N, 0.0);
	for (size_t m = 0; m < (size_t)n_mix; ++m)  // the lower triangle is what was read; the upper mirrors it
		for (size_t i = 0; i < N; ++i)
			for (size_t j = 0; j <= i; ++j) mdl->cov[(m * N + i) * N + j] = mdl->cov[(m * N + j) * N + i] = cov[(m * N + i) * N + j];
	mdl->W.swap(W);
	mdl->c.swap(c);
	mdl->set = true;
	return true;
}

// the M-step of THE rule on the totals (stats: n_mix rows of N, S1, packed S2); floor: D values or nullptr
inline void gmm_train_update(GmmTrainModel *mdl, const double *stats, long long n_live, double min_occupancy, const double *floor, int *n_starved,
							 int *n_kept) {
	const size_t N = (size_t)mdl->D, P = gmm_train_width(mdl->D);
	std::vector<double> L(N * N), W(N * N), delta(N), mean(N), cov(N * N);
	*n_starved = *n_kept = 0;
	for (size_t m = 0; m < (size_t)mdl->n_mix; ++m) {
		const double *st = stats + m * P, *S1 = st + 1, *S2 = st + 1 + N;
		const double Nm = st[0];
		if (!(Nm >= min_occupancy)) {
			++*n_starved;
			continue;
		}
		const double w = Nm / (double)n_live;
		bool fine = w > 0.0 && gmm_finite(w);
		for (size_t i = 0; i < N; ++i) {
			delta[i] = S1[i] / Nm;
			mean[i] = mdl->mean[m * N + i] + delta[i];
			fine = fine && gmm_finite(mean[i]);
		}
		for (size_t i = 0; i < N; ++i)
			for (size_t j = 0; j <= i; ++j) {
				double v = S2[i * (i + 1) / 2 + j] / Nm - delta[i] * delta[j];
				if (j == i && floor && v < floor[i]) v = floor[i];
				cov[i * N + j] = cov[j * N + i] = v;
				fine = fine && gmm_finite(v);
			}
		std::fill(W.begin(), W.end(), 0.0);
		double c = 0.0;
		if (!fine || gmm_train_factor(mdl->D, w, cov.data(), L.data(), W.data(), &c) >= 0) {
			++*n_kept;
			continue;
		}
		mdl->weight[m] = w;
		std::copy(mean.begin(), mean.end(), mdl->mean.begin() + m * N);
		std::copy(cov.begin(), cov.end(), mdl->cov.begin() + m * N * N);
		std::copy(W.begin(), W.end(), mdl->W.begin() + m * N * N);
		mdl->c[m] = c;
	}
}

}  // namespace wc
