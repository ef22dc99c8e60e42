// The host half of include/world_class_gmm.h: THE rule of create in plain C++, operation for operation (the tree is built with
// -ffp-contract=off, on the host side as well).  No device code and no HIP call: wc_gmm.hip uploads what stands here.
#pragma once
#include <cmath>
#include <string>
#include <vector>

namespace wc {

constexpr int kGmmMaxMix = 1024, kGmmMaxDim = 192;

struct GmmPlan {
	int n_mix = 0, dx = 0, dy = 0;
	std::vector<double> c, W, B, cvar;  // c n_mix; W n_mix*dx*dx row-major, upper part 0.0; B n_mix*dy*dx; cvar n_mix*dy
	std::vector<double> mux, muy;       // n_mix*dx, n_mix*dy
};

inline bool gmm_finite(double v) { return std::fabs(v) <= 1.7976931348623157e308; }  // not NaN, not infinite

// THE rule's Cholesky and W = L^-1 on the n x n matrix whose lower triangle stands in S (row i at S + i * ld): L and W are n x n
// row-major, and only their lower triangles are written.  -> the row whose diagonal s is not > 0 or not finite (L and W are then
// unfinished), or -1.  The conversion applies it to Sxx, the training (wc_gmm_train_plan.hpp) to the whole joint matrix.
inline long gmm_factor(size_t n, const double *S, size_t ld, double *L, double *W) {
	for (size_t i = 0; i < n; ++i)
		for (size_t j = 0; j <= i; ++j) {
			double s = S[i * ld + j];
			for (size_t k = 0; k < j; ++k) s = s - L[i * n + k] * L[j * n + k];
			if (j < i) {
				L[i * n + j] = s / L[j * n + j];
			} else {
				if (!(s > 0.0) || !gmm_finite(s)) return (long)i;
				L[i * n + i] = std::sqrt(s);
			}
		}
	for (size_t j = 0; j < n; ++j) {
		W[j * n + j] = 1.0 / L[j * n + j];
		for (size_t i = j + 1; i < n; ++i) {
			double s = L[i * n + j] * W[j * n + j];
			for (size_t k = j + 1; k < i; ++k) s = s + L[i * n + k] * W[k * n + j];
			W[i * n + j] = -s / L[i * n + i];
		}
	}
	return -1;
}

// c of THE rule for a factor of n rows: (log(w) - ld) - (0.5 * (double)n) * log(2 pi), ld the sum of log L(i,i) ascending
inline double gmm_constant(size_t n, double w, const double *L) {
	double ld = std::log(L[0]);
	for (size_t i = 1; i < n; ++i) ld = ld + std::log(L[i * n + i]);
	return (std::log(w) - ld) - (0.5 * (double)n) * 1.8378770664093453;
}

// fills *p; a refusal leaves its text in *why and returns false
inline bool gmm_prepare(int n_mix, int dx, int dy, const double *weight, const double *mean, const double *cov, GmmPlan *p, std::string *why) {
	const auto no = [&](const std::string &text) { *why = text; return false; };
	if (n_mix < 1 || n_mix > kGmmMaxMix) return no("n_mix outside 1 .. 1024");
	if (dx < 1 || dx > kGmmMaxDim || dy < 1 || dy > kGmmMaxDim) return no("dx and dy lie in 1 .. 192");
	if (!weight || !mean || !cov) return no("null array");
	const size_t D = (size_t)dx + dy, X = (size_t)dx, Y = (size_t)dy;
	const auto at = [](int m, size_t row) { return "mixture " + std::to_string(m) + ", row " + std::to_string(row); };
	for (int m = 0; m < n_mix; ++m) {
		if (!(weight[m] > 0.0) || !gmm_finite(weight[m])) return no("mixture " + std::to_string(m) + ": a weight that is not finite or not > 0");
		for (size_t i = 0; i < D; ++i) {
			if (!gmm_finite(mean[m * D + i])) return no(at(m, i) + ": a mean that is not finite");
			for (size_t j = 0; j <= i; ++j)
				if (!gmm_finite(cov[(m * D + i) * D + j])) return no(at(m, i) + ": a covariance entry that is not finite");
		}
	}
	p->n_mix = n_mix; p->dx = dx; p->dy = dy;
	p->c.assign((size_t)n_mix, 0.0);
	p->W.assign((size_t)n_mix * X * X, 0.0);
	p->B.assign((size_t)n_mix * Y * X, 0.0);
	p->cvar.assign((size_t)n_mix * Y, 0.0);
	p->mux.resize((size_t)n_mix * X);
	p->muy.resize((size_t)n_mix * Y);
	std::vector<double> Lbuf(X * X);
	for (int m = 0; m < n_mix; ++m) {
		const double *S = cov + (size_t)m * D * D;  // Sxx(i,j) = S[i*D + j], Syx(j,i) = S[(dx+j)*D + i], Syy(j,j) = S[(dx+j)*D + dx+j]
		double *L = Lbuf.data(), *W = p->W.data() + (size_t)m * X * X, *B = p->B.data() + (size_t)m * Y * X;
		for (size_t i = 0; i < X; ++i) p->mux[m * X + i] = mean[m * D + i];
		for (size_t j = 0; j < Y; ++j) p->muy[m * Y + j] = mean[m * D + X + j];
		const long bad = gmm_factor(X, S, D, L, W);
		if (bad >= 0) return no(at(m, (size_t)bad) + ": the source covariance is not positive definite (a Cholesky diagonal that is not > 0 or not finite)");
		for (size_t j = 0; j < Y; ++j) {
			const double *Syx = S + (X + j) * D;
			for (size_t k = 0; k < X; ++k) {
				double s = Syx[0] * W[k * X];
				for (size_t i = 1; i <= k; ++i) s = s + Syx[i] * W[k * X + i];
				B[j * X + k] = s;
			}
			double s = Syx[X + j];
			for (size_t k = 0; k < X; ++k) s = s - B[j * X + k] * B[j * X + k];
			if (!(s > 0.0) || !gmm_finite(s)) return no(at(m, X + j) + ": a conditional variance that is not > 0 or not finite");
			p->cvar[m * Y + j] = s;
		}
		p->c[m] = gmm_constant(X, weight[m], L);
	}
	return true;
}

}  // namespace wc
