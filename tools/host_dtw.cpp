// What a caller of the parent commit runs on the host instead of wc_align_features_device ("Alignment"): the
// rule of include/world_class_io.h in plain C++, one pair per thread.  A stand-alone program for that one comparison; it times
// itself on seeded random walks of the probe's shape and prints one JSON line.
//   g++ -O2 -ffp-contract=off -pthread tools/host_dtw.cpp -o host_dtw && ./host_dtw [n_pairs] [frames] [band] [threads]
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

namespace {

constexpr int kDims = 60, kDimBegin = 1;

struct Result {
	double cost = 0.0;
	int K = 0;
};

bool allowed(long long i, long long j, long long n, long long m, long long band) {
	if (band == 0) return true;
	const long long L = (n > m ? n : m) - 1, v = i * (m - 1) - j * (n - 1);
	return (v < 0 ? -v : v) <= band * L;
}

Result align(const double *a, int n, const double *b, int m, int band, std::vector<double> &b_on_a, std::vector<double> &a_on_b) {
	const double inf = INFINITY;
	std::vector<double> prev(m, inf), cur(m, inf);
	std::vector<unsigned char> choice((size_t)n * m, 0);
	for (int i = 0; i < n; ++i) {
		for (int j = 0; j < m; ++j) {
			if (!allowed(i, j, n, m, band)) {
				cur[j] = inf;
				continue;
			}
			double s = 0.0;
			for (int c = kDimBegin; c < kDims; ++c) {
				const double d = a[(size_t)i * kDims + c] - b[(size_t)j * kDims + c];
				s = s + d * d;
			}
			const double d = std::sqrt(s);
			if (i == 0 && j == 0) {
				cur[0] = d;
				continue;
			}
			const double Dd = i > 0 && j > 0 && allowed(i - 1, j - 1, n, m, band) ? prev[j - 1] : inf;
			const double Du = i > 0 && allowed(i - 1, j, n, m, band) ? prev[j] : inf;
			const double Dl = j > 0 && allowed(i, j - 1, n, m, band) ? cur[j - 1] : inf;
			double best;
			unsigned char c;
			if (Dd <= Du && Dd <= Dl) { best = Dd; c = 0; }
			else if (Du <= Dl) { best = Du; c = 1; }
			else { best = Dl; c = 2; }
			cur[j] = d + best;
			choice[(size_t)i * m + j] = c;
		}
		prev.swap(cur);
	}
	Result r;
	r.cost = prev[m - 1];
	if (!std::isfinite(r.cost)) return r;
	int i = n - 1, j = m - 1, jmax = j, imax = i;
	for (;;) {
		++r.K;
		if (i == 0 && j == 0) break;
		const unsigned char c = choice[(size_t)i * m + j];
		const int ni = c != 2 ? i - 1 : i, nj = c != 1 ? j - 1 : j;
		if (ni != i) { b_on_a[i] = (j + jmax) * 0.5; jmax = nj; }
		if (nj != j) { a_on_b[j] = (i + imax) * 0.5; imax = ni; }
		i = ni; j = nj;
	}
	b_on_a[0] = jmax * 0.5;
	a_on_b[0] = imax * 0.5;
	return r;
}

void walk(std::vector<double> &f, int frames, uint64_t seed) {
	uint64_t s = seed * 0x9e3779b97f4a7c15ull + 1;
	for (int c = 0; c < kDims; ++c) f[c] = 0.0;
	for (size_t k = kDims; k < (size_t)frames * kDims; ++k) {
		s ^= s << 13; s ^= s >> 7; s ^= s << 17;
		f[k] = f[k - kDims] + 0.2 * ((double)(s >> 11) / 9007199254740992.0 - 0.5);
	}
}

}  // namespace

int main(int argc, char **argv) {
	const int n_pairs = argc > 1 ? atoi(argv[1]) : 64, frames = argc > 2 ? atoi(argv[2]) : 2001, band = argc > 3 ? atoi(argv[3]) : 0;
	const int threads = argc > 4 ? atoi(argv[4]) : 16;
	if (n_pairs < 1 || frames < 1 || band < 0 || threads < 1) return 1;
	std::vector<std::vector<double>> a(n_pairs), b(n_pairs);
	for (int u = 0; u < n_pairs; ++u) {
		a[u].resize((size_t)frames * kDims);
		b[u].resize((size_t)frames * kDims);
		walk(a[u], frames, 2 * u + 1);
		walk(b[u], frames, 2 * u + 2);
	}
	std::vector<Result> res(n_pairs);
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<std::thread> pool;
	for (int t = 0; t < threads; ++t)
		pool.emplace_back([&, t] {
			std::vector<double> b_on_a(frames), a_on_b(frames);
			for (int u = t; u < n_pairs; u += threads) res[u] = align(a[u].data(), frames, b[u].data(), frames, band, b_on_a, a_on_b);
		});
	for (std::thread &t : pool) t.join();
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	double k = 0.0, cost = 0.0;
	for (const Result &r : res) { k += r.K; cost += r.cost; }
	printf("{\"host_dtw_ms\": %.1f, \"n_pairs\": %d, \"frames\": %d, \"band\": %d, \"threads\": %d, \"mean_path_length\": %.1f, \"mean_cost\": %.3f}\n", ms,
		   n_pairs, frames, band, threads, k / n_pairs, cost / n_pairs);
	return 0;
}
