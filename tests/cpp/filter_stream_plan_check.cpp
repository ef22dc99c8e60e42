// Drives world_class_amd/csrc/wc_filter_stream_plan.hpp alone, as a host compiler takes it (tests/test_filter_stream_plan.py builds this
// plain and under the address and undefined-behaviour sanitizers).  Standard input is a script, one call per line:
//   init FS FP N U S R         a plan of U streams at (fs, frame period, fft_size) with max_pending_samples S, max_pending_rows R (first)
//   push NS0 .. NS(U-1) NR0 .. NR(U-1) FL0 .. FL(U-1)   |   reset STREAM   |   seek STREAM N F   (a stream as if it had received so much)
//   create FS N FP KIND U S R  create's checks (needs no init)
//   count FS FP N F            T(n, F) and C(T)
// After every call it prints the refusal, or "ok" and the call's samples_out, then "/" with the totals (samples, rows, outputs,
// segments, touched streams), and then n, F, T, C, ended, pending samples and pending rows of every stream.
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../world_class_amd/csrc/wc_filter_stream_plan.hpp"

int main() {
	wc::FspPlan g;
	std::vector<wc::FspStep> steps;
	std::string line, op;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		if (!(in >> op)) continue;
		std::vector<double> a;
		for (double v; in >> v;) a.push_back(v);
		const int n = g.n_streams;
		const char *why = nullptr;
		std::vector<long long> totals;
		if (op == "create" && a.size() == 7) {
			const int N = (int)a[1];
			why = wc::ff_check_setting((int)a[0], N == 512 || N == 1024 || N == 2048 || N == 4096, N, a[2]);
			if (!why) why = wc::FspPlan::check_create((int)a[0], N, a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6]);
			std::cout << (why ? why : "ok") << "\n";
			continue;
		}
		if (op == "count" && a.size() == 4) {
			const long long T = wc::fsp_segments_done(a[1], (int)a[0], (long long)a[2], (long long)a[3]);
			std::cout << T << " " << wc::fsp_committed(a[1], (int)a[0], T) << " " << wc::ff_segments((long long)a[2], a[1], (int)a[0]) << "\n";
			continue;
		}
		if (op == "init" && a.size() == 6) {
			g.init((int)a[0], (int)a[2], a[1], (int)a[3], (int)a[4], (int)a[5]);
		} else if (op == "reset" && a.size() == 1) {
			if (g.ok((int)a[0])) g.reset((int)a[0]); else why = "reset: bad stream index";
		} else if (op == "seek" && a.size() == 3 && g.ok((int)a[0])) {
			wc::FspState &s = g.st[(size_t)a[0]];
			s = wc::FspState();
			s.n = (long long)a[1]; s.F = (long long)a[2];
			s.T = wc::fsp_segments_done(g.fp_ms, g.fs, s.n, s.F);
			s.C = wc::fsp_committed(g.fp_ms, g.fs, s.T);
		} else if (op == "push" && (int)a.size() == 3 * n) {
			std::vector<int> v(a.begin(), a.end());
			long long ts, tr, to, tg;
			int act;
			if (!(why = g.plan_push(v.data(), v.data() + n, v.data() + 2 * n, steps, &ts, &tr, &to, &tg, &act))) {
				g.commit(steps);
				totals = {ts, tr, to, tg, act};
			}
		} else {
			std::cerr << "bad line: " << line << "\n";
			return 2;
		}
		std::cout << (why ? why : "ok");
		for (int u = 0; !totals.empty() && u < n; ++u) std::cout << " " << steps[(size_t)u].out;
		std::cout << " /";
		for (long long t : totals) std::cout << " " << t;
		for (int u = 0; u < g.n_streams; ++u) {
			const wc::FspState &s = g.st[(size_t)u];
			std::cout << " | " << s.n << " " << s.F << " " << s.T << " " << s.C << " " << (s.ended ? 1 : 0) << " " << g.pending_samples(u) << " " << g.pending_rows(u);
		}
		std::cout << "\n";
	}
	return 0;
}
