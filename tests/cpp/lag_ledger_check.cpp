// Drives world_class_amd/csrc/wc_lag_stream.hpp alone, as a host compiler takes it (tests/test_lag_ledger.py builds this plain and
// under the address and undefined-behaviour sanitizers).  Standard input is a script, one call per line:
//   init N R L            a ledger of N streams, max_rows_per_push R, max_lag L (first)
//   reset U LAG           |  push K0 .. K(N-1)  |  flush W0 .. W(N-1)
//   create W N R L D      create's bound check for a row width W and D doubles per ring row (needs no init)
// After every call it prints the refusal, or "ok", the call's frames_out and "/" with the scan's totals, and then rows / emitted /
// lag / ended of every stream.
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../world_class_amd/csrc/wc_lag_stream.hpp"

int main() {
	wc::LagLedger<wc::LagState> g;
	std::string line, op;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		if (!(in >> op)) continue;
		std::vector<long long> a;
		for (long long v; in >> v;) a.push_back(v);
		const int n = g.n_streams;
		std::vector<int> arg(a.begin(), a.end()), out((size_t)n, 0);
		std::vector<long long> totals;
		const char *why = nullptr;
		if (op == "create" && a.size() == 5) {
			why = wc::lag_check_create((int)a[0], (int)a[1], (int)a[2], (int)a[3], (unsigned long long)a[4]);
			std::cout << (why ? why : "ok") << "\n";
			continue;
		}
		if (op == "init" && a.size() == 3) {
			g.init(arg[0], arg[1], arg[2]);
		} else if (op == "reset" && a.size() == 2) {
			if (!(why = wc::lag_check_reset(&g, arg[0], arg[1]))) {
				g.st[arg[0]] = wc::LagState();
				g.st[arg[0]].lag = arg[1];
			}
		} else if (op == "push" && (int)a.size() == n) {
			long long rows, frames;
			if (!(why = g.scan_push(arg.data(), &rows, &frames))) {
				for (int u = 0; u < n; ++u) out[u] = g.push_frames(u, arg[u]);
				g.commit_push(arg.data(), out.data());
				totals = {rows, frames};
			}
		} else if (op == "flush" && (int)a.size() == n) {
			long long frames;
			if (!(why = g.scan_flush(arg.data(), &frames))) {
				for (int u = 0; u < n; ++u) out[u] = g.flush_frames(u, arg[u]);
				g.commit_flush(arg.data(), out.data());
				totals = {frames};
			}
		} else {
			std::cerr << "bad line: " << line << "\n";
			return 2;
		}
		std::cout << (why ? why : "ok");
		for (int u = 0; !totals.empty() && u < n; ++u) std::cout << " " << out[u];
		std::cout << " /";
		for (long long t : totals) std::cout << " " << t;
		for (int u = 0; u < g.n_streams; ++u) {
			const wc::LagState &s = g.st[u];
			std::cout << " | " << wc::lag_rows_received(&g, u) << " " << wc::lag_frames_emitted(&g, u) << " " << wc::lag_get_lag(&g, u) << " " << (s.ended ? 1 : 0);
		}
		std::cout << "\n";
	}
	return 0;
}
