// Drives world_class_amd/csrc/wc_stage_plan.hpp and wc_options.hpp alone, as a host compiler takes them (tests/test_stage_plan.py
// builds this plain and under the address and undefined-behaviour sanitizers).  Standard input is a script, one call per line:
//   layout MASK N  x f y pos  x f y pos ...   batch_layout of N utterances; MASK: 1 x_length, 2 f0_length, 4 out_length, 8 rng_pos given
//                                             -> "x f y" totals, then " | x_off f_off y_off x_len f_len y_len f_base rng_pos" per utterance
//   draws ct FFT_SIZE F0_LENGTH  |  draws d4c FS F0_LENGTH  |  draws syn OUT_LENGTH       -> the count
//   range  pos draws  pos draws ...   DrawRange::add of each pair     -> "empty 1" (one_table), or "lo hi one_table"
//   starts pos pos ...                DrawRange::add_start of each    -> the same
//   opt READER VALUE [ARG]   READER: is (ARG the word), off, on, int (ARG the default), set; VALUE: "-" unset, else "=" and the text
//                            -> what the reader gives for a variable set that way
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../world_class_amd/csrc/wc_options.hpp"
#include "../../world_class_amd/csrc/wc_stage_plan.hpp"

static void print(const wc::DrawRange &r) {
	if (r.empty()) std::cout << "empty " << (r.one_table() ? 1 : 0) << "\n";
	else std::cout << r.lo << " " << r.hi << " " << (r.one_table() ? 1 : 0) << "\n";
}

int main() {
	const char *kName = "WC_STAGE_PLAN_CHECK_OPTION";
	std::string line, op;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		if (!(in >> op)) continue;
		if (op == "layout") {
			int mask = 0, n = 0;
			in >> mask >> n;
			std::vector<int> x(n), f(n), y(n);
			std::vector<uint64_t> pos(n);
			for (int u = 0; u < n; ++u) in >> x[u] >> f[u] >> y[u] >> pos[u];
			if (!in) { std::cerr << "bad line: " << line << "\n"; return 2; }
			std::vector<wc::UttDesc> d(n);
			const wc::BatchTotals t = wc::batch_layout(n, mask & 1 ? x.data() : nullptr, mask & 2 ? f.data() : nullptr, mask & 4 ? y.data() : nullptr,
													   mask & 8 ? pos.data() : nullptr, d.data());
			std::cout << t.x << " " << t.f << " " << t.y;
			for (const wc::UttDesc &q : d)
				std::cout << " | " << q.x_off << " " << q.f_off << " " << q.y_off << " " << q.x_len << " " << q.f_len << " " << q.y_len << " " << q.f_base << " " << q.rng_pos;
			std::cout << "\n";
		} else if (op == "draws") {
			std::string stage;
			int a = 0, b = 0;
			in >> stage >> a;
			if (stage != "syn") in >> b;
			if (!in) { std::cerr << "bad line: " << line << "\n"; return 2; }
			std::cout << (stage == "ct" ? wc::cheaptrick_draws(a, b) : stage == "d4c" ? wc::d4c_draws(a, b) : wc::synthesis_draws(a)) << "\n";
		} else if (op == "range") {
			wc::DrawRange r;
			for (uint64_t p, n; in >> p >> n;) r.add(p, n);
			print(r);
		} else if (op == "starts") {
			wc::DrawRange r;
			for (uint64_t p; in >> p;) r.add_start(p);
			print(r);
		} else if (op == "opt") {
			std::string reader, value, arg;
			in >> reader >> value;
			in >> arg;
			if (value == "-") unsetenv(kName);
			else setenv(kName, value.c_str() + 1, 1);
			if (reader == "is") std::cout << (wc::opt_is(kName, arg.c_str()) ? 1 : 0) << "\n";
			else if (reader == "off") std::cout << (wc::opt_off(kName) ? 1 : 0) << "\n";
			else if (reader == "on") std::cout << (wc::opt_on(kName) ? 1 : 0) << "\n";
			else if (reader == "int") std::cout << wc::opt_int(kName, std::atoll(arg.c_str())) << "\n";
			else if (reader == "set") std::cout << (wc::opt_set(kName) ? 1 : 0) << "\n";
			else { std::cerr << "bad line: " << line << "\n"; return 2; }
		} else {
			std::cerr << "bad line: " << line << "\n";
			return 2;
		}
	}
	return 0;
}
