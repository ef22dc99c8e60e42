// Drives world_class_amd/csrc/wc_parallel_plan.hpp -- the host half of include/world_class_parallel.h -- alone, for
// tests/test_parallel_plan.py: one call per line of standard input, one line of output per call.  Device addresses are plain numbers
// (0 is NULL): nothing is ever read through them.
//   joint n_pairs null_lengths [a b]*  fa lda cola dx  fb ldb colb dy  fo ldo colo  rows_a rows_b path_length path mask_a mask_b joint joint_mask
//   dist  n_pairs null_lengths [a b]*  fa lda cola  fb ldb colb dims  rows_a rows_b path_length path mask_a mask_b sum count cell
//   mask  n_utt null_lengths [n]*  format ld col  margin floor  rows mask
//   lanes D
// -> "ok slots frames_a frames_b / a_off b_off p_off a b / ..." (mask: "ok frames / f_off n / ..."), or "no: " and the refusal's text
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../world_class_amd/csrc/wc_parallel_plan.hpp"

using namespace wc;

static const void *ptr(unsigned long long v) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(v)); }

static bool read_ptrs(std::istringstream &in, int n, const void **out) {
	for (int k = 0; k < n; ++k) {
		unsigned long long v;
		if (!(in >> v)) return false;
		out[k] = ptr(v);
	}
	return true;
}

static void print_pairs(const ParCounts &c, const std::vector<ParPair> &pairs) {
	std::printf("ok %lld %lld %lld", c.slots, c.frames_a, c.frames_b);
	for (const ParPair &p : pairs) std::printf(" / %lld %lld %lld %d %d", p.a_off, p.b_off, p.p_off, p.a, p.b);
	std::printf("\n");
}

int main() {
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string what;
		in >> what;
		std::string why;
		if (what == "lanes") {
			int D;
			in >> D;
			std::printf("%d\n", par_row_lanes(D));
			continue;
		}
		int n = 0, null_lengths = 0;
		in >> n >> null_lengths;
		std::vector<int> a, b;
		for (int u = 0; u < n; ++u) {
			int x = 0, y = 0;
			in >> x;
			if (what != "mask") in >> y;
			a.push_back(x);
			b.push_back(y);
		}
		const int *pa = null_lengths ? nullptr : a.data(), *pb = null_lengths ? nullptr : b.data();
		if (what == "joint") {
			ParJointArgs g = {};
			g.n_pairs = n; g.a_length = pa; g.b_length = pb;
			in >> g.ra.format >> g.ra.ld >> g.ra.col >> g.ra.width >> g.rb.format >> g.rb.ld >> g.rb.col >> g.rb.width >> g.ro.format >> g.ro.ld >> g.ro.col;
			g.ro.width = g.ra.width >= 1 && g.rb.width >= 1 && (long long)g.ra.width + g.rb.width <= kParMaxJoint ? g.ra.width + g.rb.width : 1;
			const void *p[8];
			if (!read_ptrs(in, 8, p)) return 2;
			g.rows_a = p[0]; g.rows_b = p[1]; g.path_length = p[2]; g.path = p[3]; g.mask_a = p[4]; g.mask_b = p[5]; g.joint = p[6]; g.joint_mask = p[7];
			ParCounts c;
			std::vector<ParPair> pairs;
			if (par_joint_plan(g, &c, &pairs, &why)) print_pairs(c, pairs);
			else std::printf("no: %s\n", why.c_str());
		} else if (what == "dist") {
			ParDistArgs g = {};
			g.n_pairs = n; g.a_length = pa; g.b_length = pb;
			in >> g.ra.format >> g.ra.ld >> g.ra.col >> g.rb.format >> g.rb.ld >> g.rb.col >> g.ra.width;
			g.rb.width = g.ra.width;
			const void *p[9];
			if (!read_ptrs(in, 9, p)) return 2;
			g.rows_a = p[0]; g.rows_b = p[1]; g.path_length = p[2]; g.path = p[3]; g.mask_a = p[4]; g.mask_b = p[5]; g.sum = p[6]; g.count = p[7]; g.cell = p[8];
			ParCounts c;
			std::vector<ParPair> pairs;
			if (par_dist_plan(g, &c, &pairs, &why)) print_pairs(c, pairs);
			else std::printf("no: %s\n", why.c_str());
		} else if (what == "mask") {
			ParRows r = {0, 0, 0, 1};
			double margin = 0.0, floor = 0.0;
			std::string ms, fs;
			in >> r.format >> r.ld >> r.col >> ms >> fs;
			margin = std::stod(ms);  // (takes "inf", "-inf" and "nan")
			floor = std::stod(fs);
			const void *p[2];
			if (!read_ptrs(in, 2, p)) return 2;
			long long frames = 0;
			std::vector<ParUtt> utts;
			if (par_mask_plan(n, pa, r, p[0], margin, floor, p[1], &frames, &utts, &why)) {
				std::printf("ok %lld", frames);
				for (const ParUtt &u : utts) std::printf(" / %lld %d", u.f_off, u.n);
				std::printf("\n");
			} else {
				std::printf("no: %s\n", why.c_str());
			}
		} else {
			return 2;
		}
	}
	return 0;
}
