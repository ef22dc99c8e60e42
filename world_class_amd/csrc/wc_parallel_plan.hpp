// The host half of include/world_class_parallel.h in plain C++: the pairs' offsets into the packed rows and the packed path, the counts,
// and every refusal that needs no device.  No device code and no HIP call: wc_parallel.hip uploads what stands here.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace wc {

constexpr long long kParMaxSlots = 0x7fffffffll;    // path slots of one call at the most
constexpr long long kParMaxFrames = 0xffffffffll;   // frames of one side (or of one speech-mask call) at the most
constexpr int kParMaxJoint = 384;                   // dx + dy at the most

// pair u on the device: its first row of A and of B, its first path slot, its lengths.  cap = a + b - 1
struct ParPair {
	long long a_off, b_off, p_off;
	int a, b;
};

// utterance u of the speech mask: its first frame and its length
struct ParUtt {
	long long f_off;
	int n, pad;
};

struct ParCounts {
	long long slots = 0, frames_a = 0, frames_b = 0;
};

// a row argument: columns [col, col + width) of rows of ld elements of format
struct ParRows {
	int format, ld, col, width;
};

inline bool par_no(std::string *why, const std::string &text) {
	*why = text;
	return false;
}

// whether two byte ranges share a byte; a NULL or empty range shares none
inline bool par_overlap(const void *a, unsigned long long a_bytes, const void *b, unsigned long long b_bytes) {
	if (!a || !b || !a_bytes || !b_bytes) return false;
	const unsigned long long x = (unsigned long long)(uintptr_t)a, y = (unsigned long long)(uintptr_t)b;
	return x < y + b_bytes && y < x + a_bytes;
}

inline unsigned long long par_esz(int format) { return format == 1 ? 4ull : 8ull; }

// the bytes from the first element read or written of `rows` rows to the last: (rows - 1) * ld + width elements
inline unsigned long long par_span(long long rows, const ParRows &r) {
	return rows < 1 ? 0ull : ((unsigned long long)(rows - 1) * (unsigned long long)r.ld + (unsigned long long)r.width) * par_esz(r.format);
}

// the first byte read or written
inline const void *par_first(const void *base, const ParRows &r) {
	return base ? static_cast<const char *>(base) + (size_t)r.col * par_esz(r.format) : nullptr;
}

// format, column, width and ld of one row argument, named `what` in the text
inline bool par_check_rows(const char *what, const ParRows &r, std::string *why) {
	const std::string w(what);
	if (r.format != 0 && r.format != 1) return par_no(why, w + ": the format is 0 (double) or 1 (float)");
	if (r.col < 0) return par_no(why, w + ": a negative column");
	if (r.width < 1) return par_no(why, w + ": fewer than 1 column");
	if ((long long)r.ld < (long long)r.col + (long long)r.width) return par_no(why, w + ": ld is smaller than col plus the width");
	return true;
}

// the pairs of a call: counts, and -- where `out` is given -- the descriptors.  Refuses a negative count, a NULL length array with
// pairs to do, a length below 1, more than 2^31 - 1 slots and more than 2^32 - 1 frames of one side
inline bool par_pairs(int n_pairs, const int *a_length, const int *b_length, ParCounts *counts, std::vector<ParPair> *out, std::string *why) {
	if (n_pairs < 0) return par_no(why, "a negative pair count");
	if (n_pairs > 0 && (!a_length || !b_length)) return par_no(why, "null length array");
	ParCounts c;
	if (out) out->clear();
	for (int u = 0; u < n_pairs; ++u) {
		const int a = a_length[u], b = b_length[u];
		if (a < 1 || b < 1) return par_no(why, "pair " + std::to_string(u) + ": a length below 1");
		if (out) out->push_back(ParPair{c.frames_a, c.frames_b, c.slots, a, b});
		c.frames_a += a;
		c.frames_b += b;
		c.slots += (long long)a + b - 1;
		if (c.slots > kParMaxSlots) return par_no(why, "more than 2^31 - 1 path slots in one call");
		if (c.frames_a > kParMaxFrames || c.frames_b > kParMaxFrames) return par_no(why, "more than 2^32 - 1 frames in one call");
	}
	*counts = c;
	return true;
}

// the utterances of a speech-mask call
inline bool par_utts(int n_utt, const int *lengths, long long *frames, std::vector<ParUtt> *out, std::string *why) {
	if (n_utt < 0) return par_no(why, "a negative utterance count");
	if (n_utt > 0 && !lengths) return par_no(why, "null length array");
	long long total = 0;
	if (out) out->clear();
	for (int u = 0; u < n_utt; ++u) {
		if (lengths[u] < 0) return par_no(why, "utterance " + std::to_string(u) + ": a negative length");
		if (out) out->push_back(ParUtt{total, lengths[u], 0});
		total += lengths[u];
		if (total > kParMaxFrames) return par_no(why, "more than 2^32 - 1 frames in one call");
	}
	*frames = total;
	return true;
}

// ---- wc_joint_rows_device ---------------------------------------------------------------------------------------------------------
struct ParJointArgs {
	int n_pairs;
	const int *a_length, *b_length;
	ParRows ra, rb, ro;  // ra.width = dx, rb.width = dy, ro.width = dx + dy
	const void *rows_a, *rows_b, *path_length, *path, *mask_a, *mask_b;
	const void *joint, *joint_mask;
};

// every refusal of the joint rows; *counts and *pairs are filled where it holds.  counts->slots == 0: nothing to do
inline bool par_joint_plan(const ParJointArgs &g, ParCounts *counts, std::vector<ParPair> *pairs, std::string *why) {
	if (g.n_pairs < 0) return par_no(why, "a negative pair count");
	if (!par_check_rows("A", g.ra, why) || !par_check_rows("B", g.rb, why)) return false;
	if ((long long)g.ra.width + g.rb.width > kParMaxJoint) return par_no(why, "dx + dy is larger than 384");
	if (!par_check_rows("the joint rows", g.ro, why)) return false;
	if (!par_pairs(g.n_pairs, g.a_length, g.b_length, counts, pairs, why)) return false;
	if (g.n_pairs == 0) return true;
	if (!g.rows_a || !g.rows_b || !g.path_length || !g.path || !g.joint) return par_no(why, "null array");
	const unsigned long long out_bytes = par_span(counts->slots, g.ro), omask_bytes = (unsigned long long)counts->slots;
	const void *out0 = par_first(g.joint, g.ro);
	if (par_overlap(out0, out_bytes, g.joint_mask, omask_bytes)) return par_no(why, "the two outputs overlap");
	const struct { const void *p; unsigned long long bytes; } in[] = {
		{par_first(g.rows_a, g.ra), par_span(counts->frames_a, g.ra)}, {par_first(g.rows_b, g.rb), par_span(counts->frames_b, g.rb)},
		{g.path_length, 4ull * g.n_pairs}, {g.path, 8ull * counts->slots},
		{g.mask_a, (unsigned long long)counts->frames_a}, {g.mask_b, (unsigned long long)counts->frames_b}};
	for (const auto &r : in)
		if (par_overlap(out0, out_bytes, r.p, r.bytes) || par_overlap(g.joint_mask, omask_bytes, r.p, r.bytes))
			return par_no(why, "an output overlaps an input");
	return true;
}

// ---- wc_speech_mask_device --------------------------------------------------------------------------------------------------------
inline bool par_mask_plan(int n_utt, const int *lengths, const ParRows &r, const void *rows, double margin, double floor, const void *mask,
						  long long *frames, std::vector<ParUtt> *utts, std::string *why) {
	if (n_utt < 0) return par_no(why, "a negative utterance count");
	if (!par_check_rows("the rows", r, why)) return false;
	if (margin != margin || floor != floor) return par_no(why, "margin or floor is NaN");
	if (margin < 0.0) return par_no(why, "margin is negative");
	if (!par_utts(n_utt, lengths, frames, utts, why)) return false;
	if (*frames == 0) return true;
	if (!rows || !mask) return par_no(why, "null array");
	if (par_overlap(mask, (unsigned long long)*frames, par_first(rows, r), par_span(*frames, r))) return par_no(why, "the mask overlaps the rows");
	return true;
}

// ---- wc_path_distortion_device ----------------------------------------------------------------------------------------------------
struct ParDistArgs {
	int n_pairs;
	const int *a_length, *b_length;
	ParRows ra, rb;  // both of width dims
	const void *rows_a, *rows_b, *path_length, *path, *mask_a, *mask_b;
	const void *sum, *count, *cell;
};

inline bool par_dist_plan(const ParDistArgs &g, ParCounts *counts, std::vector<ParPair> *pairs, std::string *why) {
	if (g.n_pairs < 0) return par_no(why, "a negative pair count");
	if (!par_check_rows("A", g.ra, why) || !par_check_rows("B", g.rb, why)) return false;
	if (!par_pairs(g.n_pairs, g.a_length, g.b_length, counts, pairs, why)) return false;
	if (g.n_pairs == 0) return true;
	if (!g.rows_a || !g.rows_b || !g.path_length || !g.path) return par_no(why, "null array");
	if (!g.sum && !g.count && !g.cell) return par_no(why, "all three outputs are NULL");
	const struct { const void *p; unsigned long long bytes; } out[] = {
		{g.sum, 8ull * g.n_pairs}, {g.count, 8ull * g.n_pairs}, {g.cell, 8ull * counts->slots}};
	const struct { const void *p; unsigned long long bytes; } in[] = {
		{par_first(g.rows_a, g.ra), par_span(counts->frames_a, g.ra)}, {par_first(g.rows_b, g.rb), par_span(counts->frames_b, g.rb)},
		{g.path_length, 4ull * g.n_pairs}, {g.path, 8ull * counts->slots},
		{g.mask_a, (unsigned long long)counts->frames_a}, {g.mask_b, (unsigned long long)counts->frames_b}};
	for (int x = 0; x < 3; ++x) {
		for (int y = x + 1; y < 3; ++y)
			if (par_overlap(out[x].p, out[x].bytes, out[y].p, out[y].bytes)) return par_no(why, "two outputs overlap");
		for (const auto &r : in)
			if (par_overlap(out[x].p, out[x].bytes, r.p, r.bytes)) return par_no(why, "an output overlaps an input");
	}
	return true;
}

// ---- the launch shape of the gather -----------------------------------------------------------------------------------------------
// lanes of one output row: the smallest power of two that holds D = dx + dy, 64 at the most.  A wavefront holds 64 / lanes rows
inline int par_row_lanes(int D) {
	int g = 1;
	while (g < D && g < 64) g <<= 1;
	return g;
}

}  // namespace wc
