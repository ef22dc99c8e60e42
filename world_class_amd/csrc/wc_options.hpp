// The development options of the stage handles (environment variables read once, when a handle is created) have four spellings,
// and each create reads its options through these in one function at its top.  Plain C++ (tests/cpp/stage_plan_check.cpp).
#pragma once
#include <cstdlib>
#include <cstring>

namespace wc {

// set, and equal to the word exactly
inline bool opt_is(const char *name, const char *word) {
	const char *v = std::getenv(name);
	return v && std::strcmp(v, word) == 0;
}
// set, and the first character is '0' (switches that are on by default: "0", "00", "0x" turn them off, "" does not)
inline bool opt_off(const char *name) {
	const char *v = std::getenv(name);
	return v && v[0] == '0';
}
// set, and the first character is '1' (switches that are off by default)
inline bool opt_on(const char *name) {
	const char *v = std::getenv(name);
	return v && v[0] == '1';
}
// atoll of the value when set (leading digits; "" and words give 0), else the default
inline long long opt_int(const char *name, long long otherwise) {
	const char *v = std::getenv(name);
	return v ? std::atoll(v) : otherwise;
}
// set at all, to whatever
inline bool opt_set(const char *name) { return std::getenv(name) != nullptr; }

}  // namespace wc
