// A copy of the caller's bytes that reaches a device buffer once per set(), however many finishes follow: the host copy, its generation,
// the buffer and the generation the buffer holds.  No HIP here, in the manner of own.h: `B` is the buffer (DevBuf; anything made from a
// Tally) and the policy `Up` uploads -- Up::upload(buffer, bytes, n, what begin() was given) -> 0 or an error -- so the type also
// builds with a plain C++ compiler and a counting fake (tests/upload_once_check.cpp).
#pragma once
#include "own.h"
#include <stdint.h>
#include <vector>

template <class B, class Up> struct UploadOnce {
	std::vector<uint8_t> h; bool held = false;                     // set() gave bytes (null: none, and begin() does nothing)
	uint64_t gen = 0, d_gen = 0;                                   // counts the calls of set(); which of them `d` holds (0: none)
	B d;
	explicit UploadOnce(Tally &t) : d(t) {}
	void set(const uint8_t *p, size_t bytes) { held = p != nullptr; h.assign(p, p + (p ? bytes : 0)); ++gen; }
	// after a failed upload `d` counts as holding nothing: the next begin() uploads again
	template <class... A> int begin(A &&...a)
	{
		if (!held || d_gen == gen) return 0;
		d_gen = 0;
		const int rc = Up::upload(d, (const void*)h.data(), h.size(), a...);
		if (!rc) d_gen = gen;
		return rc;
	}
};
