// Owned memory: one grow-only buffer type for device and pinned host memory.  No HIP here: the policy `Mem` allocates (ctx_internal.h
// has the two HIP ones), so the template also builds with a plain C++ compiler and a counting fake (tests/own_check.cpp).
//   Mem::alloc(bytes)      the block (bytes == 0: a valid one), or nullptr -- nothing of the failure may linger in the runtime's error state
//   Mem::free(p, bytes)    with the bytes alloc was given
//   Mem::slack             what ensure() adds to bytes + bytes / 8 when it grows
//   Mem::what              the allocator's name in the failure message
//   Mem::count_sync()      an allocation or a free that synchronises the device has happened (g_bwahip_reallocs)
#pragma once
#include "../../include/bwahip.h"
#include <stddef.h>
#include <stdio.h>
#include <type_traits>

// The bytes of the buffers bound to it (Buf's constructor): always the sum of their `cap`.  A type that holds one is default-constructed
// and assigned, never copied or move-constructed (its buffers point at the tally); assignment leaves the figure to the buffers' moves.
struct Tally {
	size_t bytes = 0;
	Tally() = default;
	Tally(const Tally&) = delete;
	Tally &operator=(const Tally&) { return *this; }
};

// Move-only; the destructor frees.  ensure() grows with slack and never shrinks; alloc_exact() allocates to size (a sorted run: counted
// once when made and once when freed, as both synchronise the device); adopt() points at memory of somebody else, which is never freed.
template <class Mem> struct Buf {
	void *p = nullptr; size_t cap = 0;
	Buf() = default;
	explicit Buf(Tally &t) : tally(&t) {}
	Buf(const Buf&) = delete;
	Buf &operator=(const Buf&) = delete;
	Buf(Buf &&o) noexcept { take(o); }                              // bound to no tally: the bytes leave o's
	Buf &operator=(Buf &&o) noexcept { if (this != &o) { release(); take(o); } return *this; }   // keeps its own tally
	~Buf()
	{
		static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "a buffer has one owner");
		release();
	}
	int ensure(size_t bytes) { return bytes <= cap && !ext ? 0 : fresh(bytes + bytes / 8 + Mem::slack, false); }
	int alloc_exact(size_t bytes) { return fresh(bytes, true); }
	void adopt(void *mem, size_t bytes) { release(); p = mem; set_cap(bytes); ext = true; }
	void release()
	{
		if (p && !ext) { Mem::free(p, cap); if (exact) Mem::count_sync(); }
		p = nullptr; set_cap(0); ext = exact = false;
	}
	template <class T> T *as() const { return (T*)p; }
private:
	Tally *tally = nullptr; bool ext = false, exact = false;
	void set_cap(size_t n) { if (tally) tally->bytes += n - cap; cap = n; }
	int fresh(size_t want, bool is_exact)
	{
		release();
		Mem::count_sync();
		if (!(p = Mem::alloc(want))) { fprintf(stderr, "[bwahip] %s(%zu) failed\n", Mem::what, want); return BWAHIP_ENOMEM; }
		set_cap(want); exact = is_exact;
		return 0;
	}
	void take(Buf &o)
	{
		p = o.p; set_cap(o.cap); ext = o.ext; exact = o.exact;
		o.p = nullptr; o.set_cap(0); o.ext = o.exact = false;
	}
};
