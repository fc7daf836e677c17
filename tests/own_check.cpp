// A stand-alone check of the owning buffer type (bwa-mem-gpu_amd/csrc/own.h): built by tests/test_own_cpu.py with
// -fsanitize=address,undefined and run as a child process.  Buf is instantiated on a fake of malloc / free that counts what is alive
// and what was ever allocated and can be told to refuse the next allocation; a second fake differs in the slack alone.  After every
// step the owner's tally must be the sum of its buffers' capacities.  Prints "ok" and returns 0, or says what went wrong; the
// sanitizer's leak check has the last word on what is alive at exit.
#include "own.h"
#include <stdlib.h>
#include <type_traits>
#include <utility>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

struct Counts { long live = 0, live_bytes = 0, allocs = 0, frees = 0, syncs = 0; bool fail_next = false; };
static Counts g;

template <size_t SLACK> struct FakeMemT {
	static constexpr size_t slack = SLACK;
	static constexpr const char *what = "fake_alloc";
	static void *alloc(size_t bytes)
	{
		if (g.fail_next) { g.fail_next = false; return nullptr; }
		void *p = malloc(bytes ? bytes : 1);
		if (p) { ++g.live; g.live_bytes += (long)bytes; ++g.allocs; }
		return p;
	}
	static void free(void *p, size_t bytes) { ::free(p); --g.live; g.live_bytes -= (long)bytes; ++g.frees; }
	static void count_sync() { ++g.syncs; }
};
using FakeMem = FakeMemT<256>;
using FBuf = Buf<FakeMem>;
using PBuf = Buf<FakeMemT<4096>>;

static_assert(!std::is_copy_constructible<FBuf>::value && !std::is_copy_assignable<FBuf>::value, "a buffer is not copied");
static_assert(std::is_nothrow_move_constructible<FBuf>::value && std::is_nothrow_move_assignable<FBuf>::value, "a buffer moves");

struct Owner {
	Tally hbm;
	FBuf a{hbm}, b{hbm}, c[2] = { FBuf{hbm}, FBuf{hbm} };
	size_t sum() const { return a.cap + b.cap + c[0].cap + c[1].cap; }
};
#define TALLY(o) CHECK((o).hbm.bytes == (o).sum())

static int growth_and_exact()
{
	Owner o;
	CHECK(o.a.ensure(1000) == 0 && o.a.p && o.a.cap == 1000 + 125 + 256 && g.allocs == 1 && g.syncs == 1);
	TALLY(o);
	void *p = o.a.p;
	CHECK(o.a.ensure(1381) == 0 && o.a.ensure(0) == 0 && o.a.ensure(7) == 0 && o.a.p == p && g.allocs == 1 && g.syncs == 1);   // within capacity: nothing
	CHECK(o.a.ensure(1382) == 0 && o.a.cap == 1382 + 172 + 256 && g.allocs == 2 && g.frees == 1 && g.live == 1 && g.syncs == 2);   // growth frees the old block, counts once
	TALLY(o);
	CHECK(g.live_bytes == (long)o.a.cap);
	PBuf h;                                                         // the pinned rule: the other constant
	CHECK(h.ensure(1000) == 0 && h.cap == 1000 + 125 + 4096);
	CHECK(h.ensure(80000) == 0 && h.cap == 80000 + 10000 + 4096 && g.live == 2);
	FBuf e;
	CHECK(e.ensure(0) == 0 && !e.p && e.cap == 0);                  // nothing asked of an empty buffer: nothing allocated
	// exact: to size, counted when made and when freed
	const long s0 = g.syncs;
	CHECK(o.b.alloc_exact(777) == 0 && o.b.cap == 777 && o.b.p && g.syncs == s0 + 1);
	TALLY(o);
	CHECK(o.c[0].alloc_exact(0) == 0 && o.c[0].cap == 0 && o.c[0].p && g.syncs == s0 + 2);   // usable: a valid block of no bytes
	TALLY(o);
	o.c[0].release();
	CHECK(!o.c[0].p && g.syncs == s0 + 3);
	o.b.release();
	CHECK(g.syncs == s0 + 4 && g.live == 2);
	TALLY(o);
	CHECK(o.b.alloc_exact(10) == 0 && o.b.alloc_exact(20) == 0 && o.b.cap == 20 && g.live == 3);   // over a live exact block: that one freed first
	CHECK(o.b.ensure(5) == 0 && o.b.cap == 20);                     // within capacity
	CHECK(o.b.ensure(21) == 0 && o.b.cap == 21 + 2 + 256 && g.live == 3);
	TALLY(o);
	return 0;
}

static int release_and_adopt()
{
	const long live0 = g.live, frees0 = g.frees;
	char mine[64], yours[32];
	{
		Owner o;
		CHECK(o.a.ensure(100) == 0);
		o.a.release(); o.a.release();                                // twice is fine
		CHECK(!o.a.p && o.a.cap == 0 && g.live == live0 && g.frees == frees0 + 1);
		TALLY(o);
		o.a.adopt(mine, sizeof mine);
		CHECK(o.a.p == mine && o.a.cap == 64 && g.live == live0);
		TALLY(o);
		CHECK(o.a.ensure(10) == 0 && o.a.p != mine && o.a.cap == 10 + 1 + 256 && g.live == live0 + 1 && g.frees == frees0 + 1);   // afresh, even within the adopted size; the adopted pointer is forgotten, not freed
		TALLY(o);
		o.a.adopt(yours, sizeof yours);                              // over a live block: that block is freed
		CHECK(o.a.p == yours && g.live == live0 && g.frees == frees0 + 2);
		TALLY(o);
		o.b.adopt(mine, sizeof mine);
		o.b.release();
		CHECK(!o.b.p && g.frees == frees0 + 2);
		o.b.adopt(mine, sizeof mine);                                // and destroyed while adopted
		TALLY(o);
	}
	CHECK(g.live == live0 && g.frees == frees0 + 2);                // adopt, then destroy: nothing freed
	return 0;
}

static int moves()
{
	const long live0 = g.live;
	Owner o;
	CHECK(o.a.ensure(500) == 0 && o.b.ensure(300) == 0);
	void *pa = o.a.p, *pb = o.b.p;
	const size_t ca = o.a.cap;
	FBuf m(std::move(o.a));                                         // construction: the source is empty and weighs nothing
	CHECK(m.p == pa && m.cap == ca && !o.a.p && o.a.cap == 0 && g.live == live0 + 2);
	TALLY(o);
	CHECK(o.hbm.bytes == o.b.cap);                                  // m is bound to no tally
	o.c[0] = std::move(m);                                          // assignment over empty: into the owner's tally
	CHECK(o.c[0].p == pa && !m.p && m.cap == 0 && g.live == live0 + 2);
	TALLY(o);
	CHECK(o.hbm.bytes == ca + o.b.cap);
	o.b = std::move(o.c[0]);                                        // over live: that block is freed first
	CHECK(o.b.p == pa && o.b.cap == ca && !o.c[0].p && g.live == live0 + 1);
	(void)pb;
	TALLY(o);
	FBuf &self = o.b;
	o.b = std::move(self);                                          // self-move: harmless
	CHECK(o.b.p == pa && o.b.cap == ca && g.live == live0 + 1);
	TALLY(o);
	o.a = FBuf();                                                   // an empty one assigned
	CHECK(!o.a.p);
	char ext[16];
	o.a.adopt(ext, sizeof ext);
	FBuf t(std::move(o.a));                                         // an adopted pointer stays adopted through a move
	CHECK(t.p == ext && !o.a.p);
	TALLY(o);
	t.release();
	CHECK(g.live == live0 + 1);
	{
		std::vector<FBuf> v;                                         // reallocates several times
		for (int i = 0; i < 40; ++i) { v.emplace_back(); CHECK((i & 1 ? v.back().alloc_exact((size_t)i) : v.back().ensure((size_t)i * 10 + 1)) == 0); }
		CHECK(g.live == live0 + 1 + 40);
		for (int i = 0; i < 40; ++i) CHECK(v[(size_t)i].p && v[(size_t)i].cap == (i & 1 ? (size_t)i : (size_t)i * 10 + 1 + (size_t)(i * 10 + 1) / 8 + 256));
		v.erase(v.begin() + 3, v.begin() + 20);
		CHECK(g.live == live0 + 1 + 23);
	}
	CHECK(g.live == live0 + 1);
	Owner q;                                                        // an owner reset by assignment: its buffers freed, the tally the buffers' own doing
	CHECK(q.a.ensure(10) == 0 && q.c[1].alloc_exact(5) == 0);
	q = Owner{};
	CHECK(!q.a.p && !q.c[1].p && q.hbm.bytes == 0 && g.live == live0 + 1);
	CHECK(q.b.ensure(64) == 0);
	TALLY(q);
	return 0;
}

static int failed_allocation()
{
	const long live0 = g.live, syncs0 = g.syncs;
	Owner o;
	g.fail_next = true;
	CHECK(o.a.ensure(100) == BWAHIP_ENOMEM && !o.a.p && o.a.cap == 0 && g.live == live0);
	TALLY(o);
	CHECK(o.a.ensure(100) == 0 && g.live == live0 + 1);             // and the buffer is usable afterwards
	g.fail_next = true;
	CHECK(o.a.ensure(100000) == BWAHIP_ENOMEM && !o.a.p && o.a.cap == 0 && g.live == live0);   // a failed growth: the old block is gone, as the tally says
	TALLY(o);
	CHECK(o.hbm.bytes == 0);
	g.fail_next = true;
	CHECK(o.b.alloc_exact(50) == BWAHIP_ENOMEM && !o.b.p && o.b.cap == 0);
	o.b.release();
	CHECK(g.syncs == syncs0 + 4);                                   // one per attempt; the release of what was never allocated counts nothing
	TALLY(o);
	return 0;
}

int main()
{
	if (growth_and_exact() || release_and_adopt() || moves() || failed_allocation()) return 1;
	CHECK(g.live == 0 && g.live_bytes == 0 && g.allocs == g.frees);  // every owner above is gone
	printf("ok\n");
	return 0;
}
