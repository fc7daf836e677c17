// A stand-alone check of what the host parts of the files beside a sorted BAM file share (bwa-mem-gpu_amd/csrc/sidecar_host.h): built by
// tests/test_sidecar_cpu.py with -fsanitize=address,undefined and run as a child process.  The bytes of put32 / put64; write_all to a pipe
// whose reader drains slowly, to no descriptor and to a closed one; check_refs at the edges of a length and of the sum; the latch of the
// builder skeleton.  Prints "ok" and returns 0, or says what went wrong.
#include "sidecar_host.h"
#include <signal.h>
#include <sys/time.h>
#include <thread>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static volatile sig_atomic_t ticks = 0;                          // the timer's signals that arrived

static int check_put()
{
	std::vector<uint8_t> o;
	o.reserve(12);
	put32(o, 0x04030201u); put64(o, 0x0c0b0a0908070605ull);
	CHECK(o.size() == 12);
	for (size_t k = 0; k < 12; ++k) CHECK(o[k] == k + 1);
	std::vector<uint8_t> p;                                        // without reserved room: the same bytes
	put64(p, ~0ull); put32(p, 0x80000000u);
	CHECK(p.size() == 12 && p[7] == 0xff && p[8] == 0 && p[11] == 0x80);
	return 0;
}

static int check_write_all()
{
	// A pipe holds less than this, and the reader takes 1 to 4 099 bytes at a time with a pause now and then: the write blocks.  A timer's
	// signal, handled without SA_RESTART and by this thread alone, ends it again and again -- with what it has written so far (a short
	// write), or with EINTR
	const size_t N = (1u << 20) + 12345;
	std::vector<uint8_t> src(N), got;
	for (size_t k = 0; k < N; ++k) src[k] = (uint8_t)(k * 2654435761u >> 13);
	int fds[2];
	CHECK(pipe(fds) == 0);
	struct sigaction sa;
	memset(&sa, 0, sizeof sa);
	sa.sa_handler = [](int) { ++ticks; };
	CHECK(sigaction(SIGALRM, &sa, nullptr) == 0);
	sigset_t alrm;
	sigemptyset(&alrm); sigaddset(&alrm, SIGALRM);
	CHECK(pthread_sigmask(SIG_BLOCK, &alrm, nullptr) == 0);        // the reader inherits the mask
	std::thread reader([&] {
		std::vector<uint8_t> buf(4099);
		unsigned seed = 5;
		for (;;) {
			seed = seed * 1664525u + 1013904223u;
			const ssize_t r = read(fds[0], buf.data(), 1 + (seed >> 8) % 4099);
			if (r <= 0) break;
			got.insert(got.end(), buf.data(), buf.data() + r);
			if ((seed >> 20 & 7) == 0) usleep(100);
		}
	});
	CHECK(pthread_sigmask(SIG_UNBLOCK, &alrm, nullptr) == 0);
	const itimerval on = { { 0, 150 }, { 0, 150 } }, off = { { 0, 0 }, { 0, 0 } };
	CHECK(setitimer(ITIMER_REAL, &on, nullptr) == 0);
	const int rc = write_all(fds[1], src.data(), (int64_t)N, "writing to the pipe");
	CHECK(setitimer(ITIMER_REAL, &off, nullptr) == 0);
	close(fds[1]);
	reader.join();
	close(fds[0]);
	CHECK(rc == 0 && got == src && ticks > 0);
	// no descriptor: nothing is written, whatever the pointer
	CHECK(write_all(-1, src.data(), (int64_t)N, "writing nowhere") == 0 && write_all(-1, nullptr, 5, nullptr) == 0);
	CHECK(write_all(fds[1], src.data(), 0, nullptr) == 0);         // nothing to write: the descriptor is not looked at
	// a closed descriptor, and a pipe nobody reads: BWAHIP_EIO, with and without the message
	CHECK(write_all(fds[1], src.data(), 10, nullptr) == BWAHIP_EIO);
	int q[2];
	CHECK(pipe(q) == 0);
	close(q[0]);
	signal(SIGPIPE, SIG_IGN);
	CHECK(write_all(q[1], src.data(), 10, nullptr) == BWAHIP_EIO);
	close(q[1]);
	return 0;
}

static int check_check_refs()
{
	const int64_t cap = 1ll << 40, top = 0x7fffffffll;
	int64_t sum = -1;
	CHECK(check_refs(0, nullptr, &sum, cap) == 0 && sum == 0);
	CHECK(check_refs(0, nullptr, nullptr, NO_SUM_CAP) == 0);
	CHECK(check_refs(-1, nullptr, &sum, NO_SUM_CAP) == BWAHIP_EINVAL && check_refs(1, nullptr, &sum, NO_SUM_CAP) == BWAHIP_EINVAL);
	const int64_t edge[3] = { top, 0, top + 1 };
	CHECK(check_refs(2, edge, &sum, cap) == 0 && sum == top);
	sum = -1;
	CHECK(check_refs(3, edge, &sum, cap) == BWAHIP_EINVAL && sum == -1);   // 2^31: refused, the sum is left alone
	const int64_t neg[2] = { 5, -1 };
	CHECK(check_refs(2, neg, &sum, NO_SUM_CAP) == BWAHIP_EINVAL);
	// 512 contigs of 2^31 - 1 and one more: 2^40 - 1 in all, then 2^40
	std::vector<int64_t> len(512, top);
	len.push_back(511);
	CHECK(check_refs(513, len.data(), &sum, cap) == 0 && sum == cap - 1);
	len.back() = 512;
	sum = -1;
	CHECK(check_refs(513, len.data(), &sum, cap) == BWAHIP_ECAPACITY && sum == -1);
	CHECK(check_refs(513, len.data(), &sum, NO_SUM_CAP) == 0 && sum == cap);
	len[7] = top + 1;                                              // a bad length counts before the sum
	CHECK(check_refs(513, len.data(), &sum, cap) == BWAHIP_EINVAL);
	return 0;
}

// a builder of the skeleton: it counts records, refuses a record of 3 bytes with BWAHIP_ECAPACITY, and its file is the count as one word
struct Counter : SidecarBuilder { int64_t n = 0; int made = 0; };
static int count_one(Counter *b, const uint8_t *, int64_t len) { if (len == 3) return BWAHIP_ECAPACITY; ++b->n; return 0; }
static int count_bytes(Counter *b, std::vector<uint8_t> *bytes) { ++b->made; put64(*bytes, (uint64_t)b->n); return 0; }
static int count_fails(Counter *b, std::vector<uint8_t> *) { ++b->made; return BWAHIP_EINTERNAL; }

static int check_builder()
{
	const uint8_t rec[16] = { 0 };
	const int64_t good[5] = { 0, 1, 3, 7, 12 }, bad_len[5] = { 0, 1, 3, 7, 10 }, back[4] = { 0, 2, 1, 3 }, below[2] = { -1, 2 };
	int fds[2];
	CHECK(pipe(fds) == 0);
	{
		Counter b;
		const int64_t lens[2] = { 5, 6 };
		const uint8_t pac[3] = { 1, 2, 3 };
		b.set_refs(2, lens, pac);
		CHECK(b.n_ref == 2 && b.ref_off.size() == 3 && b.ref_off[2] == 11 && b.pac.size() == 3 && b.ref_len[1] == 6);
		CHECK(builder_feed((Counter*)nullptr, rec, good, 4, count_one) == BWAHIP_EINVAL);
		CHECK(builder_feed(&b, rec, good, -1, count_one) == BWAHIP_EINVAL && builder_feed(&b, nullptr, good, 4, count_one) == BWAHIP_EINVAL && builder_feed(&b, rec, nullptr, 4, count_one) == BWAHIP_EINVAL);
		CHECK(b.err == 0 && builder_feed(&b, nullptr, nullptr, 0, count_one) == 0);   // bad arguments do not stay
		CHECK(builder_feed(&b, rec, good, 4, count_one) == 0 && b.n == 4);
		CHECK(builder_finish(&b, fds[1], "writing the count", count_bytes) == 0 && b.made == 1);
		uint64_t word = 0;
		CHECK(read(fds[0], &word, 8) == 8 && word == 4);
		CHECK(builder_finish(&b, fds[1], "writing the count", count_bytes) == BWAHIP_EINVAL && b.made == 1);   // a second finish
		CHECK(builder_feed(&b, rec, good, 4, count_one) == BWAHIP_EINVAL && b.n == 4);
		CHECK(builder_finish((Counter*)nullptr, -1, nullptr, count_bytes) == BWAHIP_EINVAL);
	}
	{                                                              // record 3 of the call is refused: records 0 to 2 are counted, the code stays
		Counter b;
		CHECK(builder_feed(&b, rec, good, 2, count_one) == 0 && b.n == 2);
		CHECK(builder_feed(&b, rec, bad_len, 4, count_one) == BWAHIP_ECAPACITY && b.n == 5 && b.err == BWAHIP_ECAPACITY);
		CHECK(builder_feed(&b, rec, good, 4, count_one) == BWAHIP_ECAPACITY && b.n == 5);
		CHECK(builder_feed(&b, rec, good, 0, count_one) == BWAHIP_ECAPACITY);
		CHECK(builder_finish(&b, fds[1], "writing the count", count_bytes) == BWAHIP_ECAPACITY && b.made == 0 && !b.finished);
		CHECK(builder_finish(&b, fds[1], "writing the count", count_bytes) == BWAHIP_ECAPACITY);
	}
	{                                                              // offsets that go back, after one good record; an offset below zero
		Counter b;
		CHECK(builder_feed(&b, rec, back, 3, count_one) == BWAHIP_EINVAL && b.n == 1);
		CHECK(builder_feed(&b, rec, good, 4, count_one) == BWAHIP_EINVAL && b.n == 1);
		Counter d;
		CHECK(builder_feed(&d, rec + 1, below, 1, count_one) == BWAHIP_EINVAL && d.n == 0 && d.err == BWAHIP_EINVAL);
	}
	{                                                              // a finish that fails stays failed: in the making, in the writing
		Counter b;
		CHECK(builder_finish(&b, -1, nullptr, count_fails) == BWAHIP_EINTERNAL && b.finished);
		CHECK(builder_finish(&b, -1, nullptr, count_bytes) == BWAHIP_EINVAL && builder_feed(&b, rec, good, 4, count_one) == BWAHIP_EINVAL && b.made == 1);
		Counter w;
		int q[2];
		CHECK(pipe(q) == 0);
		close(q[0]); close(q[1]);
		CHECK(builder_finish(&w, q[1], nullptr, count_bytes) == BWAHIP_EIO && w.err == BWAHIP_EIO);
		Counter nowhere;
		CHECK(builder_finish(&nowhere, -1, nullptr, count_bytes) == 0 && nowhere.made == 1);
	}
	close(fds[0]); close(fds[1]);
	return 0;
}

int main()
{
	if (check_put() || check_write_all() || check_check_refs() || check_builder()) return 1;
	printf("ok\n");
	return 0;
}
