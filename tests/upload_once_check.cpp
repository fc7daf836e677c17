// A stand-alone check of the upload-once type (bwa-mem-gpu_amd/csrc/upload_once.h), which the pileup and recalibration stages hold their
// packed reference and their mask in: built by tests/test_upload_once_cpu.py with -fsanitize=address,undefined and run as a child
// process.  The buffer is own.h's on a fake of malloc / free, the upload policy a memcpy that counts its calls and can be told to fail.  Prints
// "ok" and returns 0, or says what went wrong; the sanitizer's leak check has the last word on what is alive at exit.
#include "upload_once.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static long g_live = 0;
struct FakeMem {
	static constexpr size_t slack = 256;
	static constexpr const char *what = "fake_alloc";
	static void *alloc(size_t bytes) { void *p = malloc(bytes ? bytes : 1); if (p) ++g_live; return p; }
	static void free(void *p, size_t) { ::free(p); --g_live; }
	static void count_sync() {}
};
using FBuf = Buf<FakeMem>;

struct Upload { int calls = 0; bool fail_next = false; };       // what begin() is given, as the stages give their stream
struct FakeUpload {
	static int upload(FBuf &b, const void *src, size_t n, Upload &u)
	{
		++u.calls;
		if (u.fail_next) { u.fail_next = false; return BWAHIP_ENODEV; }
		const int rc = b.ensure(n);
		if (!rc && n) memcpy(b.p, src, n);
		return rc;
	}
};

struct Owner {
	Tally hbm;
	UploadOnce<FBuf, FakeUpload> ref{hbm}, mask{hbm};
};

static int run()
{
	Owner o;
	Upload up;
	const uint8_t a[5] = { 1, 2, 3, 4, 5 }, b[3] = { 9, 8, 7 };
	// nothing set: nothing uploaded, nothing allocated
	CHECK(o.ref.begin(up) == 0 && o.ref.begin(up) == 0 && up.calls == 0 && !o.ref.d.p && !o.ref.held && o.hbm.bytes == 0);
	// one upload per set, however many begins
	o.ref.set(a, sizeof a);
	CHECK(o.ref.held && o.ref.h.size() == 5 && up.calls == 0);      // set alone uploads nothing
	for (int k = 0; k < 4; ++k) CHECK(o.ref.begin(up) == 0);
	CHECK(up.calls == 1 && o.ref.d.p && !memcmp(o.ref.d.p, a, 5) && o.hbm.bytes == o.ref.d.cap);
	o.ref.set(b, sizeof b);                                          // other bytes, the same bytes: a set is a set
	CHECK(o.ref.begin(up) == 0 && o.ref.begin(up) == 0 && up.calls == 2 && !memcmp(o.ref.d.p, b, 3));
	o.ref.set(b, sizeof b);
	CHECK(o.ref.begin(up) == 0 && o.ref.begin(up) == 0 && up.calls == 3);
	// the two of one owner do not share a generation
	o.mask.set(a, sizeof a);
	CHECK(o.mask.begin(up) == 0 && o.ref.begin(up) == 0 && up.calls == 4 && o.hbm.bytes == o.ref.d.cap + o.mask.d.cap);
	// a failed upload: the buffer holds nothing, the next begin uploads again
	o.ref.set(a, sizeof a);
	up.fail_next = true;
	CHECK(o.ref.begin(up) == BWAHIP_ENODEV && up.calls == 5 && o.ref.d_gen == 0);
	CHECK(o.ref.begin(up) == 0 && up.calls == 6 && o.ref.d_gen == o.ref.gen && !memcmp(o.ref.d.p, a, 5));
	CHECK(o.ref.begin(up) == 0 && up.calls == 6);
	// set with null clears the host copy; begin then does nothing, and a later set uploads again
	o.ref.set(nullptr, 0);
	CHECK(!o.ref.held && o.ref.h.empty() && o.ref.begin(up) == 0 && up.calls == 6);
	o.ref.set(a, sizeof a);
	CHECK(o.ref.begin(up) == 0 && up.calls == 7);
	// no bytes held is still held: uploaded once, as nothing
	o.mask.set(a, 0);
	CHECK(o.mask.held && o.mask.h.empty() && o.mask.begin(up) == 0 && o.mask.begin(up) == 0 && up.calls == 8);
	return 0;
}

int main()
{
	if (run()) return 1;
	CHECK(g_live == 0);                                              // the owner is gone, and its buffers with it
	printf("ok\n");
	return 0;
}
