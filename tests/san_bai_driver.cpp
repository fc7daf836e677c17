// The device-free BAI builder (csrc/bai_host.cpp) and bwahip_bgzf_write_lens under the sanitizers, without Python in between.
//   san_bai <input> <mode> <out.bai>
// input: n_ref, base, n_rec (int64 each), n_rec + 1 record offsets (int64), the record bytes, n_members (int64), the member lengths (int32).
// mode 0: all records, then all members; 1: all members first; 2: one record at a time, a member after every third; 3: the members'
// lengths come from bwahip_bgzf_write_lens over the records at level 1 (dropped output) instead of the input's.
// Exit status: 0 and the index in <out.bai>, or 10 - (the library's error code) when the builder refuses.
#include "../include/bwahip.h"
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include <vector>

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
	if (argc != 4) { fprintf(stderr, "usage: san_bai input mode out.bai\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	const int mode = atoi(argv[2]);
	int64_t n_ref = 0, base = 0, n_rec = 0, n_mem = 0;
	if (!rd(f, &n_ref, 8) || !rd(f, &base, 8) || !rd(f, &n_rec, 8)) return 2;
	std::vector<int64_t> off((size_t)n_rec + 1);
	if (!rd(f, off.data(), off.size() * 8)) return 2;
	std::vector<uint8_t> rec((size_t)off[(size_t)n_rec]);
	if (!rd(f, rec.data(), rec.size()) || !rd(f, &n_mem, 8)) return 2;
	std::vector<int32_t> lens((size_t)n_mem);
	if (!rd(f, lens.data(), lens.size() * 4)) return 2;
	fclose(f);
	if (mode == 3) {
		int64_t got = 0;
		int rc = bwahip_bgzf_write_lens(-1, rec.data(), (int64_t)rec.size(), 1, 3, lens.data(), n_mem ? n_mem - 1 : 0, &got);
		if (n_mem && rc != BWAHIP_ECAPACITY) { fprintf(stderr, "a table one too short was not refused: %d\n", rc); return 3; }
		rc = bwahip_bgzf_write_lens(-1, rec.data(), (int64_t)rec.size(), 1, 3, lens.data(), n_mem, &got);
		if (rc || got != n_mem) { fprintf(stderr, "bwahip_bgzf_write_lens: %d, %lld members\n", rc, (long long)got); return 3; }
	}
	bwahip_bai_builder *b = nullptr;
	int rc = bwahip_bai_builder_open((int32_t)n_ref, base, &b);
	if (!rc && mode == 1) rc = bwahip_bai_builder_add_members(b, lens.data(), n_mem);
	if (!rc && mode == 2) {
		int64_t fed = 0;
		for (int64_t i = 0; i < n_rec && !rc; ++i) {
			// a copy of its own for every record: a read past the record's end is a read past an allocation
			std::vector<uint8_t> one(rec.begin() + off[(size_t)i], rec.begin() + off[(size_t)i + 1]);
			const int64_t o2[2] = { 0, (int64_t)one.size() };
			rc = bwahip_bai_builder_add_records(b, one.data(), o2, 1);
			if (!rc && i % 3 == 2 && fed < n_mem) rc = bwahip_bai_builder_add_members(b, lens.data() + fed++, 1);
		}
		if (!rc) rc = bwahip_bai_builder_add_members(b, lens.data() + fed, n_mem - fed);
	} else if (!rc) rc = bwahip_bai_builder_add_records(b, rec.data(), off.data(), n_rec);
	if (!rc && (mode == 0 || mode == 3)) rc = bwahip_bai_builder_add_members(b, lens.data(), n_mem);
	if (!rc) {
		const int fd = open(argv[3], O_WRONLY | O_CREAT | O_TRUNC, 0644);
		if (fd < 0) return 2;
		rc = bwahip_bai_builder_finish(b, fd);
		close(fd);
	}
	bwahip_bai_builder_close(b);
	return rc ? 10 - rc : 0;
}
