// Driver of the sanitizer build of the sorted-BAM merger (tests/test_bam_sorted_cpu.py): csrc/bam_sort_host.cpp + csrc/bam_host.cpp as plain
// host C++.  Reads runs from a file written by the test (n_runs; per run, in the order they are to be added: run_no, n_rec, len, keys,
// offsets, record bytes), adds them from three threads, merges them into BGZF blocks on the output file.
//   san_bam_sort <runs.bin> <tmp_dir> <mem_budget> <level> <out>
#include "../include/bwahip.h"
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include <thread>
#include <vector>

struct RunIn { int64_t run_no, n_rec, len; std::vector<uint64_t> keys; std::vector<int64_t> off; std::vector<uint8_t> rec; };

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "san_bam_sort: %s failed (line %d)\n", #cond, __LINE__); return 1; } } while (0)

int main(int argc, char **argv)
{
	if (argc != 6) { fprintf(stderr, "usage: san_bam_sort runs.bin tmp_dir mem_budget level out\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	CHECK(f);
	int64_t n_runs = 0;
	CHECK(fread(&n_runs, 8, 1, f) == 1 && n_runs >= 0 && n_runs < 100000);
	std::vector<RunIn> runs((size_t)n_runs);
	for (auto &r : runs) {
		int64_t h[3];
		CHECK(fread(h, 8, 3, f) == 3);
		r.run_no = h[0]; r.n_rec = h[1]; r.len = h[2];
		r.keys.resize((size_t)r.n_rec); r.off.resize((size_t)r.n_rec + 1); r.rec.resize((size_t)r.len);
		CHECK(fread(r.keys.data(), 8, (size_t)r.n_rec, f) == (size_t)r.n_rec);
		CHECK(fread(r.off.data(), 8, (size_t)r.n_rec + 1, f) == (size_t)r.n_rec + 1);
		CHECK(r.len == 0 || fread(r.rec.data(), 1, (size_t)r.len, f) == (size_t)r.len);
	}
	fclose(f);
	const int64_t budget = atoll(argv[3]);
	const int level = atoi(argv[4]);

	bwahip_bam_merger *m = nullptr;
	CHECK(bwahip_bam_merger_open((std::string(argv[2]) + "/missing").c_str(), budget, &m) == BWAHIP_EIO && m == nullptr);
	CHECK(bwahip_bam_merger_open(argv[2], budget, &m) == 0 && m);
	std::vector<int> rc(3, 0);
	std::vector<std::thread> th;
	for (int t = 0; t < 3; ++t) th.emplace_back([&, t] {
		for (size_t k = (size_t)t; k < runs.size(); k += 3) {
			const RunIn &r = runs[k];
			const int x = bwahip_bam_merger_add(m, r.run_no, r.rec.data(), r.len, r.keys.data(), r.off.data(), r.n_rec);
			if (x) rc[(size_t)t] = x;
		}
	});
	for (auto &t : th) t.join();
	CHECK(rc[0] == 0 && rc[1] == 0 && rc[2] == 0);
	if (!runs.empty()) CHECK(bwahip_bam_merger_add(m, runs[0].run_no, runs[0].rec.data(), runs[0].len, runs[0].keys.data(), runs[0].off.data(), runs[0].n_rec) == BWAHIP_EINVAL);
	int64_t n_records = 0, n_merged = 0, spilled = 0;
	const int fd = open(argv[5], O_WRONLY | O_CREAT | O_TRUNC, 0644);
	CHECK(fd >= 0);
	CHECK(bwahip_bam_merger_finish(m, fd, level, 3) == 0);
	CHECK(close(fd) == 0);
	CHECK(bwahip_bam_merger_stats(m, &n_records, &n_merged, &spilled, nullptr) == 0 && n_merged == n_runs);
	int64_t want = 0;
	for (auto &r : runs) want += r.n_rec;
	CHECK(n_records == want && (budget > 0 || spilled > 0 || want == 0));
	bwahip_bam_merger_close(m);
	// the header and the key need no merger
	bwahip_ann_t anns[2] = { { 0, 1000, 0, 0, 0, (char*)"a", (char*)"" }, { 1000, 50, 0, 0, 1, (char*)"b", (char*)"" } };
	bwahip_bns_t bns;
	memset(&bns, 0, sizeof bns);
	bns.n_seqs = 2; bns.anns = anns; bns.l_pac = 1050;
	uint8_t *h = nullptr; int64_t hl = 0;
	CHECK(bwahip_bam_header_sorted(&bns, "@PG\tID:x", &h, &hl) == 0 && hl > 40 && memcmp(h + 8, "@HD\tVN:1.6\tSO:coordinate\n", 25) == 0);
	free(h);
	CHECK(bwahip_bam_header_sorted(&bns, "@HD\tVN:1.0", &h, &hl) == BWAHIP_EINVAL);
	CHECK(bwahip_bam_sort_key(&bns, 1, 49, 1) < bwahip_bam_sort_key(&bns, -1, -1, 0) && bwahip_bam_sort_key_bits(&bns) == 1 + 10 + 2);
	return 0;
}
