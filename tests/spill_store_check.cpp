// A stand-alone caller of the store of spilled runs (bwa-mem-gpu_amd/csrc/spill_store.cpp): built by tests/test_bam_spill_cpu.py together
// with the store, with -fsanitize=address,undefined, and run as a child process.  argv[1]: a directory files can be made in; argv[2]: a
// path that is no directory.  Prints "ok" and returns 0, or says what went wrong.
#include "spill_store.h"
#include "bwahip.h"
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

static int n_alloc = 0, n_free = 0;
static size_t live_bytes = 0;
static void *count_alloc(size_t n, void *user) { ++n_alloc; live_bytes += n; return user == (void*)&n_alloc ? malloc(n ? n : 1) : nullptr; }
static void count_free(void *p, size_t n, void *) { ++n_free; live_bytes -= n; free(p); }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static std::vector<uint8_t> bytes_of(int64_t n, unsigned seed)
{
	std::vector<uint8_t> v((size_t)n);
	for (auto &b : v) { seed = seed * 1664525u + 1013904223u; b = (uint8_t)(seed >> 24); }
	return v;
}

static int entries(const char *dir)
{
	DIR *d = opendir(dir);
	if (!d) return -1;
	int n = 0;
	while (struct dirent *e = readdir(d)) if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) ++n;
	closedir(d);
	return n;
}

// every slice that matters: whole, empty at both ends, one byte at both ends, and some in between
static int slices_match(const SpillStore *s, int64_t id, const std::vector<uint8_t> &want)
{
	const int64_t n = (int64_t)want.size();
	CHECK(spill_store_len(s, id) == n);
	std::vector<uint8_t> got((size_t)n + 1, 0xa5);
	const int64_t cuts[][2] = { { 0, n }, { 0, 0 }, { n, 0 }, { 0, n ? 1 : 0 }, { n ? n - 1 : 0, n ? 1 : 0 }, { n / 3, n / 2 }, { n / 2, n - n / 2 }, { 1 % (n + 1), n > 2 ? n - 2 : 0 } };
	for (auto &c : cuts) {
		std::fill(got.begin(), got.end(), (uint8_t)0xa5);
		CHECK(spill_store_get(s, id, c[0], c[1], got.data()) == 0);
		CHECK(!c[1] || !memcmp(got.data(), want.data() + c[0], (size_t)c[1]));
		CHECK(got[(size_t)c[1]] == 0xa5);                              // nothing behind the slice was written
	}
	CHECK(spill_store_get(s, id, 0, n + 1, got.data()) == BWAHIP_EINVAL);   // beyond the run
	CHECK(spill_store_get(s, id, n, 1, got.data()) == BWAHIP_EINVAL);
	CHECK(spill_store_get(s, id, -1, 1, got.data()) == BWAHIP_EINVAL);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	const char *dir = argv[1], *no_dir = argv[2];
	const int64_t lens[] = { 100000, 0, 70001, 1, 300000 };
	std::vector<std::vector<uint8_t>> runs;
	for (int k = 0; k < 5; ++k) runs.push_back(bytes_of(lens[k], 7u + k));
	CHECK(!spill_store_new(-1, dir, nullptr, nullptr, nullptr));
	// ---- memory, files, some of each: budgets everything fits, nothing fits, and one that holds runs 0 and 3 alone
	const int64_t budgets[] = { 1 << 30, 0, 100001 };
	for (int64_t budget : budgets) {
		n_alloc = n_free = 0;
		SpillStore *s = spill_store_new(budget, dir, count_alloc, count_free, &n_alloc);
		CHECK(s);
		int64_t in_mem = 0, in_file = 0;
		for (int k = 0; k < 5; ++k) {
			CHECK(spill_store_put(s, 10 + k, runs[k].data(), lens[k]) == 0);
			const bool mem = lens[k] && in_mem + lens[k] <= budget;
			(mem ? in_mem : in_file) += lens[k];
			CHECK((spill_store_mem(s, 10 + k) != nullptr) == mem);
			CHECK(spill_store_host_bytes(s) == in_mem && spill_store_file_bytes(s) == in_file);
		}
		CHECK(budget != 100001 || (in_mem == 100001 && in_file == 370001));
		CHECK(entries(dir) == 0);                                      // the files have no name
		CHECK(spill_store_put(s, 12, runs[0].data(), lens[0]) == BWAHIP_EINVAL);   // held already
		CHECK(spill_store_host_bytes(s) == in_mem && spill_store_file_bytes(s) == in_file);
		for (int k = 0; k < 5; ++k) if (slices_match(s, 10 + k, runs[k])) return 1;
		CHECK(spill_store_len(s, 99) == -1 && spill_store_drop(s, 99) == BWAHIP_EINVAL);
		CHECK(spill_store_drop(s, 10) == 0 && spill_store_len(s, 10) == -1);
		CHECK(spill_store_host_bytes(s) + spill_store_file_bytes(s) == in_mem + in_file - lens[0]);
		if (slices_match(s, 14, runs[4])) return 1;
		// reserve, then filled by the caller in pieces and out of order
		uint8_t *mem = nullptr;
		CHECK(spill_store_reserve(s, 10, lens[0], &mem) == 0);
		if (mem) memcpy(mem, runs[0].data(), (size_t)lens[0]);
		else {
			CHECK(spill_store_write(s, 10, 60000, runs[0].data() + 60000, 40000) == 0);
			CHECK(spill_store_write(s, 10, 0, runs[0].data(), 60000) == 0);
			CHECK(spill_store_write(s, 10, 99999, runs[0].data(), 2) == BWAHIP_EINVAL);
		}
		if (slices_match(s, 10, runs[0])) return 1;
		spill_store_free(s);
		CHECK(n_alloc == n_free && live_bytes == 0);
		CHECK(entries(dir) == 0);
	}
	// ---- a directory that cannot be used: refused, and the earlier runs are still there
	const char *bad_dirs[] = { nullptr, no_dir, "/nonexistent/bwahip/spill" };
	for (const char *bad : bad_dirs) {
		SpillStore *s = spill_store_new(150000, bad, nullptr, nullptr, nullptr);   // malloc and free
		CHECK(s);
		CHECK(spill_store_put(s, 0, runs[0].data(), lens[0]) == 0);   // memory
		CHECK(spill_store_put(s, 1, runs[1].data(), 0) == 0);          // no bytes: no file
		CHECK(spill_store_put(s, 2, runs[2].data(), lens[2]) == BWAHIP_EIO);
		CHECK(spill_store_len(s, 2) == -1 && spill_store_host_bytes(s) == lens[0] && spill_store_file_bytes(s) == 0);
		CHECK(spill_store_put(s, 3, runs[3].data(), lens[3]) == 0);   // one byte still fits
		if (slices_match(s, 0, runs[0]) || slices_match(s, 1, runs[1]) || slices_match(s, 3, runs[3])) return 1;
		spill_store_free(s);
	}
	// ---- an allocator that refuses
	{
		SpillStore *s = spill_store_new(1 << 30, dir, count_alloc, count_free, nullptr);
		CHECK(s && spill_store_put(s, 0, runs[0].data(), lens[0]) == BWAHIP_ENOMEM && spill_store_len(s, 0) == -1 && spill_store_host_bytes(s) == 0);
		live_bytes = 0;
		spill_store_free(s);
	}
	puts("ok");
	return 0;
}
