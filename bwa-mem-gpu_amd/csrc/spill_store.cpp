// The store of spilled runs: see spill_store.h.  Device-free; built into libbwahip.so and, alone, into the sanitizer program of
// tests/test_bam_spill_cpu.py.
#include "spill_store.h"
#include "../../include/bwahip.h"
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <map>
#include <mutex>
#include <string>

namespace {
struct Run { int64_t len = 0; uint8_t *mem = nullptr; int fd = -1; };
void *std_alloc(size_t n, void *) { return malloc(n ? n : 1); }
void std_free(void *p, size_t, void *) { free(p); }
}

struct SpillStore {
	int64_t host_budget = 0, host_bytes = 0, file_bytes = 0;
	std::string tmp_dir; bool has_dir = false;
	spill_alloc_fn alloc = std_alloc; spill_free_fn free_ = std_free; void *user = nullptr;
	mutable std::mutex mu;
	std::map<int64_t, Run> runs;
	void release(Run &r)
	{
		if (r.mem) { free_(r.mem, (size_t)r.len, user); host_bytes -= r.len; }
		if (r.fd >= 0) { close(r.fd); file_bytes -= r.len; }
		r.mem = nullptr; r.fd = -1;
	}
};

SpillStore *spill_store_new(int64_t host_budget, const char *tmp_dir, spill_alloc_fn alloc, spill_free_fn free_, void *user)
{
	if (host_budget < 0 || !alloc != !free_) return nullptr;
	SpillStore *s = new SpillStore;
	s->host_budget = host_budget;
	if (tmp_dir) { s->tmp_dir = tmp_dir; s->has_dir = true; }
	if (alloc) { s->alloc = alloc; s->free_ = free_; s->user = user; }
	return s;
}

void spill_store_free(SpillStore *s)
{
	if (!s) return;
	for (auto &kv : s->runs) s->release(kv.second);
	delete s;
}

// an unlinked file in the directory: its name is gone before a byte is written, so nothing is left behind whatever happens
static int make_file(const SpillStore *s)
{
	if (!s->has_dir) { fprintf(stderr, "[bwahip] spilled runs: a run needs a file and no tmp_dir was given\n"); return -1; }
	struct stat sb;
	if (stat(s->tmp_dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) { fprintf(stderr, "[bwahip] spilled runs: %s is not a directory\n", s->tmp_dir.c_str()); return -1; }
	std::string path = s->tmp_dir + "/bwahip_spill_XXXXXX";
	const int fd = mkstemp(&path[0]);
	if (fd < 0) { fprintf(stderr, "[bwahip] spilled runs: no file can be made in %s: %s\n", s->tmp_dir.c_str(), strerror(errno)); return -1; }
	(void)unlink(path.c_str());
	return fd;
}

int spill_store_reserve(SpillStore *s, int64_t id, int64_t len, uint8_t **mem)
{
	if (!s || !mem || len < 0) return BWAHIP_EINVAL;
	*mem = nullptr;
	std::lock_guard<std::mutex> lk(s->mu);
	if (s->runs.count(id)) return BWAHIP_EINVAL;
	Run r;
	r.len = len;
	if (len && s->host_bytes + len <= s->host_budget) {
		r.mem = (uint8_t*)s->alloc((size_t)len, s->user);
		if (!r.mem) return BWAHIP_ENOMEM;
		s->host_bytes += len;
	} else if (len) {
		if ((r.fd = make_file(s)) < 0) return BWAHIP_EIO;
		s->file_bytes += len;
	}
	s->runs[id] = r;
	*mem = r.mem;
	return 0;
}

int spill_store_write(SpillStore *s, int64_t id, int64_t at, const uint8_t *bytes, int64_t len)
{
	if (!s || at < 0 || len < 0 || (len && !bytes)) return BWAHIP_EINVAL;
	int fd;
	{
		std::lock_guard<std::mutex> lk(s->mu);
		auto it = s->runs.find(id);
		if (it == s->runs.end() || at + len > it->second.len) return BWAHIP_EINVAL;
		if (!len) return 0;
		if (it->second.mem) { memcpy(it->second.mem + at, bytes, (size_t)len); return 0; }
		fd = it->second.fd;
	}
	while (len > 0) {
		const ssize_t w = pwrite(fd, bytes, (size_t)(len > (1ll << 30) ? (1ll << 30) : len), (off_t)at);
		if (w < 0) { if (errno == EINTR) continue; fprintf(stderr, "[bwahip] spilled runs: writing a run's file failed: %s\n", strerror(errno)); return BWAHIP_EIO; }
		if (w == 0) return BWAHIP_EIO;
		bytes += w; at += w; len -= w;
	}
	return 0;
}

int spill_store_put(SpillStore *s, int64_t id, const uint8_t *bytes, int64_t len)
{
	if (len > 0 && !bytes) return BWAHIP_EINVAL;
	uint8_t *mem = nullptr;
	int rc = spill_store_reserve(s, id, len, &mem);
	if (rc) return rc;
	if (mem) memcpy(mem, bytes, (size_t)len);
	else if (len && (rc = spill_store_write(s, id, 0, bytes, len))) (void)spill_store_drop(s, id);
	return rc;
}

const uint8_t *spill_store_mem(const SpillStore *s, int64_t id)
{
	if (!s) return nullptr;
	std::lock_guard<std::mutex> lk(s->mu);
	auto it = s->runs.find(id);
	return it == s->runs.end() ? nullptr : it->second.mem;
}

int spill_store_get(const SpillStore *s, int64_t id, int64_t at, int64_t len, uint8_t *dst)
{
	if (!s || at < 0 || len < 0 || (len && !dst)) return BWAHIP_EINVAL;
	int fd;
	{
		std::lock_guard<std::mutex> lk(s->mu);
		auto it = s->runs.find(id);
		if (it == s->runs.end() || at + len > it->second.len) return BWAHIP_EINVAL;
		if (!len) return 0;
		if (it->second.mem) { memcpy(dst, it->second.mem + at, (size_t)len); return 0; }
		fd = it->second.fd;
	}
	while (len > 0) {
		const ssize_t g = pread(fd, dst, (size_t)(len > (1ll << 30) ? (1ll << 30) : len), (off_t)at);
		if (g < 0) { if (errno == EINTR) continue; fprintf(stderr, "[bwahip] spilled runs: reading a run's file failed: %s\n", strerror(errno)); return BWAHIP_EIO; }
		if (g == 0) return BWAHIP_EIO;                                 // the file is shorter than what was written into it
		dst += g; at += g; len -= g;
	}
	return 0;
}

int64_t spill_store_len(const SpillStore *s, int64_t id)
{
	if (!s) return -1;
	std::lock_guard<std::mutex> lk(s->mu);
	auto it = s->runs.find(id);
	return it == s->runs.end() ? -1 : it->second.len;
}

int spill_store_drop(SpillStore *s, int64_t id)
{
	if (!s) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(s->mu);
	auto it = s->runs.find(id);
	if (it == s->runs.end()) return BWAHIP_EINVAL;
	s->release(it->second);
	s->runs.erase(it);
	return 0;
}

int64_t spill_store_host_bytes(const SpillStore *s) { if (!s) return 0; std::lock_guard<std::mutex> lk(s->mu); return s->host_bytes; }
int64_t spill_store_file_bytes(const SpillStore *s) { if (!s) return 0; std::lock_guard<std::mutex> lk(s->mu); return s->file_bytes; }
