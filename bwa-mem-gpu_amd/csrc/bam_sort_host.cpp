// Host side of the coordinate-sorted BAM output: what needs no device.  The host restatement of the sort key (bam_sort_key.h), the
// header that announces the order, and the merger of sorted runs -- one run per batch, each already sorted on the GPU (k_bamsort.hip)
// and handed over with its keys and record offsets, so that nothing here ever parses a record.
#include "../../include/bwahip.h"
#include "bam_sort_key.h"
#include "bai_tables.h"                                         // MergeHooks: the index builder listens to the merge (bai_host.cpp)
#include "sidecar_host.h"
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

extern "C" uint64_t bwahip_bam_sort_key(const bwahip_bns_t *bns, int32_t refID, int32_t pos, int reverse)
{
	if (!bns || bns->n_seqs < 0 || (bns->n_seqs && !bns->anns)) return ~0ull;
	return bam_key_pack(bns->n_seqs, bam_key_pos_bits(bns), refID, pos, reverse);
}

extern "C" int bwahip_bam_sort_key_bits(const bwahip_bns_t *bns)
{
	if (!bns || bns->n_seqs < 0 || (bns->n_seqs && !bns->anns)) return BWAHIP_EINVAL;
	return bam_key_bits(bns);
}

// the same two from the numbers of an index alone (its contig count and longest contig): what bwahip_bam_sort_key / _key_bits compute once
// they have walked the contig table
extern "C" uint64_t bwahip_bam_sort_key_for(int32_t n_seqs, int32_t longest, int32_t refID, int32_t pos, int reverse)
{
	if (n_seqs < 0 || longest < 0) return ~0ull;
	return bam_key_pack(n_seqs, bam_key_pos_bits_of(longest), refID, pos, reverse);
}

extern "C" int bwahip_bam_sort_key_bits_for(int32_t n_seqs, int32_t longest)
{
	if (n_seqs < 0 || longest < 0) return BWAHIP_EINVAL;
	return bam_key_bits_of(n_seqs, longest);
}

// bwahip_bam_header with "@HD\tVN:1.6\tSO:coordinate" as the first line of the text
extern "C" int bwahip_bam_header_sorted(const bwahip_bns_t *bns, const char *hdr_line, uint8_t **out, int64_t *len)
{
	if (!out || !len) return BWAHIP_EINVAL;
	if (hdr_line) for (const char *p = hdr_line; (p = strstr(p, "@HD")) != nullptr; p += 3)
		if ((p == hdr_line || p[-1] == '\n') && (p[3] == '\t' || p[3] == '\n' || p[3] == 0)) return BWAHIP_EINVAL;   // the order is ours to state
	uint8_t *h = nullptr; int64_t hl = 0;
	const int rc = bwahip_bam_header(bns, hdr_line, &h, &hl);
	if (rc) return rc;
	static const char hd[] = "@HD\tVN:1.6\tSO:coordinate\n";
	const int64_t add = (int64_t)sizeof hd - 1;
	uint32_t l_text;
	memcpy(&l_text, h + 4, 4);
	uint8_t *b = (uint8_t*)malloc((size_t)(hl + add));
	if (!b) { free(h); return BWAHIP_ENOMEM; }
	memcpy(b, h, 4);
	l_text += (uint32_t)add;
	memcpy(b + 4, &l_text, 4);
	memcpy(b + 8, hd, (size_t)add);
	memcpy(b + 8 + add, h + 8, (size_t)(hl - 8));
	free(h);
	*out = b; *len = hl + add;
	return 0;
}

// ---- merger -------------------------------------------------------------------------------------------------------------------------
// A run = the sorted records of one batch, its keys and its record offsets.  Runs are kept in host memory while their total stays within
// the budget; from the first run that would exceed it, every further run goes to a file of its own under tmp_dir:
//     n_rec keys (u64) | n_rec + 1 offsets (i64) | the record bytes            (private, uncompressed, removed on close)
// finish() is a k-way merge by (key, run_no): the runs are sorted and stable in themselves and run numbers are unique, so the position in
// the run needs no comparison.  Spilled runs are read through bounded windows (keys / offsets: WIN_ITEMS at a time, records: WIN_BYTES),
// the output goes to the BGZF writer in pieces that are whole multiples of a block's input, so the file is the one a single
// bwahip_bgzf_write of all records would give -- whatever the budget and the number of runs.
namespace {

constexpr int64_t WIN_ITEMS = 8192, WIN_BYTES = 1 << 20;
constexpr int64_t PIECE = 512 * 65280;       // bytes handed to the BGZF writer at a time

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Run {
	int64_t n_rec = 0, len = 0;
	std::vector<uint8_t> rec; std::vector<uint64_t> keys; std::vector<int64_t> off;   // in memory
	std::string path;                                                                // spilled
};

int pread_full(int fd, void *p, int64_t len, int64_t at)
{
	uint8_t *b = (uint8_t*)p;
	while (len > 0) {
		const ssize_t r = pread(fd, b, (size_t)len, (off_t)at);
		if (r < 0) { if (errno == EINTR) continue; return BWAHIP_EIO; }
		if (r == 0) return BWAHIP_EIO;                           // shorter than what was written
		b += r; len -= r; at += r;
	}
	return 0;
}

// the merge's view of one run: current key, and the bytes of the current record
struct Cursor {
	const Run *run = nullptr; int64_t run_no = 0, i = 0;
	std::vector<uint64_t> wkeys; std::vector<int64_t> woff; std::vector<uint8_t> wrec;
	int64_t win0 = 0, win_n = 0;             // keys / offsets window: records [win0, win0 + win_n)
	int64_t rec0 = 0, rec1 = 0;              // record bytes window: bytes [rec0, rec1) of the run
	uint64_t key = 0;

	// a spilled run's file is open only while a window is filled: the merge holds no descriptor per run, so the number of runs is not
	// bounded by the process's limit on open files
	int read_at(void *p, int64_t len, int64_t at) const
	{
		const int fd = open(run->path.c_str(), O_RDONLY);
		if (fd < 0) return BWAHIP_EIO;
		const int rc = pread_full(fd, p, len, at);
		close(fd);
		return rc;
	}
	int load_window()
	{
		win0 = i; win_n = run->n_rec - i < WIN_ITEMS ? run->n_rec - i : WIN_ITEMS;
		wkeys.resize((size_t)win_n); woff.resize((size_t)win_n + 1);
		int rc;
		if ((rc = read_at(wkeys.data(), win_n * 8, win0 * 8)) || (rc = read_at(woff.data(), (win_n + 1) * 8, run->n_rec * 8 + win0 * 8))) return rc;
		for (int64_t k = 0; k < win_n; ++k) if (woff[(size_t)k] < 0 || woff[(size_t)k] > woff[(size_t)k + 1] || woff[(size_t)k + 1] > run->len) return BWAHIP_EIO;
		return 0;
	}
	int open_run()
	{
		if (run->path.empty()) { key = run->keys[0]; return 0; }
		const int rc = load_window();
		if (!rc) key = wkeys[0];
		return rc;
	}
	// the current record; valid until the next call
	int record(const uint8_t **p, int64_t *n)
	{
		if (run->path.empty()) { *p = run->rec.data() + run->off[(size_t)i]; *n = run->off[(size_t)i + 1] - run->off[(size_t)i]; return 0; }
		const int64_t b = woff[(size_t)(i - win0)], e = woff[(size_t)(i - win0) + 1];
		if (b < rec0 || e > rec1) {
			int64_t want = e - b > WIN_BYTES ? e - b : WIN_BYTES;
			if (b + want > run->len) want = run->len - b;
			wrec.resize((size_t)want);
			const int rc = read_at(wrec.data(), want, (2 * run->n_rec + 1) * 8 + b);
			if (rc) return rc;
			rec0 = b; rec1 = b + want;
		}
		*p = wrec.data() + (b - rec0); *n = e - b;
		return 0;
	}
	// to the next record; *more = false at the end of the run
	int advance(bool *more)
	{
		if (++i >= run->n_rec) { *more = false; return 0; }
		*more = true;
		if (run->path.empty()) { key = run->keys[(size_t)i]; return 0; }
		if (i >= win0 + win_n) { const int rc = load_window(); if (rc) return rc; }
		key = wkeys[(size_t)(i - win0)];
		return 0;
	}
};

std::atomic<long> g_merger_serial{0};

} // namespace

struct bwahip_bam_merger {
	std::string dir;
	int64_t budget = 0, mem_bytes = 0, spilled_bytes = 0, n_records = 0;
	bool spilling = false;
	long serial = 0;
	std::mutex mu;
	std::map<int64_t, Run> runs;             // by run_no: the tie-break of the merge
	double merge_s = 0;
	int (*listen)(void *arg, const uint8_t *rec, int64_t len) = nullptr; void *listen_arg = nullptr;   // bam_merger_listen: told every record as it is emitted
};

extern "C" int bwahip_bam_merger_open(const char *tmp_dir, int64_t mem_budget, bwahip_bam_merger **out)
{
	if (!out) return BWAHIP_EINVAL;
	*out = nullptr;
	const char *dir = tmp_dir && tmp_dir[0] ? tmp_dir : getenv("TMPDIR");
	if (!dir || !dir[0]) dir = "/tmp";
	struct stat sb;
	if (stat(dir, &sb) != 0 || !S_ISDIR(sb.st_mode) || access(dir, W_OK | X_OK) != 0) {
		fprintf(stderr, "[bwahip] sorted BAM: %s is not a directory files can be made in\n", dir);
		return BWAHIP_EIO;
	}
	bwahip_bam_merger *m = new bwahip_bam_merger;
	m->dir = dir; m->budget = mem_budget; m->spilling = mem_budget <= 0;
	m->serial = ++g_merger_serial;
	*out = m;
	return 0;
}

extern "C" int bwahip_bam_merger_add(bwahip_bam_merger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys, const int64_t *rec_off, int64_t n_rec)
{
	if (!m || run_no < 0 || len < 0 || n_rec < 0 || (n_rec && (!rec || !keys || !rec_off)) || (!n_rec && len)) return BWAHIP_EINVAL;
	if (n_rec && (rec_off[0] != 0 || rec_off[n_rec] != len)) return BWAHIP_EINVAL;
	const int64_t bytes = len + n_rec * 8 + (n_rec + 1) * 8;
	bool spill;
	Run *r;
	{
		std::lock_guard<std::mutex> lk(m->mu);
		if (m->runs.count(run_no)) return BWAHIP_EINVAL;
		if (!m->spilling && m->mem_bytes + bytes > m->budget) m->spilling = true;   // this run and every later one
		spill = m->spilling && n_rec > 0;
		if (!spill) m->mem_bytes += bytes;
		r = &m->runs[run_no];                                    // (std::map: the address stays put while other runs arrive)
		r->n_rec = n_rec; r->len = len;
		m->n_records += n_rec;
		if (spill) r->path = m->dir + "/bwahip_sort_" + std::to_string((long)getpid()) + "_" + std::to_string(m->serial) + "_" + std::to_string((long long)run_no) + ".run";
	}
	if (!n_rec) return 0;
	if (!spill) {
		r->rec.assign(rec, rec + len); r->keys.assign(keys, keys + n_rec); r->off.assign(rec_off, rec_off + n_rec + 1);
		return 0;
	}
	const int fd = open(r->path.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0600);
	int rc = fd < 0 ? BWAHIP_EIO : 0;
	if (!rc && ((rc = write_all(fd, keys, n_rec * 8, nullptr)) || (rc = write_all(fd, rec_off, (n_rec + 1) * 8, nullptr)) || (rc = write_all(fd, rec, len, nullptr)))) {}
	if (fd >= 0 && close(fd) != 0 && !rc) rc = BWAHIP_EIO;
	if (rc) {
		fprintf(stderr, "[bwahip] sorted BAM: writing %s failed: %s\n", r->path.c_str(), strerror(errno));
		if (fd >= 0) unlink(r->path.c_str());
		std::lock_guard<std::mutex> lk(m->mu);
		m->n_records -= n_rec;
		m->runs.erase(run_no);
		return rc;
	}
	std::lock_guard<std::mutex> lk(m->mu);
	m->spilled_bytes += bytes;
	return 0;
}

// bai (may be NULL): who is told every record as it is emitted and the lengths of a piece's members as the piece leaves the writer
int bam_merger_finish_hooks(bwahip_bam_merger *m, int fd, int level, int n_threads, const MergeHooks *bai)
{
	if (!m || level < 0 || level > 9) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	const double t0 = now_s();
	std::vector<Cursor> cur(m->runs.size());
	std::vector<Cursor*> heap;                                   // binary min-heap by (key, run_no)
	auto less = [](const Cursor *a, const Cursor *b) { return a->key != b->key ? a->key < b->key : a->run_no < b->run_no; };
	auto sift_down = [&](size_t k) {
		for (;;) {
			size_t c = 2 * k + 1;
			if (c >= heap.size()) break;
			if (c + 1 < heap.size() && less(heap[c + 1], heap[c])) ++c;
			if (!less(heap[c], heap[k])) break;
			std::swap(heap[c], heap[k]); k = c;
		}
	};
	int rc = 0;
	size_t n_cur = 0;
	for (auto &kv : m->runs) {
		if (!kv.second.n_rec) continue;
		Cursor &c = cur[n_cur++];
		c.run = &kv.second; c.run_no = kv.first;
		if ((rc = c.open_run())) return rc;
		heap.push_back(&c);
	}
	for (size_t k = heap.size() / 2; k-- > 0;) sift_down(k);
	std::vector<uint8_t> piece;
	if (!heap.empty()) piece.resize((size_t)PIECE);
	int64_t fill = 0;
	std::vector<int32_t> lens(bai ? (size_t)(PIECE / 65280) : 0);
	auto flush = [&]() -> int {
		if (!bai) return bwahip_bgzf_write(fd, piece.data(), fill, level, n_threads);
		int64_t n_mem = 0;
		const int r = bwahip_bgzf_write_lens(fd, piece.data(), fill, level, n_threads, lens.data(), (int64_t)lens.size(), &n_mem);
		return r ? r : bai->members(bai->arg, lens.data(), n_mem);
	};
	while (!heap.empty()) {
		Cursor *c = heap[0];
		const uint8_t *p; int64_t n;
		if ((rc = c->record(&p, &n))) return rc;
		if (bai && (rc = bai->record(bai->arg, p, n))) return rc;
		if (m->listen && (rc = m->listen(m->listen_arg, p, n))) return rc;
		while (n > 0) {                                           // a record may straddle two pieces: the BGZF stream is one sequence of bytes
			const int64_t take = n < PIECE - fill ? n : PIECE - fill;
			memcpy(piece.data() + fill, p, (size_t)take);
			fill += take; p += take; n -= take;
			if (fill == PIECE) { if ((rc = flush())) return rc; fill = 0; }
		}
		bool more;
		if ((rc = c->advance(&more))) return rc;
		if (!more) { heap[0] = heap.back(); heap.pop_back(); }
		if (!heap.empty()) sift_down(0);
	}
	if (fill && (rc = flush())) return rc;
	m->merge_s = now_s() - t0;
	return 0;
}

extern "C" int bwahip_bam_merger_finish(bwahip_bam_merger *m, int fd, int level, int n_threads) { return bam_merger_finish_hooks(m, fd, level, n_threads, nullptr); }

int bam_merger_listen(bwahip_bam_merger *m, int (*record)(void *arg, const uint8_t *rec, int64_t len), void *arg)
{
	if (!m) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	m->listen = record; m->listen_arg = arg;
	return 0;
}

extern "C" int bwahip_bam_merger_stats(bwahip_bam_merger *m, int64_t *n_records, int64_t *n_runs, int64_t *spilled_bytes, double *merge_s)
{
	if (!m) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	if (n_records) *n_records = m->n_records;
	if (n_runs) *n_runs = (int64_t)m->runs.size();
	if (spilled_bytes) *spilled_bytes = m->spilled_bytes;
	if (merge_s) *merge_s = m->merge_s;
	return 0;
}

extern "C" void bwahip_bam_merger_close(bwahip_bam_merger *m)
{
	if (!m) return;
	for (auto &kv : m->runs) if (!kv.second.path.empty()) unlink(kv.second.path.c_str());
	delete m;
}
