// What the files beside a coordinate-sorted BAM file -- the BAI index, the QC summary, the pileup, the recalibration table -- share on the
// host: little-endian words into a byte vector, all bytes to a descriptor, the check of a table of contig lengths, and the skeleton of a
// device-free builder (bai_host.cpp, qc_host.cpp, pileup_host.cpp, recal_host.cpp): what it keeps of the contigs, how it is fed, how an
// error stays, how it ends.  Plain C++17 and inline: every file that includes it compiles alone.
#pragma once
#include "../../include/bwahip.h"
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <vector>

// a word at a time into reserved room: byte-wise push_back took 3.5 or 4.4 ms for a 4.5 MB index, depending on where the linker put the loop
inline void put32(std::vector<uint8_t> &o, uint32_t v) { uint8_t b[4]; for (int k = 0; k < 4; ++k) b[k] = (uint8_t)(v >> (8 * k)); o.insert(o.end(), b, b + 4); }
inline void put64(std::vector<uint8_t> &o, uint64_t v) { uint8_t b[8]; for (int k = 0; k < 8; ++k) b[k] = (uint8_t)(v >> (8 * k)); o.insert(o.end(), b, b + 8); }

// All `len` bytes at p to fd, or BWAHIP_EIO: a short write goes on, EINTR tries again, at most 1 GiB per call of write.  fd < 0: nothing is
// written.  what: "[bwahip] <what> failed: <strerror>" on stderr (null: the caller says it)
inline int write_all(int fd, const void *p, int64_t len, const char *what)
{
	const uint8_t *b = (const uint8_t*)p;
	while (fd >= 0 && len > 0) {
		const ssize_t w = write(fd, b, (size_t)(len > (1ll << 30) ? (1ll << 30) : len));
		if (w < 0) { if (errno == EINTR) continue; if (what) fprintf(stderr, "[bwahip] %s failed: %s\n", what, strerror(errno)); return BWAHIP_EIO; }
		if (w == 0) return BWAHIP_EIO;
		b += w; len -= w;
	}
	return 0;
}

// A table of contig lengths: BWAHIP_EINVAL for n_ref < 0, a missing table, a length outside [0, 2^31 - 1]; then BWAHIP_ECAPACITY for a sum
// of max_sum or more.  *sum_len (may be null): the sum
constexpr int64_t NO_SUM_CAP = INT64_MAX;
inline int check_refs(int32_t n_ref, const int64_t *ref_len, int64_t *sum_len, int64_t max_sum)
{
	if (n_ref < 0 || (n_ref && !ref_len)) return BWAHIP_EINVAL;
	int64_t s = 0;
	for (int32_t r = 0; r < n_ref; ++r) { if (ref_len[r] < 0 || ref_len[r] > 0x7fffffffll) return BWAHIP_EINVAL; s += ref_len[r]; }
	if (s >= max_sum) return BWAHIP_ECAPACITY;
	if (sum_len) *sum_len = s;
	return 0;
}

// What every builder keeps: the latch -- after a refusal every later call returns the same code -- and, where it is asked for, the contigs'
// lengths, their first bases among all contigs (n_ref + 1) and a copy of the packed reference
struct SidecarBuilder {
	int32_t n_ref = 0; int err = 0; bool finished = false;
	std::vector<int64_t> ref_len, ref_off;
	std::vector<uint8_t> pac;
	void set_refs(int32_t n, const int64_t *len, const uint8_t *pac_)   // checked lengths; pac_: null, or (their sum + 3) / 4 bytes
	{
		n_ref = n;
		ref_len.assign(len, len + n);
		ref_off.assign((size_t)n + 1, 0);
		for (int32_t r = 0; r < n; ++r) ref_off[(size_t)r + 1] = ref_off[(size_t)r] + len[r];
		if (pac_) pac.assign(pac_, pac_ + (ref_off[(size_t)n] + 3) / 4);
	}
};

// n_rec records, record i = rec[rec_off[i] .. rec_off[i + 1]), each through one(b, record, length): the first non-zero code ends the call and
// stays, the records before it are counted
template <class B, class One> inline int builder_feed(B *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, One one)
{
	if (!b || n_rec < 0 || (n_rec && (!rec || !rec_off)) || b->finished) return BWAHIP_EINVAL;
	if (b->err) return b->err;
	for (int64_t i = 0; i < n_rec; ++i) {
		if (rec_off[i] < 0 || rec_off[i + 1] < rec_off[i]) return b->err = BWAHIP_EINVAL;
		const int rc = one(b, rec + rec_off[i], rec_off[i + 1] - rec_off[i]);
		if (rc) return b->err = rc;
	}
	return 0;
}

// The one finish of a builder: make(b, &bytes) turns what was fed into the file's bytes, they go to fd (write_all), the result stays
template <class B, class Make> inline int builder_finish(B *b, int fd, const char *what, Make make)
{
	if (!b || b->finished) return BWAHIP_EINVAL;
	if (b->err) return b->err;
	b->finished = true;
	std::vector<uint8_t> bytes;
	int rc = make(b, &bytes);
	if (!rc) rc = write_all(fd, bytes.data(), (int64_t)bytes.size(), what);
	return b->err = rc;
}
