// Host side of the BAM output: what needs no device.  The BAM header of an index (SAM specification 4.2), the BGZF container (4.1:
// gzip members with the BC extra subfield) written from several deflate workers in order, and the batch-entry check of what a
// record cannot hold (k_bam.hip encodes only what passed here).
#include "../../include/bwahip.h"
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>
#include <string>
#include <thread>
#include <vector>

// ---- what a BAM record cannot hold --------------------------------------------------------------------------------------------
// l_read_name is one byte and counts the NUL: names of 255 bytes or more.  The -C comment is appended verbatim to the SAM text; in
// BAM each tab-separated field has to be a tag: XX:Z:<printable>, XX:A:<char> or XX:i:<integer in [-2^31, 2^32)>.
static bool comment_is_tags(const char *c)
{
	for (;;) {
		const char *e = c;
		while (*e && *e != '\t') ++e;
		const size_t len = (size_t)(e - c);
		if (len < 5 || c[2] != ':' || c[4] != ':') return false;
		const bool a0 = (c[0] >= 'A' && c[0] <= 'Z') || (c[0] >= 'a' && c[0] <= 'z');
		const bool a1 = (c[1] >= 'A' && c[1] <= 'Z') || (c[1] >= 'a' && c[1] <= 'z') || (c[1] >= '0' && c[1] <= '9');
		if (!a0 || !a1) return false;
		const char *v = c + 5;
		if (c[3] == 'Z') { for (const char *q = v; q < e; ++q) if (*q < ' ' || *q > '~') return false; }
		else if (c[3] == 'A') { if (e - v != 1 || *v < '!' || *v > '~') return false; }
		else if (c[3] == 'i') {
			const char *q = v;
			const bool neg = *q == '-';
			if (*q == '-' || *q == '+') ++q;
			if (q == e || e - q > 10) return false;
			long long x = 0;
			for (; q < e; ++q) { if (*q < '0' || *q > '9') return false; x = x * 10 + (*q - '0'); }
			if (neg ? x > 2147483648ll : x > 4294967295ll) return false;
		} else return false;
		if (!*e) return true;
		c = e + 1;
	}
}

int bam_check_reads(int n, const bwahip_seq_t *seqs)
{
	for (int i = 0; i < n; ++i) {
		if (!seqs[i].name) return BWAHIP_EINVAL;
		const size_t ln = strlen(seqs[i].name);
		if (ln >= 255) { fprintf(stderr, "[bwahip] BAM: the name of read %d has %zu bytes (at most 254 fit a record): %.40s...\n", i, ln, seqs[i].name); return BWAHIP_EINVAL; }
		if (seqs[i].comment && seqs[i].comment[0] && !comment_is_tags(seqs[i].comment)) {
			fprintf(stderr, "[bwahip] BAM: the comment of read %d (%s) is not a list of XX:Z: / XX:A: / XX:i: tags: %.60s\n", i, seqs[i].name, seqs[i].comment);
			return BWAHIP_EINVAL;
		}
	}
	return 0;
}

// ---- header ---------------------------------------------------------------------------------------------------------------------
static void put32(std::string &s, uint32_t v) { for (int k = 0; k < 4; ++k) s.push_back((char)(v >> (8 * k))); }

// magic, l_text + text, n_ref, names and lengths.  The text is what bwa_print_sam_hdr (bwa.c:520) writes for this bns and hdr_line:
// its own @SQ lines (AH:* for ALT contigs) unless hdr_line brings @SQ lines, then hdr_line and a newline.  A @PG line is the caller's.
extern "C" int bwahip_bam_header(const bwahip_bns_t *bns, const char *hdr_line, uint8_t **out, int64_t *len)
{
	if (!bns || !out || !len || bns->n_seqs < 0 || (bns->n_seqs && !bns->anns)) return BWAHIP_EINVAL;
	int n_sq = 0;
	if (hdr_line) for (const char *p = hdr_line; (p = strstr(p, "@SQ\t")) != nullptr; p += 4) if (p == hdr_line || p[-1] == '\n') ++n_sq;
	std::string text;
	if (n_sq == 0)
		for (int i = 0; i < bns->n_seqs; ++i) {
			if (!bns->anns[i].name) return BWAHIP_EINVAL;
			text += "@SQ\tSN:"; text += bns->anns[i].name; text += "\tLN:"; text += std::to_string(bns->anns[i].len);
			text += bns->anns[i].is_alt ? "\tAH:*\n" : "\n";
		}
	if (hdr_line) { text += hdr_line; text += '\n'; }
	std::string b("BAM\1", 4);
	put32(b, (uint32_t)text.size());
	b += text;
	put32(b, (uint32_t)bns->n_seqs);
	for (int i = 0; i < bns->n_seqs; ++i) {
		const char *nm = bns->anns[i].name;
		if (!nm) return BWAHIP_EINVAL;
		put32(b, (uint32_t)strlen(nm) + 1);
		b.append(nm, strlen(nm) + 1);
		put32(b, (uint32_t)bns->anns[i].len);
	}
	uint8_t *buf = (uint8_t*)malloc(b.size() ? b.size() : 1);
	if (!buf) return BWAHIP_ENOMEM;
	memcpy(buf, b.data(), b.size());
	*out = buf; *len = (int64_t)b.size();
	return 0;
}

// ---- BGZF -----------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t BGZF_IN = 65280;          // input bytes per block (what htslib uses: a stored block then still fits 64 KiB)
constexpr int64_t BGZF_SLOT = 65536;        // a block is at most 64 KiB
constexpr int BGZF_HEAD = 18, BGZF_TAIL = 8;

// one block: header | deflate stream | CRC32, ISIZE; returns its length
int64_t bgzf_block(z_stream *zs, const uint8_t *in, int n, int level, uint8_t *out)
{
	static const uint8_t head[16] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0 };
	memcpy(out, head, 16);
	uint8_t *d = out + BGZF_HEAD;
	int64_t dl = -1;
	if (level > 0) {
		deflateReset(zs);
		zs->next_in = (Bytef*)in; zs->avail_in = (uInt)n;
		zs->next_out = d; zs->avail_out = (uInt)(BGZF_SLOT - BGZF_HEAD - BGZF_TAIL);
		if (deflate(zs, Z_FINISH) == Z_STREAM_END) dl = (int64_t)(BGZF_SLOT - BGZF_HEAD - BGZF_TAIL) - zs->avail_out;
	}
	if (dl < 0) {                                                // level 0, or data that deflate would grow beyond the block: one stored block
		d[0] = 1; d[1] = (uint8_t)n; d[2] = (uint8_t)(n >> 8); d[3] = (uint8_t)~n; d[4] = (uint8_t)(~n >> 8);
		memcpy(d + 5, in, (size_t)n);
		dl = 5 + n;
	}
	const int64_t total = BGZF_HEAD + dl + BGZF_TAIL;
	out[16] = (uint8_t)(total - 1); out[17] = (uint8_t)((total - 1) >> 8);
	const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n);
	uint8_t *t = d + dl;
	for (int k = 0; k < 4; ++k) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
	return total;
}

int write_all(int fd, const uint8_t *p, int64_t len)
{
	int64_t o = 0;
	while (o < len) {
		const ssize_t w = write(fd, p + o, (size_t)(len - o > (1ll << 30) ? (1ll << 30) : len - o));
		if (w < 0) { if (errno == EINTR) continue; fprintf(stderr, "[bwahip] writing BGZF blocks failed: %s\n", strerror(errno)); return BWAHIP_EIO; }
		o += w;
	}
	return 0;
}
} // namespace

// data -> BGZF blocks on fd (< 0: compressed and dropped).  The blocks are dealt to n_threads workers in contiguous runs, each run
// deflated into its own part of one buffer and the parts written in order: the file does not depend on n_threads.  Pieces of at
// most 256 MiB, so the buffer stays bounded.  level 0: stored, 1..9: zlib's levels.
// lens (may be NULL): receives the length of every member, in file order
static int bgzf_write_impl(int fd, const void *data, int64_t len, int level, int n_threads, int32_t *lens)
{
	if (len < 0 || (len && !data) || level < 0 || level > 9) return BWAHIP_EINVAL;
	if (n_threads < 1) n_threads = 1;
	if (n_threads > 256) n_threads = 256;
	const int64_t piece_blocks = 4096;
	// the block buffer is kept per calling thread and never initialised: a fresh, zero-filled quarter of a gigabyte per call would cost
	// the writer more than the deflate workers take at level 0
	struct Buf { uint8_t *p = nullptr; size_t cap = 0; ~Buf() { free(p); } };
	static thread_local Buf buf;
	for (int64_t p0 = 0; p0 < len; p0 += piece_blocks * BGZF_IN) {
		const uint8_t *in = (const uint8_t*)data + p0;
		const int64_t plen = len - p0 < piece_blocks * BGZF_IN ? len - p0 : piece_blocks * BGZF_IN;
		const int64_t nb = (plen + BGZF_IN - 1) / BGZF_IN;
		const int T = (int)(nb < n_threads ? nb : n_threads);
		if (buf.cap < (size_t)(nb * BGZF_SLOT)) {
			free(buf.p);
			buf.cap = (size_t)((nb < 64 ? 64 : nb) * BGZF_SLOT);
			buf.p = (uint8_t*)malloc(buf.cap);
			if (!buf.p) { buf.cap = 0; return BWAHIP_ENOMEM; }
		}
		uint8_t *const blocks = buf.p;                               // (the workers must not name the thread-local themselves: they would see their own)
		std::vector<int64_t> part_len((size_t)T, 0);
		std::vector<int> bad((size_t)T, 0);
		auto run = [&](int t) {
			z_stream zs;
			memset(&zs, 0, sizeof zs);
			if (level > 0 && deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { bad[(size_t)t] = 1; return; }
			uint8_t *o = blocks + nb * t / T * BGZF_SLOT;
			for (int64_t b = nb * t / T; b < nb * (t + 1) / T; ++b) {
				const int64_t n = plen - b * BGZF_IN < BGZF_IN ? plen - b * BGZF_IN : BGZF_IN;
				const int64_t m = bgzf_block(&zs, in + b * BGZF_IN, (int)n, level, o);
				if (lens) lens[p0 / BGZF_IN + b] = (int32_t)m;
				o += m;
			}
			part_len[(size_t)t] = o - (blocks + nb * t / T * BGZF_SLOT);
			if (level > 0) deflateEnd(&zs);
		};
		if (T == 1) run(0);
		else { std::vector<std::thread> th; for (int t = 0; t < T; ++t) th.emplace_back(run, t); for (auto &x : th) x.join(); }
		for (int t = 0; t < T; ++t) if (bad[(size_t)t]) return BWAHIP_ENOMEM;
		if (fd >= 0) for (int t = 0; t < T; ++t) { const int rc = write_all(fd, blocks + nb * t / T * BGZF_SLOT, part_len[(size_t)t]); if (rc) return rc; }
	}
	return 0;
}

extern "C" int bwahip_bgzf_write(int fd, const void *data, int64_t len, int level, int n_threads) { return bgzf_write_impl(fd, data, len, level, n_threads, nullptr); }

// bwahip_bgzf_write that also says how long every member is (member_len: room for cap lengths; fewer than the (len + 65279) / 65280
// members there will be: BWAHIP_ECAPACITY, before anything is written)
extern "C" int bwahip_bgzf_write_lens(int fd, const void *data, int64_t len, int level, int n_threads, int32_t *member_len, int64_t cap, int64_t *n_members)
{
	if (len < 0 || !n_members || cap < 0 || (cap && !member_len)) return BWAHIP_EINVAL;
	const int64_t nb = (len + BGZF_IN - 1) / BGZF_IN;
	if (nb > cap) return BWAHIP_ECAPACITY;
	*n_members = 0;
	const int rc = bgzf_write_impl(fd, data, len, level, n_threads, nb ? member_len : nullptr);
	if (!rc) *n_members = nb;
	return rc;
}

// the end-of-file marker of the specification: an empty block
extern "C" int bwahip_bgzf_eof(int fd)
{
	static const uint8_t eof[28] = { 0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	return fd < 0 ? 0 : write_all(fd, eof, 28);
}
