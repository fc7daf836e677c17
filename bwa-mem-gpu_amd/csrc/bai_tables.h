// The BAI index of a coordinate-sorted BAM file (SAM specification 5.2, 5.3), the parts that the device-free builder (bai_host.cpp) and
// the device stage (k_bai.hip) share: how one record is read and judged, the virtual offset of a position of the uncompressed record
// stream, and the compact tables that both hand to the one serialiser.  Plain C++; __host__ __device__ where a HIP compiler reads it.
#pragma once
#include "bam_rec.h"
#include <stdint.h>
#include <string.h>
#include <vector>

#define BAI_HD BAM_HD

constexpr int64_t BAI_BLOCK_IN = 65280;          // the record stream is cut into BGZF members every 65 280 bytes
constexpr int32_t BAI_MAX_END = 1 << 29;         // the last position the binning scheme of BAI holds
constexpr uint32_t BAI_META_BIN = 37450;         // the pseudo-bin that carries a reference's extent and its record counts
constexpr int BAI_BAD = 1, BAI_TOO_FAR = 2;      // what bai_parse says of a record it refuses: BWAHIP_EINVAL, BWAHIP_ECAPACITY

struct BaiRec { int32_t ref, pos, e; uint32_t bin; int unm; };

// One record of `len` bytes at p.  No byte beyond p + len is read: every field is bounded by the length first.  0: *r is filled (a record
// without a reference: ref < 0, nothing else means anything); BAI_BAD: not a BAM record of n_ref references; BAI_TOO_FAR: it ends beyond 2^29.
BAI_HD inline int bai_parse(const uint8_t *p, int64_t len, int32_t n_ref, BaiRec *r)
{
	if (len < 36) return BAI_BAD;
	if ((int64_t)(int32_t)bam_ld32(p) + 4 != len) return BAI_BAD;
	const int32_t ref = (int32_t)bam_ld32(p + 4), pos = (int32_t)bam_ld32(p + 8);
	const uint32_t w3 = bam_ld32(p + 12), w4 = bam_ld32(p + 16);
	const int64_t l_read_name = w3 & 0xff, n_cigar = w4 & 0xffff;
	if (36 + l_read_name + 4 * n_cigar > len) return BAI_BAD;
	if (ref >= n_ref || (ref >= 0 && pos < 0)) return BAI_BAD;
	r->ref = ref; r->pos = pos; r->unm = (int)(w4 >> 18 & 1); r->e = 0; r->bin = 0;
	if (ref < 0) return 0;
	int64_t rlen = 0;
	const uint8_t *cig = p + 36 + l_read_name;
	for (int64_t k = 0; k < n_cigar; ++k) {
		const uint32_t w = bam_ld32(cig + 4 * k), op = w & 15;
		if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += w >> 4;   // M D N = X
	}
	const int64_t e = rlen > 0 && !r->unm ? (int64_t)pos + rlen : (int64_t)pos + 1;
	if (e > BAI_MAX_END) return BAI_TOO_FAR;
	r->e = (int32_t)e; r->bin = bam_reg2bin(pos, e);
	return 0;
}

// coordinate order: refID as unsigned, then pos; records without a reference are ordered by their refID alone
BAI_HD inline uint64_t bai_order_key(int32_t ref, int32_t pos) { return (uint64_t)(uint32_t)ref << 32 | (ref < 0 ? 0u : (uint32_t)pos); }

// The virtual offset of byte u of the record stream of `total` bytes.  c: the offsets of the members in the file, counted from the first
// member of the records (c[b], b <= n_blocks; c[n_blocks] is where the end-of-file block goes); base: the file offset of that member.
BAI_HD inline uint64_t bai_voffset(int64_t u, int64_t total, const int64_t *c, int64_t n_blocks, int64_t base)
{
	if (u >= total) return (uint64_t)(base + c[n_blocks]) << 16;
	return (uint64_t)(base + c[u / BAI_BLOCK_IN]) << 16 | (uint64_t)(u % BAI_BLOCK_IN);
}

// The compact tables of an index.  Chunks: sorted by key = refID << 16 | bin, in file order within a key, already joined.  meta: four
// words per reference -- begin of its first record, end of its last, records with 0x4 clear, with 0x4 set (both 0: no record).  lin: the
// linear index of all references one after the other, windows without a record filled; reference r has lin_off[r + 1] - lin_off[r] windows.
struct BaiTables {
	int32_t n_ref = 0;
	int64_t n_chunks = 0;
	const uint64_t *ckey = nullptr, *cbeg = nullptr, *cend = nullptr;
	const uint64_t *meta = nullptr;
	const int64_t *lin_off = nullptr;
	const uint64_t *lin = nullptr;
	uint64_t n_no_coor = 0;
};
// bai_host.cpp: the tables as the bytes of a .bai file; BWAHIP_EINVAL for tables that do not fit together
int bai_serialise(const BaiTables &t, std::vector<uint8_t> *out);

// bam_sort_host.cpp: bwahip_bam_merger_finish with a listener -- every record as it is emitted (whole, in file order), the lengths of
// the members of every piece as it leaves the BGZF writer; a hook's non-zero return ends the merge with that code
struct MergeHooks { int (*record)(void *arg, const uint8_t *rec, int64_t len); int (*members)(void *arg, const int32_t *member_len, int64_t n); void *arg; };
struct bwahip_bam_merger;
int bam_merger_finish_hooks(bwahip_bam_merger *m, int fd, int level, int n_threads, const MergeHooks *hooks);
// a listener that stays with the merger: every finish tells it every record as it is emitted, beside the hooks (record == nullptr: nobody listens)
int bam_merger_listen(bwahip_bam_merger *m, int (*record)(void *arg, const uint8_t *rec, int64_t len), void *arg);
