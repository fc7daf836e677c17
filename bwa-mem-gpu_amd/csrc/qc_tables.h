// The QC summary of a coordinate-sorted BAM file (include/bwahip.h), the parts that the device-free builder (qc_host.cpp)
// and the device stage (k_qc.hip) share: how one record is read and judged, which counts it adds to, and the compact tables that both
// hand to the one serialiser.  Plain C++; __host__ __device__ where a HIP compiler reads it.
#pragma once
#include "../../include/bwahip.h"
#include "bam_rec.h"
#include <stdint.h>
#include <string.h>
#include <vector>

#define QC_HD BAM_HD

constexpr int QC_TILE = 2048;                    // slots of the difference array one workgroup scans; a reference's slots are padded to whole tiles
// the fixed part of the tables, in 64-bit words: records without a reference, count[2][16], the three histograms
constexpr int QC_NO_COOR = 0, QC_COUNT = 1, QC_MAPQ = QC_COUNT + 32, QC_ISIZE = QC_MAPQ + 256, QC_DEPTH = QC_ISIZE + 1025, QC_FIXED = QC_DEPTH + 256;
constexpr int QC_PER_REF = 3;                    // then per reference: mapped, placed_unmapped, covered; then the windows of all references

struct QcRec { int32_t ref, pos, next_ref, tlen; uint32_t flag, mapq; const uint8_t *cig; int32_t n_cigar; };

// One record of `len` bytes at p: the checks of bai_parse (bai_tables.h), no byte beyond p + len is read.  false: not a BAM record of n_ref references.
QC_HD inline bool qc_parse(const uint8_t *p, int64_t len, int32_t n_ref, QcRec *r)
{
	if (len < 36) return false;
	if ((int64_t)(int32_t)bam_ld32(p) + 4 != len) return false;
	const uint32_t w3 = bam_ld32(p + 12), w4 = bam_ld32(p + 16);
	const int64_t l_read_name = w3 & 0xff, n_cigar = w4 & 0xffff;
	if (36 + l_read_name + 4 * n_cigar > len) return false;
	r->ref = (int32_t)bam_ld32(p + 4); r->pos = (int32_t)bam_ld32(p + 8);
	if (r->ref >= n_ref || (r->ref >= 0 && r->pos < 0)) return false;
	r->mapq = w3 >> 8 & 0xff; r->flag = w4 >> 16; r->n_cigar = (int32_t)n_cigar;
	r->next_ref = (int32_t)bam_ld32(p + 24); r->tlen = (int32_t)bam_ld32(p + 32);
	r->cig = p + 36 + l_read_name;
	return true;
}

// bit k: the record counts in count[q][k]
QC_HD inline uint32_t qc_categories(const QcRec &r)
{
	const uint32_t f = r.flag;
	const bool prim = !(f & 0x900), mapped = !(f & 0x4), dup = (f & 0x400) != 0;
	uint32_t m = 1u;
	if (prim) m |= 1u << 1;
	if (f & 0x100) m |= 1u << 2;
	if ((f & 0x900) == 0x800) m |= 1u << 3;
	if (dup) m |= 1u << 4;
	if (dup && prim) m |= 1u << 5;
	if (mapped) m |= 1u << 6;
	if (mapped && prim) m |= 1u << 7;
	if (prim && (f & 0x1)) {
		m |= 1u << 8;
		if (f & 0x40) m |= 1u << 9;
		if (f & 0x80) m |= 1u << 10;
		if ((f & 0x2) && mapped) m |= 1u << 11;
		if (mapped && !(f & 0x8)) {
			m |= 1u << 12;
			if (r.next_ref != r.ref) { m |= 1u << 14; if (r.mapq >= 5) m |= 1u << 15; }
		}
		if (mapped && (f & 0x8)) m |= 1u << 13;
	}
	return m;
}
QC_HD inline bool qc_in_mapq_hist(const QcRec &r) { return !(r.flag & 0x904); }
QC_HD inline bool qc_in_isize_hist(const QcRec &r) { return (r.flag & 0x90f) == 0x3 && r.tlen > 0; }
QC_HD inline bool qc_covers(const QcRec &r, const bwahip_qc_opt_t &o) { return r.ref >= 0 && !(r.flag & (uint32_t)o.exclude_flags) && r.mapq >= (uint32_t)o.min_mapq; }

// The covered intervals of a record on a reference of L bases, clipped, neighbours joined (an insertion or a clip between two covering
// operations does not part them; N does): put(a, b) for every [a, b) with 0 <= a < b <= L
template <class Put> QC_HD inline void qc_intervals(const QcRec &r, int64_t L, Put put)
{
	int64_t p = r.pos, a = -1;
	for (int32_t k = 0; k <= r.n_cigar; ++k) {
		const uint32_t w = k < r.n_cigar ? bam_ld32(r.cig + 4 * k) : 3u, op = w & 15;   // behind the last operation: an N of no length
		const int64_t n = w >> 4;
		if (op == 0 || op == 2 || op == 7 || op == 8) { if (a < 0) a = p; p += n; }
		else if (op == 3) {
			if (a >= 0) { const int64_t b = p < L ? p : L; if (a < b) put(a, b); a = -1; }
			p += n;
		}
	}
}

inline int64_t qc_windows(int64_t len, int shift) { return (len + (1ll << shift) - 1) >> shift; }
// the bytes of a summary's file: magic, n_ref and the three options, the fixed words, six words per reference, the windows
inline int64_t qc_file_bytes(int64_t n_ref, int64_t n_windows) { return 20 + 8 * QC_FIXED + 48 * n_ref + 8 * n_windows; }

// The compact tables of a summary.  fixed: QC_FIXED words; per_ref: QC_PER_REF words per reference; win: the windows of all references one
// after the other, reference r has qc_windows(ref_len[r], opt.window_shift) of them.  opt: as resolved.
struct QcTables {
	int32_t n_ref = 0;
	const int64_t *ref_len = nullptr;
	bwahip_qc_opt_t opt = { 14, 1796, 0 };
	const uint64_t *fixed = nullptr, *per_ref = nullptr, *win = nullptr;
};
// qc_host.cpp
int qc_resolve(const bwahip_qc_opt_t *in, bwahip_qc_opt_t *out);               // NULL: the defaults; BWAHIP_EINVAL for a value out of range
int qc_serialise(const QcTables &t, std::vector<uint8_t> *out);
