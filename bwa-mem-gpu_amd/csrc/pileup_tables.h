// The pileup of candidate variant sites of a coordinate-sorted BAM file (include/bwahip.h), the parts that the device-free
// builder (pileup_host.cpp) and the device stage (k_pileup.hip) share: how the options resolve, how one record is read and judged, how a
// base, a reference base and an observation's key are formed, the walk of one record, and the compact tables that both hand to the one
// serialiser.  Plain C++; __host__ __device__ where a HIP compiler reads it.
#pragma once
#include "qc_tables.h"

#define PU_HD QC_HD

constexpr int PU_SNV = 0, PU_DEL = 1, PU_INS = 2;
constexpr uint32_t PU_DEL_CAP = (1u << 21) - 1;                   // a deletion's length in its allele
constexpr int64_t PU_MAX_SUM = 1ll << 40;                        // the sum of the contig lengths stays below it (check_refs, sidecar_host.h): a global position takes 40 bits
constexpr int64_t PU_MAX_OBS = 0x7fffffffll;

// a record that passed qc_parse and the two checks of the bases
struct PuRec { QcRec q; int32_t l_seq; const uint8_t *seq, *qual; };

PU_HD inline bool pu_parse(const uint8_t *p, int64_t len, int32_t n_ref, PuRec *r)
{
	if (!qc_parse(p, len, n_ref, &r->q)) return false;
	const int32_t l_seq = (int32_t)bam_ld32(p + 20);
	if (l_seq < 0) return false;
	const int64_t at = 36 + (int64_t)(bam_ld32(p + 12) & 0xff) + 4 * (int64_t)r->q.n_cigar;
	if (at + ((int64_t)l_seq + 1) / 2 + l_seq > len) return false;
	r->l_seq = l_seq; r->seq = p + at; r->qual = r->seq + ((int64_t)l_seq + 1) / 2;
	return true;
}

PU_HD inline bool pu_is_match(uint32_t op) { return op == 0 || op == 7 || op == 8; }

// the query length of the CIGAR: M I S = X
PU_HD inline int64_t pu_query_len(const PuRec &r)
{
	int64_t n = 0;
	for (int32_t k = 0; k < r.q.n_cigar; ++k) {
		const uint32_t w = bam_ld32(r.q.cig + 4 * k), op = w & 15;
		if (pu_is_match(op) || op == 1 || op == 4) n += w >> 4;
	}
	return n;
}

PU_HD inline bool pu_takes_part(const PuRec &r, const bwahip_pileup_opt_t &o)
{
	return r.q.ref >= 0 && !(r.q.flag & (uint32_t)o.exclude_flags) && r.q.mapq >= (uint32_t)o.min_mapq && r.l_seq > 0 && pu_query_len(r) == r.l_seq;
}

PU_HD inline uint32_t pu_base(const uint8_t *seq, int64_t q) { return seq[q >> 1] >> ((~q & 1) << 2) & 15; }   // the BAM code of base q
PU_HD inline int pu_code2(uint32_t code) { return code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : -1; }   // A C G T as 0..3, anything else -1
PU_HD inline uint32_t pu_ref2(const uint8_t *pac, int64_t g) { return pac[g >> 2] >> ((~g & 3) << 1) & 3; }   // .pac's layout

// an allele's 21 bits in the key: ascending by them is ascending by (len, bases) within a kind
PU_HD inline uint32_t pu_allele21(int kind, uint32_t len, uint32_t bases) { return kind == PU_SNV ? bases : kind == PU_DEL ? len : len << 16 | bases; }
PU_HD inline uint64_t pu_key(int64_t gpos, int kind, uint32_t allele21, uint32_t strand) { return (uint64_t)gpos << 24 | (uint64_t)kind << 22 | (uint64_t)allele21 << 1 | strand; }
PU_HD inline void pu_unkey(uint64_t key, int64_t *gpos, uint32_t *kind, uint32_t *len, uint32_t *bases)
{
	const uint32_t a = (uint32_t)(key >> 1) & 0x1fffff;
	*gpos = (int64_t)(key >> 24); *kind = (uint32_t)(key >> 22) & 3;
	*len = *kind == PU_SNV ? 1 : *kind == PU_DEL ? a : a >> 16;
	*bases = *kind == PU_SNV ? a : *kind == PU_DEL ? 0 : a & 0xffff;
}
// the allele of an insertion of n > 0 bases from base q on, all of them A C G T
PU_HD inline uint32_t pu_ins_allele(const uint8_t *seq, int64_t q, int64_t n)
{
	uint32_t bases = 0;
	for (int j = 0; j < 8 && j < n; ++j) bases |= (uint32_t)pu_code2(pu_base(seq, q + j)) << (2 * j);
	return pu_allele21(PU_INS, (uint32_t)(n < 31 ? n : 31), bases);
}

// The walk of a record that takes part, on a contig of L bases that begins at base g0 of the packed reference, one base after the other:
// cover(p) for every base of [0, L) an M = X or D operation covers, match(p) for an M = X base that passes and equals the reference,
// obs(p, kind, allele21) for every observation.  Operations of no length give nothing.
template <class Cover, class Match, class Obs> PU_HD inline void pu_walk(const PuRec &r, int64_t L, int64_t g0, const uint8_t *pac, int min_baseq, Cover cover, Match match, Obs obs)
{
	const bool all_pass = r.qual[0] == 0xff;
	int64_t p = r.q.pos, q = 0;
	for (int32_t k = 0; k < r.q.n_cigar; ++k) {
		const uint32_t w = bam_ld32(r.q.cig + 4 * k), op = w & 15;
		const int64_t n = w >> 4;
		if (pu_is_match(op)) {
			for (int64_t j = 0; j < n && p + j < L; ++j) {
				cover(p + j);
				const int c2 = pu_code2(pu_base(r.seq, q + j));
				if (c2 < 0 || !(all_pass || r.qual[q + j] >= min_baseq)) continue;
				if ((uint32_t)c2 == pu_ref2(pac, g0 + p + j)) match(p + j); else obs(p + j, PU_SNV, pu_allele21(PU_SNV, 1, (uint32_t)c2));
			}
			p += n; q += n;
		} else if (op == 2) {
			if (n && p < L) obs(p, PU_DEL, pu_allele21(PU_DEL, n < PU_DEL_CAP ? (uint32_t)n : PU_DEL_CAP, 0));
			for (int64_t j = 0; j < n && p + j < L; ++j) cover(p + j);
			p += n;
		} else if (op == 1) {
			bool acgt = n > 0 && p < L;
			for (int64_t j = 0; acgt && j < n; ++j) acgt = pu_code2(pu_base(r.seq, q + j)) >= 0;
			if (acgt) obs(p, PU_INS, pu_ins_allele(r.seq, q, n));
			q += n;
		} else if (op == 3) p += n;
		else if (op == 4) q += n;
	}
}

// The compact tables of a pileup: the kept alleles in the file's order, the sites in the file's order (first: the site's first allele).
// gpos: the position among the bases of all contigs.  opt: as resolved.
struct PuAllele { uint64_t gpos; uint32_t kind, len, bases, fwd, rev, pad; };
struct PuSite { uint64_t gpos; uint32_t ref_base, first, n_cov, n_ref_fwd, n_ref_rev, pad; };
struct PuTables {
	int32_t n_ref = 0;
	const int64_t *ref_len = nullptr;
	bwahip_pileup_opt_t opt = { 0, 0, 1796, 2 };
	uint64_t n_obs[3] = { 0, 0, 0 };
	int64_t n_alleles = 0, n_sites = 0;
	const PuAllele *alleles = nullptr;
	const PuSite *sites = nullptr;
};
// pileup_host.cpp
int pu_resolve(const bwahip_pileup_opt_t *in, bwahip_pileup_opt_t *out);        // NULL: the defaults; BWAHIP_EINVAL for a value out of range
int pu_serialise(const PuTables &t, std::vector<uint8_t> *out);
