// The base-quality recalibration table of a coordinate-sorted BAM file (include/bwahip.h), the parts that the device-free
// builder (recal_host.cpp) shares with the device stage (k_recal.hip): how the options resolve, which record takes part, the covariates of a
// base, the mask, the dense tables and their one serialiser, and the whole of the device stage's private counting -- which cell of a workgroup's LDS a base
// goes to, how a quality claims a slot there, how the claimed slots are flushed -- so that a CPU program (tests/recal_slots_check.cpp) runs the
// same lines the kernel does.  A record is read and judged as for the pileup (pileup_tables.h).  Plain C++; __host__ __device__ where a HIP
// compiler reads it.
#pragma once
#include "pileup_tables.h"

#define RC_HD PU_HD

constexpr int RC_NQ = 94;                                        // the rows: Q = min(quality byte, 93)
constexpr int RC_NCTX = 17;                                      // the contexts: 4 x prev + this, 16 = none
constexpr int RC_MAX_CYCLE = 65536, RC_DEFAULT_CYCLE = 1024, RC_DEFAULT_EXCLUDE = 3844;
// The dense tables: RC_NQ rows of rc_ncol(max_cycle) cells, a cell is two 64-bit words (n_obs, n_err).  Column 0 is the quality table, then
// max_cycle columns of the first mate's cycles and max_cycle of the second's, then the RC_NCTX contexts.
RC_HD inline int64_t rc_ncol(int max_cycle) { return 1 + 2 * (int64_t)max_cycle + RC_NCTX; }
RC_HD inline int64_t rc_col_cycle(int max_cycle, uint32_t mate, uint32_t c) { return 1 + (int64_t)mate * max_cycle + c; }
RC_HD inline int64_t rc_col_context(int max_cycle, uint32_t x) { return 1 + 2 * (int64_t)max_cycle + x; }
RC_HD inline int64_t rc_cell(int max_cycle, uint32_t Q, int64_t col) { return 2 * (Q * rc_ncol(max_cycle) + col); }
inline int64_t rc_table_words(int max_cycle) { return 2 * RC_NQ * rc_ncol(max_cycle); }

// the pileup's rule, and a first quality byte that is not 0xff (l_seq > 0 holds when it is read)
RC_HD inline bool rc_takes_part(const PuRec &r, const bwahip_recal_opt_t &o)
{
	return r.q.ref >= 0 && !(r.q.flag & (uint32_t)o.exclude_flags) && r.q.mapq >= (uint32_t)o.min_mapq && r.l_seq > 0 && pu_query_len(r) == r.l_seq && r.qual[0] != 0xff;
}

RC_HD inline uint32_t rc_quality(uint32_t b) { return b < RC_NQ - 1 ? b : RC_NQ - 1; }
RC_HD inline uint32_t rc_cycle(bool rev, int32_t l_seq, int64_t q) { return (uint32_t)(rev ? l_seq - 1 - q : q); }
// where the base read one cycle earlier lies (looked at for a cycle > 0 only: then it is inside the read)
RC_HD inline int64_t rc_prev_index(bool rev, int64_t q) { return rev ? q + 1 : q - 1; }
// this2: the base as 0..3; prev2: the base read one cycle earlier, < 0 when it is not A C G T.  Both as stored; a reverse record complements both
RC_HD inline uint32_t rc_context(bool rev, uint32_t cycle, int this2, int prev2)
{
	if (cycle == 0 || prev2 < 0) return 16;
	return rev ? 4u * (uint32_t)(3 - prev2) + (uint32_t)(3 - this2) : 4u * (uint32_t)prev2 + (uint32_t)this2;
}
RC_HD inline bool rc_masked(const uint8_t *mask, int64_t g) { return mask && (mask[g >> 3] >> (g & 7) & 1); }

// The walk of a record that takes part (l_seq <= max_cycle), on a contig of L bases that begins at base g0 of the packed reference, one base
// after the other: count(Q, mate, cycle, context, error) for every counted base, masked() for every base only the mask keeps out
template <class Count, class Masked> RC_HD inline void rc_walk(const PuRec &r, int64_t L, int64_t g0, const uint8_t *pac, const uint8_t *mask, int min_baseq, Count count, Masked masked)
{
	const bool rev = (r.q.flag & 0x10) != 0;
	const uint32_t mate = r.q.flag >> 7 & 1;
	int64_t p = r.q.pos, q = 0;
	for (int32_t k = 0; k < r.q.n_cigar; ++k) {
		const uint32_t w = bam_ld32(r.q.cig + 4 * k), op = w & 15;
		const int64_t n = w >> 4;
		if (pu_is_match(op)) {
			for (int64_t j = 0; j < n && p + j < L; ++j) {
				const int c2 = pu_code2(pu_base(r.seq, q + j));
				const uint32_t b = r.qual[q + j];
				if (c2 < 0 || b < (uint32_t)min_baseq) continue;
				if (rc_masked(mask, g0 + p + j)) { masked(); continue; }
				const uint32_t c = rc_cycle(rev, r.l_seq, q + j);
				const int prev2 = c ? pu_code2(pu_base(r.seq, rc_prev_index(rev, q + j))) : -1;
				count(rc_quality(b), mate, c, rc_context(rev, c, c2, prev2), (uint32_t)c2 != pu_ref2(pac, g0 + p + j));
			}
			p += n; q += n;
		} else if (op == 2 || op == 3) p += n;
		else if (op == 1 || op == 4) q += n;
	}
}

// ---- The private counting of the device stage (k_recal.hip).  A workgroup counts a share of RC_SHARE consecutive records in 32-bit cells
// of its LDS and adds every non-zero cell to the dense tables once, at its end.  Two arrays of pairs (n_obs, n_err): the context table
// whole (RC_NQ x RC_NCTX), and the cycle table for the cycles below RC_LDS_CYCLES of RC_LDS_SLOTS qualities.  A quality gets its slot at
// its first base: tag[slot] goes from RC_SLOT_EMPTY to Q by compare-and-swap and never changes again.  A base whose cycle or quality has
// no cell there goes straight to the dense table.  The kernel body holds none of this: it hands in functors over its arrays.
// 32 bits hold a cell: it counts at most one base per cycle and record (the context table: one per base), a record that is counted has
// at most RC_MAX_CYCLE bases (a longer one is refused before its walk), so a cell stays below RC_SHARE x RC_MAX_CYCLE = 2^25.
constexpr int RC_SHARE = 512, RC_LDS_SLOTS = 8, RC_LDS_CYCLES = 256;
constexpr int RC_LDS_CTX_WORDS = 2 * RC_NQ * RC_NCTX, RC_LDS_CYC_WORDS = 2 * RC_LDS_SLOTS * 2 * RC_LDS_CYCLES;
constexpr uint32_t RC_SLOT_EMPTY = 0xffffffffu;                   // no quality: as one it lies outside the dense table
static_assert(RC_SLOT_EMPTY >= (uint32_t)RC_NQ && (int64_t)RC_SHARE * RC_MAX_CYCLE < (1ll << 32), "the empty tag is no quality; a cell holds a share");
RC_HD inline int rc_lds_ctx_cell(uint32_t Q, uint32_t x) { return 2 * (int)(Q * RC_NCTX + x); }                                   // Q < RC_NQ, x < RC_NCTX
RC_HD inline int rc_lds_cyc_cell(int slot, uint32_t mate, uint32_t c) { return 2 * (int)(((uint32_t)slot * 2 + mate) * RC_LDS_CYCLES + c); }   // 0 <= slot < RC_LDS_SLOTS, mate < 2, c < RC_LDS_CYCLES

// The slot of quality Q < RC_NQ, claimed here if it has none and one is empty; -1: every slot holds another quality.  load(s): tag[s];
// cas(s, expected, desired): the compare-and-swap on tag[s], returns what was there.  A tag only ever goes from RC_SLOT_EMPTY to a quality,
// and a slot is passed only when it holds another quality, so a quality never has two slots, whoever else claims meanwhile.
template <class Load, class Cas> RC_HD inline int rc_slot_claim(uint32_t Q, Load load, Cas cas)
{
	for (int s = 0; s < RC_LDS_SLOTS; ++s) {
		uint32_t t = load(s);
		if (t == RC_SLOT_EMPTY) { t = cas(s, RC_SLOT_EMPTY, Q); if (t == RC_SLOT_EMPTY) return s; }
		if (t == Q) return s;
	}
	return -1;
}

// One counted base.  ctx_add(cell, error) and cyc_add(cell, error) add (1, error) to the pair at that cell of the two LDS arrays,
// tab_add(word, error) to the pair at that word of the dense tables
template <class Load, class Cas, class CtxAdd, class CycAdd, class TabAdd>
RC_HD inline void rc_count_base(int max_cycle, uint32_t Q, uint32_t mate, uint32_t c, uint32_t x, bool error, Load load, Cas cas, CtxAdd ctx_add, CycAdd cyc_add, TabAdd tab_add)
{
	ctx_add(rc_lds_ctx_cell(Q, x), error);
	const int slot = c < (uint32_t)RC_LDS_CYCLES ? rc_slot_claim(Q, load, cas) : -1;
	if (slot >= 0) cyc_add(rc_lds_cyc_cell(slot, mate, c), error);
	else tab_add(rc_cell(max_cycle, Q, rc_col_cycle(max_cycle, mate, c)), error);
}

// The flush of a share, by `step` workers of which this is worker `first`: flush(word, n_obs, n_err) for every non-zero pair, `word` its
// place in the dense tables.  The quality column gets the context table's row sums.  An unclaimed slot is skipped before anything is
// formed from its tag; so is a cycle the table has no column for (nothing was counted there: a counted record has at most max_cycle bases).
// load(s): tag[s]; ctx(i), cyc(i): word i of the two LDS arrays
template <class Load, class Ctx, class Cyc, class Flush> RC_HD inline void rc_flush(int max_cycle, int first, int step, Load load, Ctx ctx, Cyc cyc, Flush flush)
{
	for (int i = first; i < RC_NQ * RC_NCTX; i += step) {
		const uint32_t Q = (uint32_t)i / RC_NCTX, x = (uint32_t)i % RC_NCTX;
		const int cell = rc_lds_ctx_cell(Q, x);
		const uint32_t n = ctx(cell), e = ctx(cell + 1);
		if (n) flush(rc_cell(max_cycle, Q, rc_col_context(max_cycle, x)), n, e);
	}
	for (int i = first; i < RC_NQ; i += step) {
		uint64_t n = 0, e = 0;
		for (uint32_t x = 0; x < (uint32_t)RC_NCTX; ++x) { n += ctx(rc_lds_ctx_cell((uint32_t)i, x)); e += ctx(rc_lds_ctx_cell((uint32_t)i, x) + 1); }
		if (n) flush(rc_cell(max_cycle, (uint32_t)i, 0), n, e);
	}
	for (int i = first; i < RC_LDS_SLOTS * 2 * RC_LDS_CYCLES; i += step) {
		const int slot = i / (2 * RC_LDS_CYCLES);
		const uint32_t mate = (uint32_t)i / RC_LDS_CYCLES & 1, c = (uint32_t)i % RC_LDS_CYCLES, Q = load(slot);
		if (Q >= (uint32_t)RC_NQ || c >= (uint32_t)max_cycle) continue;   // nobody claimed the slot
		const int cell = rc_lds_cyc_cell(slot, mate, c);
		const uint32_t n = cyc(cell), e = cyc(cell + 1);
		if (n) flush(rc_cell(max_cycle, Q, rc_col_cycle(max_cycle, mate, c)), n, e);
	}
}

// The tables of a file: tab = rc_table_words(opt.max_cycle) words as laid out above.  opt: as resolved.  n_bases and n_err are the sums of
// the quality table.
struct RcTables {
	int32_t n_ref = 0;
	bwahip_recal_opt_t opt = { 0, 0, RC_DEFAULT_EXCLUDE, RC_DEFAULT_CYCLE };
	uint64_t n_records = 0, n_masked = 0;
	const uint64_t *tab = nullptr;
};
// recal_host.cpp
int rc_resolve(const bwahip_recal_opt_t *in, bwahip_recal_opt_t *out);           // NULL: the defaults; BWAHIP_EINVAL for a value out of range
int rc_serialise(const RcTables &t, std::vector<uint8_t> *out);
