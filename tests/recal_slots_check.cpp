// The private counting of the recalibration-table stage (csrc/recal_tables.h: rc_slot_claim, rc_count_base, rc_flush and the LDS cell
// indices -- the lines csrc/k_recal.hip compiles into its kernel), played by one thread: a stand-alone program, built with the address
// and undefined-behaviour sanitizers by tests/test_recal_slots_cpu.py.  A share of records is counted as a workgroup counts it -- arrays
// of exactly the LDS arrays' sizes, each an allocation of its own, the claim with a serial compare-and-swap, the flush by 256 workers one
// after the other into a dense table of exactly rc_table_words words -- and the dense table must equal, word for word, the one rc_walk
// fills as the host builder does.  Prints "ok"; any difference, or a report of a sanitizer, fails the test.
#include "recal_tables.h"
#include <random>
#include <stdio.h>
#include <stdlib.h>

static int fails = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static void put32le(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }

// a BAM record: name "r", the CIGAR as (length, operation) pairs, the bases as BAM codes, the quality bytes
static std::vector<uint8_t> make_rec(int32_t ref, int32_t pos, uint32_t flag, uint32_t mapq, const std::vector<std::pair<uint32_t, uint32_t>> &cig, const std::vector<uint8_t> &codes,
                                     const std::vector<uint8_t> &qual)
{
	std::vector<uint8_t> o;
	put32le(o, 0);
	put32le(o, (uint32_t)ref); put32le(o, (uint32_t)pos);
	put32le(o, 2u | mapq << 8 | 4680u << 16);
	put32le(o, (uint32_t)cig.size() | flag << 16);
	put32le(o, (uint32_t)codes.size());
	put32le(o, (uint32_t)-1); put32le(o, (uint32_t)-1); put32le(o, 0);
	o.push_back('r'); o.push_back(0);
	for (auto &c : cig) put32le(o, c.first << 4 | c.second);
	for (size_t k = 0; k < codes.size(); k += 2) o.push_back((uint8_t)(codes[k] << 4 | (k + 1 < codes.size() ? codes[k + 1] : 0)));
	o.insert(o.end(), qual.begin(), qual.end());
	const uint32_t bs = (uint32_t)o.size() - 4;
	for (int k = 0; k < 4; ++k) o[(size_t)k] = (uint8_t)(bs >> (8 * k));
	return o;
}

struct Genome {
	std::vector<int64_t> len{ 3000, 517 }, off{ 0, 3000, 3517 };
	std::vector<uint8_t> pac, mask;                                 // exactly the bytes the rule reads
	explicit Genome(std::mt19937 &rng) : pac((3517 + 3) / 4), mask((3517 + 7) / 8)
	{
		for (auto &b : pac) b = (uint8_t)rng();
		for (auto &b : mask) b = rng() % 8 == 0 ? (uint8_t)rng() : 0;
	}
	uint8_t code(int r, int64_t p) const { return (uint8_t)(1u << pu_ref2(pac.data(), off[(size_t)r] + p)); }
};

// a record of n bases over [pos, pos + n) of contig r, one base in nine changed, with these qualities (cycled through)
static std::vector<uint8_t> read_at(const Genome &g, std::mt19937 &rng, int r, int32_t pos, int n, uint32_t flag, const std::vector<uint8_t> &quals, uint32_t clip = 0)
{
	std::vector<uint8_t> codes, qual;
	std::vector<std::pair<uint32_t, uint32_t>> cig;
	if (clip) { cig.push_back({ clip, 4 }); for (uint32_t k = 0; k < clip; ++k) { codes.push_back(k & 1 ? 15 : 2); qual.push_back(9); } }
	cig.push_back({ (uint32_t)n, 0 });
	for (int k = 0; k < n; ++k) {
		const int64_t p = pos + k;
		uint8_t c = p < g.len[(size_t)r] ? g.code(r, p) : 1;
		if (rng() % 9 == 0) c = (uint8_t)(1u << rng() % 4);
		if (rng() % 61 == 0) c = 15;
		codes.push_back(c);
		qual.push_back(quals[(size_t)(rng() % quals.size())]);
	}
	if (qual[0] == 0xff) qual[0] = 0xfe;
	return make_rec(r, pos, flag, 60, cig, codes, qual);
}

struct Played { std::vector<uint64_t> tab; uint64_t n_records = 0, n_masked = 0; int claimed = 0; uint64_t early_to_tab = 0; };

// One share as a workgroup counts it.  `with_mask`: the genome's mask
static Played play(const Genome &g, const std::vector<std::vector<uint8_t>> &share, const bwahip_recal_opt_t &opt, bool with_mask)
{
	const int mc = opt.max_cycle;
	Played out;
	out.tab.assign((size_t)rc_table_words(mc), 0);
	std::vector<uint32_t> ctx((size_t)RC_LDS_CTX_WORDS, 0), cyc((size_t)RC_LDS_CYC_WORDS, 0), tag((size_t)RC_LDS_SLOTS, RC_SLOT_EMPTY);
	std::vector<uint64_t> &tab = out.tab;
	auto load = [&](int s) { return tag.at((size_t)s); };
	auto cas = [&](int s, uint32_t expected, uint32_t desired) { const uint32_t old = tag.at((size_t)s); if (old == expected) tag.at((size_t)s) = desired; return old; };
	CHECK((int)share.size() <= RC_SHARE);
	for (const auto &rec : share) {
		PuRec r;
		if (!pu_parse(rec.data(), (int64_t)rec.size(), (int32_t)g.len.size(), &r)) { CHECK(!"a record of the program's own does not parse"); continue; }
		if (!rc_takes_part(r, opt) || r.l_seq > mc) continue;
		++out.n_records;
		rc_walk(r, g.len[(size_t)r.q.ref], g.off[(size_t)r.q.ref], g.pac.data(), with_mask ? g.mask.data() : nullptr, opt.min_baseq,
		        [&](uint32_t Q, uint32_t mate, uint32_t c, uint32_t x, bool error) {
			        rc_count_base(mc, Q, mate, c, x, error, load, cas,
			                      [&](int cell, bool e) { ++ctx.at((size_t)cell); ctx.at((size_t)cell + 1) += e; },
			                      [&](int cell, bool e) { ++cyc.at((size_t)cell); cyc.at((size_t)cell + 1) += e; },
			                      [&](int64_t word, bool e) { ++tab.at((size_t)word); tab.at((size_t)word + 1) += e; out.early_to_tab += c < (uint32_t)RC_LDS_CYCLES; });
		        },
		        [&]() { ++out.n_masked; });
	}
	for (uint32_t t : tag) out.claimed += t != RC_SLOT_EMPTY;
	for (int first = 0; first < 256; ++first)
		rc_flush(mc, first, 256, load, [&](int i) { return ctx.at((size_t)i); }, [&](int i) { return cyc.at((size_t)i); },
		         [&](int64_t word, uint64_t n, uint64_t e) { CHECK(n > 0); tab.at((size_t)word) += n; tab.at((size_t)word + 1) += e; });
	return out;
}

// the same share as the host builder counts it (recal_host.cpp: rc_builder_add_one)
static Played judge(const Genome &g, const std::vector<std::vector<uint8_t>> &share, const bwahip_recal_opt_t &opt, bool with_mask)
{
	const int mc = opt.max_cycle;
	Played out;
	out.tab.assign((size_t)rc_table_words(mc), 0);
	for (const auto &rec : share) {
		PuRec r;
		if (!pu_parse(rec.data(), (int64_t)rec.size(), (int32_t)g.len.size(), &r) || !rc_takes_part(r, opt) || r.l_seq > mc) continue;
		++out.n_records;
		rc_walk(r, g.len[(size_t)r.q.ref], g.off[(size_t)r.q.ref], g.pac.data(), with_mask ? g.mask.data() : nullptr, opt.min_baseq,
		        [&](uint32_t Q, uint32_t mate, uint32_t c, uint32_t x, bool error) {
			        for (int64_t col : { (int64_t)0, rc_col_cycle(mc, mate, c), rc_col_context(mc, x) }) { uint64_t *cell = &out.tab.at((size_t)rc_cell(mc, Q, col)); ++cell[0]; cell[1] += error; }
		        },
		        [&]() { ++out.n_masked; });
	}
	return out;
}

// plays and judges a share; returns what was played
static Played both(const char *what, const Genome &g, const std::vector<std::vector<uint8_t>> &share, const bwahip_recal_opt_t &opt, bool with_mask = true)
{
	const Played a = play(g, share, opt, with_mask), b = judge(g, share, opt, with_mask);
	if (a.tab != b.tab || a.n_records != b.n_records || a.n_masked != b.n_masked) {
		size_t w = 0;
		while (w < a.tab.size() && a.tab[w] == b.tab[w]) ++w;
		fprintf(stderr, "%s: the played share differs from the walk: records %llu / %llu, masked %llu / %llu, first word %zu of %zu\n", what, (unsigned long long)a.n_records,
		        (unsigned long long)b.n_records, (unsigned long long)a.n_masked, (unsigned long long)b.n_masked, w, a.tab.size());
		++fails;
	}
	return a;
}

static uint64_t sum_of(const Played &p) { uint64_t s = 0; for (uint64_t w : p.tab) s += w; return s; }

int main()
{
	std::mt19937 rng(20260);
	const Genome g(rng);
	const bwahip_recal_opt_t dflt = { 0, 0, RC_DEFAULT_EXCLUDE, RC_DEFAULT_CYCLE };
	const uint32_t F1 = 0x1 | 0x40, F1R = F1 | 0x10, F2 = 0x1 | 0x80, F2R = F2 | 0x10;
	const uint32_t mates[4] = { F1, F1R, F2, F2R };

	{   // no record takes part: every slot is unclaimed at the flush, which must form nothing from their tags
		std::vector<std::vector<uint8_t>> share;
		for (int k = 0; k < 40; ++k) share.push_back(read_at(g, rng, k & 1, 10 * k, 50, mates[k & 3] | (k % 3 == 0 ? 0x4u : k % 3 == 1 ? 0x400u : 0x100u), { 30 }));
		share.push_back(make_rec(-1, -1, 0x4, 0, {}, { 1, 2 }, { 20, 20 }));
		const Played p = both("no record takes part", g, share, dflt);
		CHECK(p.n_records == 0 && p.claimed == 0 && sum_of(p) == 0);
		const Played q = both("no record at all", g, {}, dflt);
		CHECK(q.claimed == 0 && sum_of(q) == 0);
	}
	{   // exactly one quality
		std::vector<std::vector<uint8_t>> share;
		for (int k = 0; k < 100; ++k) share.push_back(read_at(g, rng, 0, 20 * k, 151, mates[k & 3], { 37 }));
		const Played p = both("one quality", g, share, dflt);
		CHECK(p.n_records == 100 && p.claimed == 1 && p.early_to_tab == 0 && sum_of(p) > 0);
	}
	{   // exactly as many qualities as there are slots: nothing of the early cycles goes past the LDS
		std::vector<uint8_t> q8;
		for (int k = 0; k < RC_LDS_SLOTS; ++k) q8.push_back((uint8_t)(2 + 5 * k));
		std::vector<std::vector<uint8_t>> share;
		for (int k = 0; k < RC_SHARE; ++k) share.push_back(read_at(g, rng, k % 2, (7 * k) % 400, 100, mates[k & 3], q8, k % 5 == 0 ? 3 : 0));
		const Played p = both("as many qualities as slots", g, share, dflt);
		CHECK(p.n_records == (uint64_t)RC_SHARE && p.claimed == RC_LDS_SLOTS && p.early_to_tab == 0);
		const Played u = both("as many qualities as slots, no mask", g, share, dflt, false);
		CHECK(u.n_masked == 0 && p.n_masked > 0);
	}
	{   // more qualities than slots: the overflow path
		std::vector<uint8_t> q;
		for (int k = 0; k < 94; ++k) q.push_back((uint8_t)k);
		std::vector<std::vector<uint8_t>> share;
		for (int k = 0; k < 200; ++k) share.push_back(read_at(g, rng, k % 2, (11 * k) % 500, 64, mates[k & 3], q));   // some across their contig's end
		const Played p = both("every quality", g, share, dflt);
		CHECK(p.claimed == RC_LDS_SLOTS && p.early_to_tab > 0);
		bwahip_recal_opt_t o = dflt;
		o.min_baseq = 20; o.min_mapq = 30; o.exclude_flags = 0;
		both("every quality, other options", g, share, o);
	}
	{   // Q = 93 from quality bytes above 93
		std::vector<std::vector<uint8_t>> share;
		for (int k = 0; k < 64; ++k) share.push_back(read_at(g, rng, 1, 3 * k, 33, mates[k & 3], { 93, 94, 100, 127, 200, 254, 255 }));
		const Played p = both("quality bytes above 93", g, share, dflt);
		CHECK(p.claimed == 1 && p.early_to_tab == 0);
		uint64_t other = 0;
		for (uint32_t Q = 0; Q + 1 < (uint32_t)RC_NQ; ++Q) other += p.tab[(size_t)rc_cell(dflt.max_cycle, Q, 0)];
		CHECK(other == 0 && p.tab[(size_t)rc_cell(dflt.max_cycle, RC_NQ - 1, 0)] > 0);
	}
	{   // cycles 255 and 256 on both mates, both strands: the last cell of the LDS, the first beyond it; and a read as long as max_cycle allows
		std::vector<std::vector<uint8_t>> share;
		for (int k = 0; k < 4; ++k) { share.push_back(read_at(g, rng, 0, 100 + k, 256, mates[k], { 11, 25 })); share.push_back(read_at(g, rng, 0, 200 + k, 257, mates[k], { 11, 25 })); }
		for (int k = 0; k < 4; ++k) share.push_back(read_at(g, rng, 0, 50 + k, 700, mates[k], { 25, 37 }));
		bwahip_recal_opt_t o = dflt;
		o.max_cycle = 700;
		const Played p = both("cycles 255 and 256", g, share, o);
		for (uint32_t mate = 0; mate < 2; ++mate) {
			uint64_t at255 = 0, at256 = 0, at699 = 0;
			for (uint32_t Q = 0; Q < (uint32_t)RC_NQ; ++Q) {
				at255 += p.tab[(size_t)rc_cell(700, Q, rc_col_cycle(700, mate, 255))]; at256 += p.tab[(size_t)rc_cell(700, Q, rc_col_cycle(700, mate, 256))];
				at699 += p.tab[(size_t)rc_cell(700, Q, rc_col_cycle(700, mate, 699))];
			}
			CHECK(at255 > 0 && at256 > 0 && at699 > 0);
		}
		o.max_cycle = 256;                                            // the longer ones are left out, as the kernel leaves a refused record out
		const Played s = both("max_cycle 256", g, share, o);
		CHECK(s.n_records == 4);
	}
	// the index helpers alone: the LDS cells are distinct pairs inside their arrays
	{
		std::vector<uint8_t> seen((size_t)RC_LDS_CYC_WORDS, 0);
		for (int s = 0; s < RC_LDS_SLOTS; ++s) for (uint32_t mate = 0; mate < 2; ++mate) for (uint32_t c = 0; c < (uint32_t)RC_LDS_CYCLES; ++c) {
			const int cell = rc_lds_cyc_cell(s, mate, c);
			CHECK(cell >= 0 && cell % 2 == 0 && cell + 1 < RC_LDS_CYC_WORDS && !seen.at((size_t)cell));
			seen.at((size_t)cell) = 1;
		}
		std::vector<uint8_t> seen2((size_t)RC_LDS_CTX_WORDS, 0);
		for (uint32_t Q = 0; Q < (uint32_t)RC_NQ; ++Q) for (uint32_t x = 0; x < (uint32_t)RC_NCTX; ++x) {
			const int cell = rc_lds_ctx_cell(Q, x);
			CHECK(cell >= 0 && cell % 2 == 0 && cell + 1 < RC_LDS_CTX_WORDS && !seen2.at((size_t)cell));
			seen2.at((size_t)cell) = 1;
		}
		CHECK(RC_SLOT_EMPTY >= (uint32_t)RC_NQ);
	}
	for (int mc : { 1, RC_MAX_CYCLE }) {   // max_cycle 1 and 65 536: every word rc_count_base and rc_flush can form lies in the dense tables, no two cells share one
		const int64_t words = rc_table_words(mc);
		for (uint32_t Q : { 0u, 1u, (uint32_t)RC_NQ - 1 })
			for (int64_t col : { (int64_t)0, rc_col_cycle(mc, 0, 0), rc_col_cycle(mc, 0, (uint32_t)mc - 1), rc_col_cycle(mc, 1, 0), rc_col_cycle(mc, 1, (uint32_t)mc - 1), rc_col_context(mc, 0),
			                     rc_col_context(mc, RC_NCTX - 1) }) {
				const int64_t w = rc_cell(mc, Q, col);
				CHECK(w >= 0 && w + 1 < words);
			}
		CHECK(rc_cell(mc, RC_NQ - 1, rc_col_context(mc, RC_NCTX - 1)) == words - 2);
		// a flush whose LDS holds a count in every cell: with max_cycle 1 only cycle 0 has a column, and nothing else may be formed
		std::vector<uint32_t> ctx((size_t)RC_LDS_CTX_WORDS, 1), cyc((size_t)RC_LDS_CYC_WORDS, 1), tag((size_t)RC_LDS_SLOTS, RC_SLOT_EMPTY);
		tag[0] = RC_NQ - 1; tag[3] = 0; tag[7] = 40;
		int64_t n_flushed = 0, highest = -1;
		for (int first = 0; first < 64; ++first)
			rc_flush(mc, first, 64, [&](int s) { return tag.at((size_t)s); }, [&](int i) { return ctx.at((size_t)i); }, [&](int i) { return cyc.at((size_t)i); },
			         [&](int64_t word, uint64_t n, uint64_t) { CHECK(word >= 0 && word + 1 < words && n > 0); ++n_flushed; if (word > highest) highest = word; });
		const int64_t cycles = mc < RC_LDS_CYCLES ? mc : RC_LDS_CYCLES;
		CHECK(n_flushed == RC_NQ * RC_NCTX + RC_NQ + 3 * 2 * cycles && highest == words - 2);
		// a base of the last cycle of the second mate, of a quality without a slot
		int64_t got = -1;
		std::vector<uint32_t> full((size_t)RC_LDS_SLOTS, 5);
		rc_count_base(mc, RC_NQ - 1, 1, (uint32_t)mc - 1, 16, true, [&](int s) { return full.at((size_t)s); }, [&](int s, uint32_t, uint32_t) { return full.at((size_t)s); },
		              [&](int cell, bool) { CHECK(cell == rc_lds_ctx_cell(RC_NQ - 1, 16)); }, [&](int, bool) { CHECK(!"no slot is free"); }, [&](int64_t word, bool) { got = word; });
		CHECK(got == rc_cell(mc, RC_NQ - 1, rc_col_cycle(mc, 1, (uint32_t)mc - 1)) && got + 1 < words);
	}
	if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
	printf("ok\n");
	return 0;
}
