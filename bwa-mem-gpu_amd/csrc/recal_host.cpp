// The base-quality recalibration table of a coordinate-sorted BAM file, the parts that need no device: a builder that is fed the records
// in any cut and any order, and the serialiser of the dense tables (one serialiser: the device stage, k_recal.hip, hands its own tables to it).  The
// rule is in include/bwahip.h.  The builder keeps the dense tables of recal_tables.h (16 bytes a cell, 3 MB at the default max_cycle, made
// at the first record that takes part) and copies of the packed reference and the mask.  A judge's twin and a library for small inputs: nothing falls back on it.
#include "recal_tables.h"
#include "sidecar_host.h"

int rc_resolve(const bwahip_recal_opt_t *in, bwahip_recal_opt_t *out)
{
	bwahip_recal_opt_t o = { 0, 0, RC_DEFAULT_EXCLUDE, RC_DEFAULT_CYCLE };
	if (in) {
		if (in->min_mapq < 0 || in->min_mapq > 255 || in->min_baseq < 0 || in->min_baseq > 93 || in->exclude_flags > 0xffff || in->max_cycle < 0 || in->max_cycle > RC_MAX_CYCLE) return BWAHIP_EINVAL;
		o.min_mapq = in->min_mapq; o.min_baseq = in->min_baseq;
		if (in->exclude_flags >= 0) o.exclude_flags = in->exclude_flags;
		if (in->max_cycle) o.max_cycle = in->max_cycle;
	}
	*out = o;
	return 0;
}

int rc_serialise(const RcTables &t, std::vector<uint8_t> *out)
{
	if (!out || t.n_ref < 0 || !t.tab || t.opt.max_cycle < 1 || t.opt.max_cycle > RC_MAX_CYCLE) return BWAHIP_EINVAL;
	const int mc = t.opt.max_cycle;
	const int64_t first[4] = { 0, 1, rc_col_context(mc, 0), rc_ncol(mc) };   // the tables' first columns
	uint64_t n_rows[3] = { 0, 0, 0 }, n_obs[3] = { 0, 0, 0 }, n_err[3] = { 0, 0, 0 };
	for (int k = 0; k < 3; ++k)
		for (uint32_t Q = 0; Q < RC_NQ; ++Q)
			for (int64_t col = first[k]; col < first[k + 1]; ++col) {
				const uint64_t *cell = t.tab + rc_cell(mc, Q, col);
				if (!cell[0] && cell[1]) return BWAHIP_EINVAL;            // not the tables of a walk
				n_rows[k] += cell[0] != 0; n_obs[k] += cell[0]; n_err[k] += cell[1];
			}
	if (n_obs[1] != n_obs[0] || n_obs[2] != n_obs[0] || n_err[1] != n_err[0] || n_err[2] != n_err[0]) return BWAHIP_EINVAL;
	std::vector<uint8_t> &o = *out;
	o.clear();
	o.reserve((size_t)(80 + 24 * (n_rows[0] + n_rows[1] + n_rows[2])));
	o.insert(o.end(), { 'B', 'R', 'C', 1 });
	put32(o, (uint32_t)t.n_ref);
	put32(o, (uint32_t)t.opt.min_mapq); put32(o, (uint32_t)t.opt.min_baseq); put32(o, (uint32_t)t.opt.exclude_flags); put32(o, (uint32_t)t.opt.max_cycle);
	put64(o, t.n_records); put64(o, n_obs[0]); put64(o, n_err[0]); put64(o, t.n_masked);
	for (int k = 0; k < 3; ++k) put64(o, n_rows[k]);
	for (int k = 0; k < 3; ++k)
		for (uint32_t Q = 0; Q < RC_NQ; ++Q)
			for (int64_t col = first[k]; col < first[k + 1]; ++col) {
				const uint64_t *cell = t.tab + rc_cell(mc, Q, col);
				if (!cell[0]) continue;
				const int64_t j = col - first[k];                         // the cycle table: the first mate's columns, then the second's
				put32(o, Q); put32(o, k == 1 ? (uint32_t)(j >= mc ? 1u << 31 | (uint32_t)(j - mc) : (uint32_t)j) : (uint32_t)j);
				put64(o, cell[0]); put64(o, cell[1]);
			}
	return 0;
}

struct bwahip_recal_builder : SidecarBuilder {
	bwahip_recal_opt_t opt = { 0, 0, RC_DEFAULT_EXCLUDE, RC_DEFAULT_CYCLE };
	bool with_mask = false;
	std::vector<uint8_t> mask;
	std::vector<uint64_t> tab;                                     // the dense tables, made at the first record that takes part
	uint64_t n_records = 0, n_masked = 0;
};

extern "C" int bwahip_recal_builder_open(int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const uint8_t *mask, const bwahip_recal_opt_t *opt, bwahip_recal_builder **out)
{
	if (!out) return BWAHIP_EINVAL;
	*out = nullptr;
	bwahip_recal_opt_t o;
	int64_t sum = 0;
	int rc;
	if ((rc = check_refs(n_ref, ref_len, &sum, PU_MAX_SUM)) || (rc = rc_resolve(opt, &o))) return rc;
	if (sum && !pac) return BWAHIP_EINVAL;
	bwahip_recal_builder *b = new bwahip_recal_builder;
	b->set_refs(n_ref, ref_len, sum ? pac : nullptr); b->opt = o;
	if (sum && mask) { b->mask.assign(mask, mask + (sum + 7) / 8); b->with_mask = true; }
	*out = b;
	return 0;
}

static int rc_builder_add_one(bwahip_recal_builder *b, const uint8_t *rec, int64_t len)
{
	PuRec r;
	if (!pu_parse(rec, len, b->n_ref, &r)) return BWAHIP_EINVAL;
	if (!rc_takes_part(r, b->opt)) return 0;
	if (r.l_seq > b->opt.max_cycle) return BWAHIP_ECAPACITY;
	const int mc = b->opt.max_cycle;
	if (b->tab.empty()) b->tab.assign((size_t)rc_table_words(mc), 0);
	uint64_t *tab = b->tab.data();
	++b->n_records;
	rc_walk(r, b->ref_len[(size_t)r.q.ref], b->ref_off[(size_t)r.q.ref], b->pac.data(), b->with_mask ? b->mask.data() : nullptr, b->opt.min_baseq,
	        [&](uint32_t Q, uint32_t mate, uint32_t c, uint32_t x, bool error) {
		        for (int64_t col : { (int64_t)0, rc_col_cycle(mc, mate, c), rc_col_context(mc, x) }) { uint64_t *cell = tab + rc_cell(mc, Q, col); ++cell[0]; cell[1] += error; }
	        },
	        [&]() { ++b->n_masked; });
	return 0;
}

extern "C" int bwahip_recal_builder_add_records(bwahip_recal_builder *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec)
{
	return builder_feed(b, rec, rec_off, n_rec, rc_builder_add_one);
}

static int rc_builder_bytes(bwahip_recal_builder *b, std::vector<uint8_t> *bytes)
{
	if (b->tab.empty()) b->tab.assign((size_t)rc_table_words(b->opt.max_cycle), 0);
	RcTables t;
	t.n_ref = b->n_ref; t.opt = b->opt; t.n_records = b->n_records; t.n_masked = b->n_masked; t.tab = b->tab.data();
	return rc_serialise(t, bytes);
}

extern "C" int bwahip_recal_builder_finish(bwahip_recal_builder *b, int rc_fd) { return builder_finish(b, rc_fd, "writing the recalibration table", rc_builder_bytes); }

extern "C" void bwahip_recal_builder_close(bwahip_recal_builder *b) { delete b; }

// what the device stage (k_recal.hip) holds: the dense tables, the mask, and 4 096 for the counters, the error word and the contig table's first entries
extern "C" int64_t bwahip_recal_hbm_need(int64_t sum_len, int max_cycle, int with_mask)
{
	if (sum_len < 0 || sum_len >= PU_MAX_SUM || max_cycle < 0 || max_cycle > RC_MAX_CYCLE) return -1;
	const int64_t work = 8 * rc_table_words(max_cycle ? max_cycle : RC_DEFAULT_CYCLE) + (with_mask ? (sum_len + 7) / 8 : 0) + 4096;
	return work + work / 8;
}
