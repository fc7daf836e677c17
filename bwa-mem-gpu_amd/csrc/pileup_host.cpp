// The pileup of candidate variant sites of a coordinate-sorted BAM file, the parts that need no device: a builder that is fed the records in
// any cut and any order, and the serialiser of the compact tables, which the device stage (k_pileup.hip) hands its own tables to.  The rule is
// in include/bwahip.h.  The builder keeps n_cov, n_ref_fwd and n_ref_rev for every base of a reference that a record has covered (12 bytes
// per base, made at the first such record), every observation as its 64-bit key, and a copy of the packed reference; finish() sorts the
// keys, and alleles, strand counts and sites are runs of the sorted keys.  A judge and a library for small inputs: nothing falls back on it.
#include "pileup_tables.h"
#include "sidecar_host.h"
#include <algorithm>

int pu_resolve(const bwahip_pileup_opt_t *in, bwahip_pileup_opt_t *out)
{
	bwahip_pileup_opt_t o = { 0, 0, 1796, 2 };
	if (in) {
		if (in->min_mapq < 0 || in->min_mapq > 255 || in->min_baseq < 0 || in->min_baseq > 93 || in->exclude_flags > 0xffff || in->min_alt < 0 || in->min_alt > 0xffff) return BWAHIP_EINVAL;
		o.min_mapq = in->min_mapq; o.min_baseq = in->min_baseq;
		if (in->exclude_flags >= 0) o.exclude_flags = in->exclude_flags;
		if (in->min_alt) o.min_alt = in->min_alt;
	}
	*out = o;
	return 0;
}

int pu_serialise(const PuTables &t, std::vector<uint8_t> *out)
{
	if (!out || t.n_ref < 0 || t.n_alleles < 0 || t.n_sites < 0 || (t.n_ref && !t.ref_len) || (t.n_alleles && !t.alleles) || (t.n_sites && !t.sites)) return BWAHIP_EINVAL;
	std::vector<uint8_t> &o = *out;
	o.clear();
	o.reserve((size_t)(64 + 28 * t.n_sites + 20 * t.n_alleles));
	o.insert(o.end(), { 'B', 'P', 'U', 1 });
	put32(o, (uint32_t)t.n_ref);
	put32(o, (uint32_t)t.opt.min_mapq); put32(o, (uint32_t)t.opt.min_baseq); put32(o, (uint32_t)t.opt.exclude_flags); put32(o, (uint32_t)t.opt.min_alt);
	put64(o, (uint64_t)t.n_sites); put64(o, (uint64_t)t.n_alleles);
	for (int k = 0; k < 3; ++k) put64(o, t.n_obs[k]);
	int32_t r = 0; int64_t r0 = 0;                                 // the contig of the site at hand, its first base: the sites ascend
	for (int64_t s = 0; s < t.n_sites; ++s) {
		const PuSite &x = t.sites[s];
		while (r < t.n_ref && (int64_t)x.gpos >= r0 + t.ref_len[r]) r0 += t.ref_len[r++];
		const int64_t next = s + 1 < t.n_sites ? t.sites[s + 1].first : t.n_alleles;
		if (r >= t.n_ref || (int64_t)x.gpos < r0 || next <= x.first || next > t.n_alleles) return BWAHIP_EINVAL;   // not the tables of a pileup
		put32(o, (uint32_t)r); put32(o, (uint32_t)((int64_t)x.gpos - r0)); put32(o, x.ref_base); put32(o, (uint32_t)(next - x.first));
		put32(o, x.n_cov); put32(o, x.n_ref_fwd); put32(o, x.n_ref_rev);
	}
	for (int64_t a = 0; a < t.n_alleles; ++a) {
		const PuAllele &x = t.alleles[a];
		put32(o, x.kind); put32(o, x.len); put32(o, x.bases); put32(o, x.fwd); put32(o, x.rev);
	}
	return 0;
}

struct bwahip_pileup_builder : SidecarBuilder {
	bwahip_pileup_opt_t opt = { 0, 0, 1796, 2 };
	std::vector<std::vector<uint32_t>> ev;                         // per reference 3 words per base (n_cov, n_ref_fwd, n_ref_rev), empty until a record covers it
	std::vector<uint64_t> keys;                                    // the observations
};

extern "C" int bwahip_pileup_builder_open(int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const bwahip_pileup_opt_t *opt, bwahip_pileup_builder **out)
{
	if (!out) return BWAHIP_EINVAL;
	*out = nullptr;
	bwahip_pileup_opt_t o;
	int64_t sum = 0;
	int rc;
	if ((rc = check_refs(n_ref, ref_len, &sum, PU_MAX_SUM)) || (rc = pu_resolve(opt, &o))) return rc;
	if (sum && !pac) return BWAHIP_EINVAL;
	bwahip_pileup_builder *b = new bwahip_pileup_builder;
	b->set_refs(n_ref, ref_len, sum ? pac : nullptr); b->opt = o;
	b->ev.resize((size_t)n_ref);
	*out = b;
	return 0;
}

static int pu_builder_add_one(bwahip_pileup_builder *b, const uint8_t *rec, int64_t len)
{
	PuRec r;
	if (!pu_parse(rec, len, b->n_ref, &r)) return BWAHIP_EINVAL;
	if (!pu_takes_part(r, b->opt)) return 0;
	const int64_t L = b->ref_len[(size_t)r.q.ref], g0 = b->ref_off[(size_t)r.q.ref];
	std::vector<uint32_t> &e = b->ev[(size_t)r.q.ref];
	const uint32_t strand = r.q.flag >> 4 & 1;
	bool full = false;
	pu_walk(r, L, g0, b->pac.data(), b->opt.min_baseq,
	        [&](int64_t p) { if (e.empty()) e.assign(3 * (size_t)L, 0); ++e[3 * (size_t)p]; },
	        [&](int64_t p) { ++e[3 * (size_t)p + 1 + strand]; },
	        [&](int64_t p, int kind, uint32_t allele) { if ((int64_t)b->keys.size() >= PU_MAX_OBS) full = true; else b->keys.push_back(pu_key(g0 + p, kind, allele, strand)); });
	return full ? BWAHIP_ECAPACITY : 0;
}

extern "C" int bwahip_pileup_builder_add_records(bwahip_pileup_builder *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec)
{
	return builder_feed(b, rec, rec_off, n_rec, pu_builder_add_one);
}

static int pu_builder_bytes(bwahip_pileup_builder *b, std::vector<uint8_t> *bytes)
{
	std::vector<uint64_t> &k = b->keys;
	std::sort(k.begin(), k.end());
	PuTables t;
	t.n_ref = b->n_ref; t.ref_len = b->ref_len.data(); t.opt = b->opt;
	std::vector<PuAllele> alleles;
	std::vector<PuSite> sites;
	int32_t r = 0;
	for (size_t i = 0; i < k.size();) {
		size_t j = i, n_rev = 0;
		for (; j < k.size() && k[j] >> 1 == k[i] >> 1; ++j) n_rev += k[j] & 1;
		PuAllele a;
		int64_t g;
		pu_unkey(k[i], &g, &a.kind, &a.len, &a.bases);
		t.n_obs[a.kind] += j - i;
		a.gpos = (uint64_t)g; a.fwd = (uint32_t)(j - i - n_rev); a.rev = (uint32_t)n_rev; a.pad = 0;
		if (j - i >= (size_t)b->opt.min_alt) {
			if (sites.empty() || sites.back().gpos != a.gpos) {
				while (g >= b->ref_off[(size_t)r + 1]) ++r;             // an observation lies inside a contig
				static const uint32_t none[3] = { 0, 0, 0 };              // an insertion's site may lie on a reference no record covers
				const uint32_t *e = b->ev[(size_t)r].empty() ? none : b->ev[(size_t)r].data() + 3 * (size_t)(g - b->ref_off[(size_t)r]);
				sites.push_back(PuSite{ a.gpos, pu_ref2(b->pac.data(), g), (uint32_t)alleles.size(), e[0], e[1], e[2], 0 });
			}
			alleles.push_back(a);
		}
		i = j;
	}
	t.n_alleles = (int64_t)alleles.size(); t.alleles = alleles.data(); t.n_sites = (int64_t)sites.size(); t.sites = sites.data();
	return pu_serialise(t, bytes);
}

extern "C" int bwahip_pileup_builder_finish(bwahip_pileup_builder *b, int pu_fd) { return builder_finish(b, pu_fd, "writing the pileup", pu_builder_bytes); }

extern "C" void bwahip_pileup_builder_close(bwahip_pileup_builder *b) { delete b; }

extern "C" int64_t bwahip_pileup_hbm_need(int64_t n_records)
{
	if (n_records < 0) return -1;
	const int64_t work = 12 * n_records + 4096;
	return work + work / 8;
}
