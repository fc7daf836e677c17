// The QC summary of a coordinate-sorted BAM file, the parts that need no device: a builder that is fed the records in any cut and any
// order, and the serialiser of the compact tables, which the device stage (k_qc.hip) hands its own tables to.  The rule is in
// include/bwahip.h.  The builder keeps a difference array per reference that a record has covered (4 bytes per base), made at the first
// such record; finish() turns each into depths by one prefix sum.
#include "qc_tables.h"
#include "sidecar_host.h"

int qc_resolve(const bwahip_qc_opt_t *in, bwahip_qc_opt_t *out)
{
	bwahip_qc_opt_t o = { 14, 1796, 0 };
	if (in) {
		if (in->window_shift != 0 && (in->window_shift < 4 || in->window_shift > 29)) return BWAHIP_EINVAL;
		if (in->exclude_flags > 0xffff || in->min_mapq < 0 || in->min_mapq > 255) return BWAHIP_EINVAL;
		if (in->window_shift) o.window_shift = in->window_shift;
		if (in->exclude_flags >= 0) o.exclude_flags = in->exclude_flags;
		o.min_mapq = in->min_mapq;
	}
	*out = o;
	return 0;
}

int qc_serialise(const QcTables &t, std::vector<uint8_t> *out)
{
	if (!out || t.n_ref < 0 || !t.fixed || (t.n_ref && (!t.ref_len || !t.per_ref))) return BWAHIP_EINVAL;
	int64_t n_win = 0;
	for (int32_t r = 0; r < t.n_ref; ++r) n_win += qc_windows(t.ref_len[r], t.opt.window_shift);
	if (n_win && !t.win) return BWAHIP_EINVAL;
	std::vector<uint8_t> &o = *out;
	o.clear();
	o.reserve((size_t)qc_file_bytes(t.n_ref, n_win));
	o.insert(o.end(), { 'B', 'Q', 'C', 1 });
	put32(o, (uint32_t)t.n_ref);
	put32(o, (uint32_t)t.opt.window_shift); put32(o, (uint32_t)t.opt.exclude_flags); put32(o, (uint32_t)t.opt.min_mapq);
	for (int k = 0; k < QC_FIXED; ++k) put64(o, t.fixed[k]);          // n_no_coor, the counts and the histograms are in the file's order
	int64_t w0 = 0;
	for (int32_t r = 0; r < t.n_ref; ++r) {
		const int64_t nw = qc_windows(t.ref_len[r], t.opt.window_shift);
		uint64_t depth_sum = 0;
		for (int64_t w = 0; w < nw; ++w) depth_sum += t.win[w0 + w];
		const uint64_t *p = t.per_ref + QC_PER_REF * (size_t)r;
		put64(o, (uint64_t)t.ref_len[r]); put64(o, p[0]); put64(o, p[1]); put64(o, p[2]); put64(o, depth_sum); put64(o, (uint64_t)nw);
		w0 += nw;
	}
	for (int64_t w = 0; w < n_win; ++w) put64(o, t.win[w]);
	return (int64_t)o.size() == qc_file_bytes(t.n_ref, n_win) ? 0 : BWAHIP_EINTERNAL;   // (what the stream driver reports after a fall-back)
}

struct bwahip_qc_builder : SidecarBuilder {
	bwahip_qc_opt_t opt = { 14, 1796, 0 };
	std::vector<uint64_t> fixed, per_ref;
	std::vector<std::vector<int32_t>> diff;                        // per reference len + 1 words, empty until a record covers it
};

extern "C" int bwahip_qc_builder_open(int32_t n_ref, const int64_t *ref_len, const bwahip_qc_opt_t *opt, bwahip_qc_builder **out)
{
	if (!out) return BWAHIP_EINVAL;
	*out = nullptr;
	bwahip_qc_opt_t o;
	int rc;
	if ((rc = check_refs(n_ref, ref_len, nullptr, NO_SUM_CAP)) || (rc = qc_resolve(opt, &o))) return rc;
	bwahip_qc_builder *b = new bwahip_qc_builder;
	b->set_refs(n_ref, ref_len, nullptr); b->opt = o;
	b->fixed.assign(QC_FIXED, 0); b->per_ref.assign(QC_PER_REF * (size_t)n_ref, 0); b->diff.resize((size_t)n_ref);
	*out = b;
	return 0;
}

static int qc_builder_add_one(bwahip_qc_builder *b, const uint8_t *rec, int64_t len)
{
	QcRec r;
	if (!qc_parse(rec, len, b->n_ref, &r)) return BWAHIP_EINVAL;
	uint64_t *f = b->fixed.data();
	const uint32_t cat = qc_categories(r);
	uint64_t *cnt = f + QC_COUNT + ((r.flag & 0x200) ? 16 : 0);
	for (int k = 0; k < 16; ++k) cnt[k] += cat >> k & 1;
	if (qc_in_mapq_hist(r)) ++f[QC_MAPQ + r.mapq];
	if (qc_in_isize_hist(r)) ++f[QC_ISIZE + (r.tlen < 1024 ? r.tlen : 1024)];
	if (r.ref < 0) { ++f[QC_NO_COOR]; return 0; }
	++b->per_ref[QC_PER_REF * (size_t)r.ref + ((r.flag & 0x4) ? 1 : 0)];
	if (!qc_covers(r, b->opt)) return 0;
	const int64_t L = b->ref_len[(size_t)r.ref];
	std::vector<int32_t> &d = b->diff[(size_t)r.ref];
	qc_intervals(r, L, [&](int64_t a, int64_t e) {
		if (d.empty()) d.assign((size_t)L + 1, 0);
		++d[(size_t)a]; --d[(size_t)e];
	});
	return 0;
}

extern "C" int bwahip_qc_builder_add_records(bwahip_qc_builder *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec)
{
	return builder_feed(b, rec, rec_off, n_rec, qc_builder_add_one);
}

static int qc_builder_bytes(bwahip_qc_builder *b, std::vector<uint8_t> *bytes)
{
	const int ws = b->opt.window_shift;
	std::vector<uint64_t> win;
	uint64_t *hist = b->fixed.data() + QC_DEPTH;
	for (int32_t r = 0; r < b->n_ref; ++r) {
		const int64_t L = b->ref_len[(size_t)r];
		const size_t w0 = win.size();
		win.resize(w0 + (size_t)qc_windows(L, ws), 0);
		const std::vector<int32_t> &d = b->diff[(size_t)r];
		if (d.empty()) { hist[0] += (uint64_t)L; continue; }
		int64_t depth = 0; uint64_t covered = 0;
		for (int64_t x = 0; x < L; ++x) {
			depth += d[(size_t)x];
			++hist[depth < 255 ? depth : 255];
			covered += depth > 0;
			win[w0 + (size_t)(x >> ws)] += (uint64_t)depth;
		}
		b->per_ref[QC_PER_REF * (size_t)r + 2] = covered;
	}
	QcTables t;
	t.n_ref = b->n_ref; t.ref_len = b->ref_len.data(); t.opt = b->opt; t.fixed = b->fixed.data(); t.per_ref = b->per_ref.data(); t.win = win.data();
	return qc_serialise(t, bytes);
}

extern "C" int bwahip_qc_builder_finish(bwahip_qc_builder *b, int qc_fd) { return builder_finish(b, qc_fd, "writing the QC summary", qc_builder_bytes); }

extern "C" void bwahip_qc_builder_close(bwahip_qc_builder *b) { delete b; }

extern "C" int64_t bwahip_qc_hbm_need(int64_t n_ref, int64_t sum_len, int64_t n_windows, int64_t n_records)
{
	if (n_ref < 0 || sum_len < 0 || n_windows < 0 || n_records < 0) return -1;
	const int64_t slots = sum_len + QC_TILE * n_ref;
	const int64_t work = 4 * slots + 16 * (slots / QC_TILE + n_ref + 1) + 8 * (QC_FIXED + QC_PER_REF * n_ref + n_windows) + 24 * (n_ref + 1) + 4096;
	return work + work / 8;
}
