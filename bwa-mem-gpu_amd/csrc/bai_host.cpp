// The BAI index beside a coordinate-sorted BAM file, the parts that need no device: a builder that is fed the records and the lengths
// of the BGZF members as a writer produces them, and the serialiser of the compact tables, which the device stage (k_bai.hip) hands its
// own tables to.  The canonical form: a chunk is a maximal run of consecutive records of one (refID, bin); the chunks
// of a bin are in file order and a chunk that begins in the member in which its predecessor ends is joined to it; bins ascending, then
// the pseudo-bin 37450; the linear index holds the smallest begin over the records that overlap a window, an empty window the value of
// the next one to its right.  No relocation of sparse bins into their parents.
#include "../../include/bwahip.h"
#include "bai_tables.h"
#include "sidecar_host.h"
#include <algorithm>
#include <deque>

int bai_serialise(const BaiTables &t, std::vector<uint8_t> *out)
{
	if (!out || t.n_ref < 0 || t.n_chunks < 0 || (t.n_ref && (!t.meta || !t.lin_off)) || (t.n_chunks && (!t.ckey || !t.cbeg || !t.cend))) return BWAHIP_EINVAL;
	std::vector<uint8_t> &o = *out;
	o.clear();
	o.reserve(16 + 48 * (size_t)t.n_ref + 24 * (size_t)t.n_chunks + (t.n_ref ? 8 * (size_t)t.lin_off[t.n_ref] : 0));   // a bound: every chunk with a bin header of its own
	o.insert(o.end(), { 'B', 'A', 'I', 1 });
	put32(o, (uint32_t)t.n_ref);
	int64_t k = 0;
	for (int32_t r = 0; r < t.n_ref; ++r) {
		const uint64_t *m = t.meta + 4 * (size_t)r;
		const int64_t n_intv = t.lin_off[r + 1] - t.lin_off[r];
		int64_t k1 = k;
		uint32_t n_bin = 0;
		while (k1 < t.n_chunks && (int64_t)(t.ckey[k1] >> 16) == r) { if (k1 == k || t.ckey[k1] != t.ckey[k1 - 1]) ++n_bin; ++k1; }
		const bool has = m[2] + m[3] != 0;
		if (has != (k1 > k) || has != (n_intv > 0) || n_intv < 0 || (n_intv && !t.lin)) return BWAHIP_EINVAL;
		put32(o, has ? n_bin + 1 : 0);
		while (k < k1) {
			int64_t e = k;
			while (e < k1 && t.ckey[e] == t.ckey[k]) ++e;
			put32(o, (uint32_t)(t.ckey[k] & 0xffff)); put32(o, (uint32_t)(e - k));
			for (; k < e; ++k) { put64(o, t.cbeg[k]); put64(o, t.cend[k]); }
		}
		if (has) { put32(o, BAI_META_BIN); put32(o, 2); for (int j = 0; j < 4; ++j) put64(o, m[j]); }
		put32(o, (uint32_t)n_intv);
		for (int64_t w = 0; w < n_intv; ++w) put64(o, t.lin[t.lin_off[r] + w]);
	}
	if (k != t.n_chunks) return BWAHIP_EINVAL;                     // chunks of a reference that does not exist, or out of order
	put64(o, t.n_no_coor);
	return 0;
}

// ---- builder ------------------------------------------------------------------------------------------------------------------------
// Records and member lengths arrive in file order, interleaved in any proportion.  A record waits (ten words) until the member that
// holds its begin and the one that holds the begin of its successor are known; the last record ends at V(total), known at finish.  What
// is kept beyond that tail: one entry per run of records of one (refID, bin), a word per 16 Kbp window reached, four words per reference,
// and the offsets of the members no resolved record needs any more are dropped.
struct bwahip_bai_builder : SidecarBuilder {                      // (of its contigs it keeps the count alone)
	int64_t base = 0;
	int64_t u = 0; bool have_prev = false; uint64_t prev_key = 0;
	std::deque<int64_t> coff{ 0 }; int64_t coff_first = 0, n_members = 0;   // coff[b - coff_first] = offset of member b, up to b = n_members
	struct Pend { BaiRec r; int64_t u0; };
	std::deque<Pend> pend;
	struct Chunk { uint64_t key, beg, end; };
	std::vector<Chunk> chunks; bool run_open = false; Chunk run = { 0, 0, 0 };
	std::vector<uint64_t> meta; std::vector<std::vector<uint64_t>> lin;
	uint64_t n_no_coor = 0;

	bool known(int64_t blk) const { return blk <= n_members; }
	uint64_t voff(int64_t at) const { return (uint64_t)(base + coff[(size_t)(at / BAI_BLOCK_IN - coff_first)]) << 16 | (uint64_t)(at % BAI_BLOCK_IN); }
	void close_run() { if (run_open) chunks.push_back(run); run_open = false; }
	void emit(const BaiRec &r, uint64_t vb, uint64_t ve)
	{
		if (r.ref < 0) { ++n_no_coor; close_run(); return; }
		const uint64_t key = (uint64_t)r.ref << 16 | r.bin;
		if (run_open && run.key == key) run.end = ve;
		else { close_run(); run = { key, vb, ve }; run_open = true; }
		uint64_t *m = meta.data() + 4 * (size_t)r.ref;
		if (m[2] + m[3] == 0) m[0] = vb;
		m[1] = ve; ++m[r.unm ? 3 : 2];
		std::vector<uint64_t> &L = lin[(size_t)r.ref];
		const size_t w1 = (size_t)((r.e - 1) >> 14);
		if (L.size() <= w1) L.resize(w1 + 1, ~0ull);
		for (size_t w = (size_t)(r.pos >> 14); w <= w1; ++w) if (vb < L[w]) L[w] = vb;
	}
	void drain()
	{
		while (pend.size() >= 2 && known(pend[1].u0 / BAI_BLOCK_IN)) {
			emit(pend[0].r, voff(pend[0].u0), voff(pend[1].u0));
			pend.pop_front();
			const int64_t need = pend[0].u0 / BAI_BLOCK_IN;            // nothing before the member of the oldest waiting begin is asked for again
			while (coff_first < need && coff.size() > 1) { coff.pop_front(); ++coff_first; }
		}
	}
};

extern "C" int bwahip_bai_builder_open(int32_t n_ref, int64_t first_member_offset, bwahip_bai_builder **out)
{
	if (!out) return BWAHIP_EINVAL;
	*out = nullptr;
	if (n_ref < 0 || first_member_offset < 0 || first_member_offset >= (1ll << 48)) return BWAHIP_EINVAL;
	bwahip_bai_builder *b = new bwahip_bai_builder;
	b->n_ref = n_ref; b->base = first_member_offset;
	b->meta.assign(4 * (size_t)n_ref, 0); b->lin.resize((size_t)n_ref);
	*out = b;
	return 0;
}

extern "C" int bwahip_bai_builder_add_records(bwahip_bai_builder *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec)
{
	if (!b || n_rec < 0 || (n_rec && (!rec || !rec_off)) || b->finished) return BWAHIP_EINVAL;
	if (b->err) return b->err;
	for (int64_t i = 0; i < n_rec; ++i) {
		const int64_t len = rec_off[i + 1] - rec_off[i];
		bwahip_bai_builder::Pend p;
		int bad = rec_off[i] < 0 || len < 0 ? BAI_BAD : bai_parse(rec + rec_off[i], len, b->n_ref, &p.r);
		if (bad != BAI_BAD) {                                       // the order is judged before the capacity: both fields were read within the record
			const int32_t ref = (int32_t)bam_ld32(rec + rec_off[i] + 4), pos = (int32_t)bam_ld32(rec + rec_off[i] + 8);
			const uint64_t key = bai_order_key(ref, pos);
			if (b->have_prev && key < b->prev_key) bad = BAI_BAD;
			b->prev_key = key; b->have_prev = true;
		}
		if (bad) return b->err = bad == BAI_BAD ? BWAHIP_EINVAL : BWAHIP_ECAPACITY;
		p.u0 = b->u; b->u += len;
		b->pend.push_back(p);
	}
	b->drain();
	return 0;
}

extern "C" int bwahip_bai_builder_add_members(bwahip_bai_builder *b, const int32_t *member_len, int64_t n)
{
	if (!b || n < 0 || (n && !member_len) || b->finished) return BWAHIP_EINVAL;
	if (b->err) return b->err;
	for (int64_t i = 0; i < n; ++i) {
		if (member_len[i] < 1 || member_len[i] > 65536) return b->err = BWAHIP_EINVAL;
		b->coff.push_back(b->coff.back() + member_len[i]); ++b->n_members;
	}
	if (b->base + b->coff.back() >= (1ll << 48)) return b->err = BWAHIP_ECAPACITY;   // a virtual offset has 48 bits for the file offset
	b->drain();
	return 0;
}

static int bai_builder_bytes(bwahip_bai_builder *b, std::vector<uint8_t> *bytes)
{
	if (b->n_members != (b->u + BAI_BLOCK_IN - 1) / BAI_BLOCK_IN) return BWAHIP_EINVAL;   // the members are not those of these records
	b->drain();
	if (b->pend.size() > 1) return BWAHIP_EINTERNAL;
	if (!b->pend.empty()) { b->emit(b->pend[0].r, b->voff(b->pend[0].u0), (uint64_t)(b->base + b->coff.back()) << 16); b->pend.clear(); }
	b->close_run();
	std::vector<bwahip_bai_builder::Chunk> &c = b->chunks;
	std::stable_sort(c.begin(), c.end(), [](const bwahip_bai_builder::Chunk &x, const bwahip_bai_builder::Chunk &y) { return x.key < y.key; });
	std::vector<uint64_t> ckey, cbeg, cend;
	for (const auto &x : c) {
		if (!ckey.empty() && ckey.back() == x.key && x.beg >> 16 <= cend.back() >> 16) cend.back() = x.end;
		else { ckey.push_back(x.key); cbeg.push_back(x.beg); cend.push_back(x.end); }
	}
	std::vector<int64_t> lin_off((size_t)b->n_ref + 1, 0);
	for (int32_t r = 0; r < b->n_ref; ++r) lin_off[(size_t)r + 1] = lin_off[(size_t)r] + (int64_t)b->lin[(size_t)r].size();
	std::vector<uint64_t> lin((size_t)lin_off[(size_t)b->n_ref]);
	for (int32_t r = 0; r < b->n_ref; ++r) {
		const std::vector<uint64_t> &L = b->lin[(size_t)r];
		uint64_t right = ~0ull;                                      // the last window holds the record that made it
		for (size_t w = L.size(); w-- > 0;) { if (L[w] != ~0ull) right = L[w]; lin[(size_t)lin_off[(size_t)r] + w] = right; }
	}
	BaiTables t;
	t.n_ref = b->n_ref; t.n_chunks = (int64_t)ckey.size(); t.ckey = ckey.data(); t.cbeg = cbeg.data(); t.cend = cend.data();
	t.meta = b->meta.data(); t.lin_off = lin_off.data(); t.lin = lin.data(); t.n_no_coor = b->n_no_coor;
	return bai_serialise(t, bytes);
}

extern "C" int bwahip_bai_builder_finish(bwahip_bai_builder *b, int bai_fd) { return builder_finish(b, bai_fd, "writing the BAI index", bai_builder_bytes); }

extern "C" void bwahip_bai_builder_close(bwahip_bai_builder *b) { delete b; }

// the host merger's finish with the index: the builder listens to the merge
extern "C" int bwahip_bam_merger_finish_bai(bwahip_bam_merger *m, int fd, int level, int n_threads, bwahip_bai_builder *builder)
{
	if (!builder) return BWAHIP_EINVAL;
	MergeHooks h;
	h.record = [](void *b, const uint8_t *rec, int64_t len) { const int64_t one[2] = { 0, len }; return bwahip_bai_builder_add_records((bwahip_bai_builder*)b, rec, one, 1); };
	h.members = [](void *b, const int32_t *ml, int64_t n) { return bwahip_bai_builder_add_members((bwahip_bai_builder*)b, ml, n); };
	h.arg = builder;
	return bam_merger_finish_hooks(m, fd, level, n_threads, &h);
}

// the stream entry points refuse an index that BAI cannot hold before anything starts
extern "C" int bwahip_bai_check_contigs(const bwahip_bns_t *bns)
{
	if (!bns || bns->n_seqs < 0 || (bns->n_seqs && !bns->anns)) return BWAHIP_EINVAL;
	for (int32_t i = 0; i < bns->n_seqs; ++i) if (bns->anns[i].len > BAI_MAX_END) return BWAHIP_ECAPACITY;
	return 0;
}
