// K9j -- the base-quality recalibration table of the device-merged, coordinate-sorted BAM file, where the runs lie.  The rule
// is in include/bwahip.h; how a record is read and judged is pileup_tables.h, a base's covariates, the dense tables and everything about
// the private counting -- the LDS cells, the claim of a slot, the flush -- are recal_tables.h, shared with the host builder and with the
// CPU program that plays a workgroup (tests/recal_slots_check.cpp).  All on the context's stream:
//
//   clear          the dense tables (rc_table_words(max_cycle) 64-bit words), the two counters, the error word;
//   records        k_rc_count, one workgroup per share of RC_SHARE consecutive records of a run, 16 lanes per record, sixteen records at
//                  a time: pu_parse (every field bounded by the record's length); the first offending record through one 64-bit atomicMin
//                  (malformed, or taking part with more bases than max_cycle: it is not walked); the walk of the CIGAR in the shape of
//                  pu_walk16 (k_pileup.hip) -- the group's lanes on 16 consecutive bases of an M = X operation, four times 16 a round, a
//                  lane's loads of a round independent of each other: the base's nibble byte, its quality byte, the byte of the base read
//                  one cycle earlier, the aligned 32-bit words of the packed reference and of the mask that hold its position.  A
//                  counted base goes through rc_count_base: the context table and the early cycles of a few qualities in 32-bit cells of
//                  the workgroup's LDS, anything else one 64-bit atomicAdd (two for an error) on the dense tables.  Then the flush,
//                  rc_flush: one 64-bit atomicAdd per non-zero cell, the quality column as the context table's row sums.  The records
//                  that took part by a ballot per sixteen records, the masked bases by a sum over the wavefront: one atomic each per
//                  wavefront;
//   one download   of the dense tables and the counters, awaited once; they go through rc_serialise (recal_host.cpp), the host builder's.
//
// Sums and a minimum of integers: the result does not depend on the order in which wavefronts run.  No thread leaves k_rc_count before its
// last barrier: a lane whose record lies behind the run's end stays and adds nothing.  The __shared__ arrays are indexed as arrays inside
// the kernel that declares them; every offset into them and into the dense tables comes from recal_tables.h.  45.6 KB of LDS a workgroup:
// three workgroups share a compute unit.
#include "ctx_internal.h"
#include "recal_tables.h"
#include "sidecar_host.h"

namespace {

constexpr int RC_ROUND = 4;                                      // a lane takes this many bases, 16 apart, before it counts them (PU_ROUND of k_pileup.hip)
enum { RC_T_RECORDS = 0, RC_T_MASKED = 1, RC_T_ERR = 2, RC_T_WORDS = 4 };   // the stage's counters; the error word: ordinal << 8 | RC_BAD_*
enum { RC_BAD_RECORD = 1, RC_BAD_LENGTH = 2 };

// the reference base at position g among all contigs' bases, out of the aligned word that holds it (pu_ref2_word of k_pileup.hip)
__device__ __forceinline__ uint32_t rc_ref2_word(const uint8_t *pac, int64_t pac_bytes, int64_t g)
{
	const int64_t byte = g >> 2;
	if (pac_bytes < 4) return pac[byte] >> ((~g & 3) << 1) & 3;    // (the same in every lane: a reference of a dozen bases)
	int64_t at = byte & ~3ll;
	if (at > pac_bytes - 4) at = pac_bytes - 4;
	uint32_t v;
	__builtin_memcpy(&v, pac + at, 4);
	return v >> ((int)(byte - at) * 8 + (int)((~g & 3) << 1)) & 3;
}

// the mask's bit of position g, in the same manner: the last four bytes where the word would end behind the bitmap; no mask: 0
__device__ __forceinline__ uint32_t rc_mask_word(const uint8_t *mask, int64_t mask_bytes, int64_t g)
{
	if (!mask) return 0;                                           // (the same in every lane)
	const int64_t byte = g >> 3;
	if (mask_bytes < 4) return mask[byte] >> (g & 7) & 1;
	int64_t at = byte & ~3ll;
	if (at > mask_bytes - 4) at = mask_bytes - 4;
	uint32_t v;
	__builtin_memcpy(&v, mask + at, 4);
	return v >> ((int)(byte - at) * 8 + (int)(g & 7)) & 1;
}

// The walk of rc_walk (recal_tables.h) by a group of 16 lanes, l the lane in its group: count(Q, mate, cycle, context, error) for every
// counted base of this lane; returns the bases of this lane that the mask alone keeps out.  r takes part and has at most max_cycle bases
template <class Count> __device__ __forceinline__ uint32_t rc_walk16(const PuRec &r, int64_t L, int64_t g0, const uint8_t *pac, int64_t pac_bytes, const uint8_t *mask, int64_t mask_bytes,
                                                                     int min_baseq, int l, Count count)
{
	const bool rev = (r.q.flag & 0x10) != 0;
	const uint32_t mate = r.q.flag >> 7 & 1;
	int64_t p = r.q.pos, q = 0;
	uint32_t n_masked = 0;
	for (int32_t k = 0; k < r.q.n_cigar; ++k) {
		const uint32_t w = bam_ld32(r.q.cig + 4 * k), op = w & 15;
		const int64_t n = w >> 4;
		if (pu_is_match(op)) {
			const int64_t m = L - p < n ? (L - p > 0 ? L - p : 0) : n;   // the bases inside the contig
			for (int64_t j0 = 0; j0 < m; j0 += 16 * RC_ROUND) {
				bool ok[RC_ROUND];
				uint32_t code[RC_ROUND], prev[RC_ROUND], b[RC_ROUND], rb[RC_ROUND], mk[RC_ROUND], cyc[RC_ROUND];
#pragma unroll
				for (int u = 0; u < RC_ROUND; ++u) {
					const int64_t j = j0 + 16 * u + l, jj = j < m ? j : j0, qi = q + jj;   // behind the operation's end: a base of it again, and not counted
					cyc[u] = rc_cycle(rev, r.l_seq, qi);
					code[u] = pu_base(r.seq, qi);                            // the loads whatever the others say: nothing waits for a branch
					prev[u] = pu_base(r.seq, cyc[u] ? rc_prev_index(rev, qi) : qi);   // cycle > 0: inside the read
					b[u] = r.qual[qi];
					rb[u] = rc_ref2_word(pac, pac_bytes, g0 + p + jj);
					mk[u] = rc_mask_word(mask, mask_bytes, g0 + p + jj);
					ok[u] = j < m;
				}
#pragma unroll
				for (int u = 0; u < RC_ROUND; ++u) {
					const int c2 = pu_code2(code[u]);
					if (!ok[u] || c2 < 0 || b[u] < (uint32_t)min_baseq) continue;
					if (mk[u]) { ++n_masked; continue; }
					count(rc_quality(b[u]), mate, cyc[u], rc_context(rev, cyc[u], c2, pu_code2(prev[u])), (uint32_t)c2 != rb[u]);
				}
			}
			p += n; q += n;
		} else if (op == 2 || op == 3) p += n;
		else if (op == 1 || op == 4) q += n;
	}
	return n_masked;
}

// tab: the dense tables; cnt: RC_T_WORDS counters.  Workgroup b counts the records [b * RC_SHARE, (b + 1) * RC_SHARE) of the run
__global__ __launch_bounds__(256) void k_rc_count(const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0, int n_ref, const int64_t *ref_len, const int64_t *ref_off,
                                                  const uint8_t *pac, int64_t pac_bytes, const uint8_t *mask, int64_t mask_bytes, bwahip_recal_opt_t opt, unsigned long long *tab,
                                                  unsigned long long *cnt)
{
	__shared__ uint32_t s_ctx[RC_LDS_CTX_WORDS], s_cyc[RC_LDS_CYC_WORDS], s_tag[RC_LDS_SLOTS];
	const int t = threadIdx.x, lane = t & 63, l = t & 15;
	for (int k = t; k < RC_LDS_CYC_WORDS; k += 256) s_cyc[k] = 0;
	for (int k = t; k < RC_LDS_CTX_WORDS; k += 256) s_ctx[k] = 0;
	if (t < RC_LDS_SLOTS) s_tag[t] = RC_SLOT_EMPTY;
	__syncthreads();
	const int mc = opt.max_cycle;
	auto tag = [&](int s) { return __hip_atomic_load(&s_tag[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
	auto cas = [&](int s, uint32_t expected, uint32_t desired) { return atomicCAS(&s_tag[s], expected, desired); };
	auto count = [&](uint32_t Q, uint32_t mate, uint32_t c, uint32_t x, bool error) {
		rc_count_base(mc, Q, mate, c, x, error, tag, cas,
		              [&](int cell, bool e) { atomicAdd(&s_ctx[cell], 1u); if (e) atomicAdd(&s_ctx[cell + 1], 1u); },
		              [&](int cell, bool e) { atomicAdd(&s_cyc[cell], 1u); if (e) atomicAdd(&s_cyc[cell + 1], 1u); },
		              [&](int64_t word, bool e) { atomicAdd(&tab[word], 1ull); if (e) atomicAdd(&tab[word + 1], 1ull); });
	};
	uint32_t n_took = 0, n_masked = 0;                              // n_took: the same in every lane of the wavefront
	for (int it = 0; it < RC_SHARE / 16; ++it) {                    // every lane takes every turn
		const int64_t i = (int64_t)blockIdx.x * RC_SHARE + it * 16 + (t >> 4);
		bool took = false;
		if (i < n_rec) {
			PuRec r;
			const int64_t o = off[i], e = off[i + 1];
			const bool live = o >= 0 && e >= o && e <= len && pu_parse(rec + o, e - o, n_ref, &r);
			if (!live) { if (l == 0) atomicMin(&cnt[RC_T_ERR], (unsigned long long)(ord0 + i) << 8 | RC_BAD_RECORD); }   // the first offending record decides
			else if (rc_takes_part(r, opt)) {
				if (r.l_seq > mc) { if (l == 0) atomicMin(&cnt[RC_T_ERR], (unsigned long long)(ord0 + i) << 8 | RC_BAD_LENGTH); }   // not walked: its cycles have no column
				else {
					took = true;
					n_masked += rc_walk16(r, ref_len[r.q.ref], ref_off[r.q.ref], pac, pac_bytes, mask, mask_bytes, opt.min_baseq, l, count);
				}
			}
		}
		n_took += (uint32_t)__popcll(__ballot(took && l == 0));
	}
	__syncthreads();                                               // the last barrier: every count of the share is in
	rc_flush(mc, t, 256, tag, [&](int i) { return s_ctx[i]; }, [&](int i) { return s_cyc[i]; },
	         [&](int64_t word, uint64_t n, uint64_t e) { atomicAdd(&tab[word], (unsigned long long)n); if (e) atomicAdd(&tab[word + 1], (unsigned long long)e); });
	for (int d = 32; d; d >>= 1) n_masked += __shfl_xor(n_masked, d);
	if (lane == 0) {
		if (n_took) atomicAdd(&cnt[RC_T_RECORDS], (unsigned long long)n_took);
		if (n_masked) atomicAdd(&cnt[RC_T_MASKED], (unsigned long long)n_masked);
	}
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV; }
inline uint64_t get64(const uint8_t *p) { uint64_t v = 0; for (int k = 7; k >= 0; --k) v = v << 8 | p[k]; return v; }

} // namespace

// The stage's buffers: counted by bwahip_recal_hbm_need (recal_host.cpp), but for a packed reference of the caller's
struct RecalStage final : RecordStage {
	Tally hbm;
	DevBuf tab{hbm}, cnt{hbm};
	HostBuf h_tab;
	Event ev[2];                                                   // begin, end
	// what recal_stage_set gave.  mask: the caller's mask, uploaded once per call as the reference is (held: with a mask)
	bwahip_recal_opt_t opt = { 0, 0, RC_DEFAULT_EXCLUDE, RC_DEFAULT_CYCLE };
	StageRef ref{hbm}; DevOnce mask{hbm};
	bwahip_recal_stats_t *stats = nullptr;
	// the call in flight
	int64_t n_records = 0;
	size_t tab_words() const { return (size_t)rc_table_words(opt.max_cycle); }
	int64_t hbm_need(int64_t) const override { return bwahip_recal_hbm_need(ref.sum, opt.max_cycle, mask.held); }
	int begin(bwahip_ctx *c, int64_t n_records) override;
	int records(bwahip_ctx *c, const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0) override;
	int done(bwahip_ctx *c) override;
	int write() override { return write_all(fd, bytes.data(), (int64_t)bytes.size(), "writing the recalibration table"); }
	bool takes_windows() const override { return true; }           // every record is read once
};

RecordStage *recal_stage_new() { return new RecalStage; }

void recal_stage_set(RecordStage *rs, const bwahip_recal_opt_t &opt, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const uint8_t *mask, int fd, bwahip_recal_stats_t *st)
{
	RecalStage *s = static_cast<RecalStage*>(rs);
	s->opt = opt; s->fd = fd; s->stats = st;
	s->ref.set(n_ref, ref_len, pac);
	s->mask.set(s->ref.sum > 0 ? mask : nullptr, (size_t)((s->ref.sum + 7) / 8));   // a mask over no base: none
}

int RecalStage::begin(bwahip_ctx *c, int64_t n_records_)
{
	if (!c || n_records_ < 0) return BWAHIP_EINVAL;
	int rc;
	n_records = n_records_;
	if ((rc = ref.begin(c))) return rc;
	if (!n_records) return 0;                                      // no record: nothing to launch, done writes the header alone
	HIP_TRY(hipSetDevice(c->device));
	for (auto &e : ev) if (!e && (rc = e.make())) return rc;
	hipStream_t q = c->stream;
	if ((rc = tab.ensure(tab_words() * 8)) || (rc = cnt.ensure(RC_T_WORDS * 8)) || (rc = h_tab.ensure((tab_words() + RC_T_WORDS) * 8))) return rc;
	HIP_TRY(hipEventRecord(ev[0], q));
	if ((rc = ref.upload(q)) || (rc = mask.begin(q))) return rc;
	HIP_TRY(hipMemsetAsync(tab.p, 0, tab_words() * 8, q));
	HIP_TRY(hipMemsetAsync(cnt.p, 0, RC_T_WORDS * 8, q));
	HIP_TRY(hipMemsetAsync(cnt.as<unsigned long long>() + RC_T_ERR, 0xff, 8, q));
	return 0;
}

// n_rec records of one run: record i = rec[off[i] .. off[i+1]) within the run's `len` bytes; ord0: the ordinal of its first record in the order given
int RecalStage::records(bwahip_ctx *c, const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0)
{
	if (!n_rec) return 0;
	if (n_rec > 0x7fffffffll) return BWAHIP_ECAPACITY;
	hipLaunchKernelGGL(k_rc_count, dim3((unsigned)((n_rec + RC_SHARE - 1) / RC_SHARE)), dim3(256), 0, c->stream, rec, off, n_rec, len, ord0, (int)ref.n_ref, ref.d_len(), ref.d_off(), ref.d_pac,
	                   ref.pac_bytes, mask.held ? mask.d.as<uint8_t>() : nullptr, (int64_t)mask.h.size(), opt, tab.as<unsigned long long>(), cnt.as<unsigned long long>());
	return launched();
}

// the download (awaited) and the file's bytes; the first offending record's code when one was refused
int RecalStage::done(bwahip_ctx *c)
{
	bwahip_recal_stats_t st;
	memset(&st, 0, sizeof st);
	RcTables t;
	t.n_ref = ref.n_ref; t.opt = opt;
	int rc;
	if (!n_records) {
		const std::vector<uint64_t> z(tab_words(), 0);
		t.tab = z.data();
		if ((rc = rc_serialise(t, &bytes))) return rc;
	} else {
		hipStream_t q = c->stream;
		HIP_TRY(hipEventRecord(ev[1], q));
		uint64_t *h = (uint64_t*)h_tab.p;
		HIP_TRY(hipMemcpyAsync(h, tab.p, tab_words() * 8, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipMemcpyAsync(h + tab_words(), cnt.p, RC_T_WORDS * 8, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		const uint64_t *k = h + tab_words();
		if (k[RC_T_ERR] != ~0ull) return (k[RC_T_ERR] & 0xff) == RC_BAD_LENGTH ? BWAHIP_ECAPACITY : BWAHIP_EINVAL;
		t.tab = h; t.n_records = k[RC_T_RECORDS]; t.n_masked = k[RC_T_MASKED];
		if ((rc = rc_serialise(t, &bytes))) return rc == BWAHIP_EINVAL ? BWAHIP_EINTERNAL : rc;
		float ms = 0;
		if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st.recal_ms = ms;
		st.hbm_bytes = (int64_t)hbm.bytes;
	}
	const uint8_t *b = bytes.data();                               // the header's counts: 80 bytes are there
	st.n_records = (int64_t)get64(b + 24); st.n_bases = (int64_t)get64(b + 32); st.n_err = (int64_t)get64(b + 40); st.n_masked = (int64_t)get64(b + 48);
	for (int k = 0; k < 3; ++k) st.n_rows[k] = (int64_t)get64(b + 56 + 8 * k);
	st.rc_bytes = (int64_t)bytes.size();
	if (stats) *stats = st;
	return 0;
}

// Exactly the stage above on the caller's records, the caller's packed reference and the caller's mask: all are uploaded, the records as one run
extern "C" int bwahip_kat_recal(bwahip_ctx *c, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const uint8_t *mask,
                                const bwahip_recal_opt_t *opt, uint8_t *out, int64_t out_cap, int64_t *out_len)
{
	if (!c || !out_len || n_rec < 0 || n_rec > 0x7fffffffll || out_cap < 0 || (out_cap && !out) || (n_rec && (!rec || !rec_off))) return BWAHIP_EINVAL;
	*out_len = 0;
	bwahip_recal_opt_t o;
	int64_t sum = 0;
	int rc;
	if ((rc = rc_resolve(opt, &o)) || (rc = check_refs(n_ref, ref_len, &sum, PU_MAX_SUM))) return rc;
	if (sum && !pac) return BWAHIP_EINVAL;
	RecalStage s;
	recal_stage_set(&s, o, n_ref, ref_len, sum ? pac : nullptr, mask, -1, nullptr);
	return record_stage_kat(&s, c, rec, rec_off, n_rec, out, out_cap, out_len);
}
