// K9i -- the pileup of candidate variant sites of the device-merged, coordinate-sorted BAM file, where the runs lie.  The rule
// is in include/bwahip.h; how a record is read and judged, a base, a key and the tables are pileup_tables.h, shared with the host builder.
// All on the context's stream:
//
//   count          k_pu_count, 16 lanes per record of a run (a wavefront holds four records): pu_parse (every field bounded by the record's
//                  length); the first offending record through one 64-bit atomicMin; the walk of the CIGAR with the group's lanes on 16
//                  consecutive bases of an M = X operation, four times 16 a round -- a lane reads its base's nibble byte and its quality
//                  byte, neighbours read neighbouring bytes, and the reference base out of the aligned 32-bit word of the packed sequence
//                  that holds it (16 bases: a group touches two words); the twelve loads of a round are independent -- then a ballot per
//                  16 bases, cut to the group's 16 bits, counts the observations; D and I are one lane's.
//                  The record's count goes to its word;
//   scan           launch_scan over the records' counts: every record's first slot.  The sum comes back (more than 2^31 - 1: refused);
//   emit           k_pu_emit, the same walk for the records that have a slot: the ballot's bits below a lane give its slot, the key --
//                  position among all contigs' bases (40 bits) | kind (2) | allele (21) | strand (1) -- goes there.  A record's slots are
//                  its own, their order inside does not matter: the keys are sorted.  k_pu_kinds counts the keys by kind;
//   sort           bam_sort_radix over the context's sort buffers (the ordinals travel along and are not read);
//   alleles        k_pu_heads: a head where key >> 1 changes; launch_scan; k_pu_starts: every allele's first key; k_pu_alleles: the
//                  segment's length is fwd + rev, a binary search for its first reverse key parts them; kept when fwd + rev >= min_alt;
//                  launch_scan; k_pu_compact: the kept alleles, in order;
//   sites          k_pu_site_heads: a head where a kept allele's position changes; launch_scan; k_pu_sites: position, reference base,
//                  first allele, counters at zero;
//   evidence       k_pu_evidence, one thread per record of a run: the lower bound of its first base among the sites' positions -- most
//                  records end there -- then the CIGAR alongside the sites inside its span: n_cov for a site under an M = X or D
//                  operation, n_ref for a base that passes and equals the reference (32-bit atomicAdd: sums, so the order does not matter);
//   one download   of the two compact tables, awaited once; they go through pu_serialise (pileup_host.cpp), the host builder's serialiser.
//
// Three counts come back on the way (observations, alleles, kept alleles and sites), each sizing the buffers of the next step.  No kernel
// waits for another workgroup, none uses LDS.  The lanes of a group take every branch of the walk together -- what differs between them
// is inside `if`s without a ballot -- and groups of one wavefront that are in different operations meet in the same ballot with their own bits.
#include "ctx_internal.h"
#include "pileup_tables.h"
#include "sidecar_host.h"

namespace {

constexpr int PU_ROUND = 4;                                      // a lane takes this many bases, 16 apart, before the group's ballots: the loads of a round do not wait for each other
enum { PU_T_OBS = 0, PU_T_ERR = 3, PU_T_SLOTS = 4, PU_T_WORDS = 8 };   // the stage's counters: observations by kind; the first offending record; count and emit disagree

// the reference base at position g among all contigs' bases, out of the aligned word that holds it -- the last four bytes where that word
// would end behind the sequence -- without a branch, so that a lane's loads of one round are issued together
__device__ __forceinline__ uint32_t pu_ref2_word(const uint8_t *pac, int64_t pac_bytes, int64_t g)
{
	const int64_t byte = g >> 2;
	if (pac_bytes < 4) return pac[byte] >> ((~g & 3) << 1) & 3;    // (the same in every lane: a reference of a dozen bases)
	int64_t at = byte & ~3ll;
	if (at > pac_bytes - 4) at = pac_bytes - 4;
	uint32_t v;
	__builtin_memcpy(&v, pac + at, 4);
	return v >> ((int)(byte - at) * 8 + (int)((~g & 3) << 1)) & 3;
}

// The walk of pu_walk (pileup_tables.h) by a group of 16 lanes, observations only.  l: the lane in its group; gshift: the group's first lane
// in the wavefront.  Returns the record's observations (the same in every lane); EMIT: their keys go to out[0 .. cap).
template <bool EMIT> __device__ __forceinline__ uint32_t pu_walk16(const PuRec &r, int64_t L, int64_t g0, const uint8_t *pac, int64_t pac_bytes, int min_baseq, int l, int gshift,
                                                                   unsigned long long *out, uint32_t cap)
{
	const uint32_t strand = r.q.flag >> 4 & 1, below = (1u << l) - 1;
	const bool all_pass = r.qual[0] == 0xff;
	int64_t p = r.q.pos, q = 0;
	uint32_t n_out = 0;
	for (int32_t k = 0; k < r.q.n_cigar; ++k) {
		const uint32_t w = bam_ld32(r.q.cig + 4 * k), op = w & 15;
		const int64_t n = w >> 4;
		if (pu_is_match(op)) {
			const int64_t m = L - p < n ? (L - p > 0 ? L - p : 0) : n;   // the bases inside the contig
			for (int64_t j0 = 0; j0 < m; j0 += 16 * PU_ROUND) {          // a round: PU_ROUND x 16 bases, a lane's loads independent of each other
				bool has[PU_ROUND];
				uint64_t key[PU_ROUND];
#pragma unroll
				for (int u = 0; u < PU_ROUND; ++u) {
					const int64_t j = j0 + 16 * u + l, jj = j < m ? j : j0;   // behind the operation's end: a base of it again, and no observation
					const int c2 = pu_code2(pu_base(r.seq, q + jj));        // the three loads whatever the others say: nothing waits for a branch
					const uint32_t ql = r.qual[q + jj], rb = pu_ref2_word(pac, pac_bytes, g0 + p + jj);
					has[u] = (j < m) & (c2 >= 0) & (all_pass | (ql >= (uint32_t)min_baseq)) & ((uint32_t)c2 != rb);
					key[u] = pu_key(g0 + p + jj, PU_SNV, pu_allele21(PU_SNV, 1, (uint32_t)(c2 & 3)), strand);
				}
#pragma unroll
				for (int u = 0; u < PU_ROUND; ++u) {
					const uint32_t gb = (uint32_t)(__ballot(has[u]) >> gshift) & 0xffffu;
					const uint32_t slot = n_out + (uint32_t)__popc(gb & below);
					if (EMIT && has[u] && slot < cap) out[slot] = key[u];
					n_out += (uint32_t)__popc(gb);
				}
			}
			p += n; q += n;
		} else if (op == 2) {
			if (n && p < L) {
				if (EMIT && l == 0 && n_out < cap) { out[n_out] = pu_key(g0 + p, PU_DEL, pu_allele21(PU_DEL, n < PU_DEL_CAP ? (uint32_t)n : PU_DEL_CAP, 0), strand); }
				++n_out;
			}
			p += n;
		} else if (op == 1) {
			if (n && p < L) {
				bool other = false;                                      // a base that is not A C G T
				for (int64_t j = l; j < n; j += 16) other |= pu_code2(pu_base(r.seq, q + j)) < 0;
				if (!((uint32_t)(__ballot(other) >> gshift) & 0xffffu)) {
					if (EMIT && l == 0 && n_out < cap) { out[n_out] = pu_key(g0 + p, PU_INS, pu_ins_allele(r.seq, q, n), strand); }
					++n_out;
				}
			}
			q += n;
		} else if (op == 3) p += n;
		else if (op == 4) q += n;
	}
	return n_out;
}

// cnt[ord0 + i]: the observations of record i of the run (0 for a record that does not take part, or is refused)
__global__ __launch_bounds__(256) void k_pu_count(const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0, int n_ref, const int64_t *ref_len, const int64_t *ref_off,
                                                  const uint8_t *pac, int64_t pac_bytes, bwahip_pileup_opt_t opt, int *cnt, unsigned long long *tab)
{
	const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
	const int lane = threadIdx.x & 63, l = lane & 15;
	if (i >= n_rec) return;
	PuRec r;
	const int64_t o = off[i], e = off[i + 1];
	const bool live = o >= 0 && e >= o && e <= len && pu_parse(rec + o, e - o, n_ref, &r);
	uint32_t n = 0;
	if (!live) { if (l == 0) atomicMin(&tab[PU_T_ERR], (unsigned long long)(ord0 + i) << 8 | 1u); }   // the first offending record decides
	else if (pu_takes_part(r, opt)) n = pu_walk16<false>(r, ref_len[r.q.ref], ref_off[r.q.ref], pac, pac_bytes, opt.min_baseq, l, lane & 48, nullptr, 0);
	if (l == 0) cnt[ord0 + i] = (int)n;
}

// obs_off: the exclusive scan of cnt.  The records were judged by k_pu_count: one that it refused has no slot
__global__ __launch_bounds__(256) void k_pu_emit(const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t ord0, int n_ref, const int64_t *ref_len, const int64_t *ref_off,
                                                 const uint8_t *pac, int64_t pac_bytes, bwahip_pileup_opt_t opt, const int64_t *obs_off, unsigned long long *keys, unsigned long long *tab)
{
	const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
	const int lane = threadIdx.x & 63, l = lane & 15;
	if (i >= n_rec) return;
	const int64_t at = obs_off[ord0 + i];
	const uint32_t cap = (uint32_t)(obs_off[ord0 + i + 1] - at);
	if (!cap) return;
	PuRec r;
	const int64_t o = off[i];
	if (!pu_parse(rec + o, off[i + 1] - o, n_ref, &r) || !pu_takes_part(r, opt) ||
	    pu_walk16<true>(r, ref_len[r.q.ref], ref_off[r.q.ref], pac, pac_bytes, opt.min_baseq, l, lane & 48, keys + at, cap) != cap) { if (l == 0) tab[PU_T_SLOTS] = 1; }   // every writer writes 1
}

// tab[kind]: the keys of that kind.  A fixed grid walks the keys; a thread keeps its counts, a wavefront adds them once: a few thousand
// atomics on three words (one per wavefront of k_pu_count was a million on one)
__global__ __launch_bounds__(256) void k_pu_kinds(const unsigned long long *keys, int n, unsigned long long *tab)
{
	uint32_t c[3] = { 0, 0, 0 };
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
		const uint32_t kind = (uint32_t)(keys[i] >> 22) & 3;
		c[0] += kind == PU_SNV; c[1] += kind == PU_DEL; c[2] += kind == PU_INS;
	}
	for (int k = 0; k < 3; ++k) {                                   // every lane of the wavefront is here
		uint32_t v = c[k];
		for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
		if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tab[PU_T_OBS + k], (unsigned long long)v);
	}
}

__global__ __launch_bounds__(256) void k_pu_heads(const unsigned long long *keys, int n, int *flag)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) flag[i] = i == 0 || keys[i] >> 1 != keys[i - 1] >> 1;
}

// astart[a]: the first key of allele a; astart[n_all] = n
__global__ __launch_bounds__(256) void k_pu_starts(const int *flag, const int64_t *pos, int n, int *astart)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	if (flag[i]) astart[pos[i]] = i;
	if (i == 0) astart[pos[n]] = n;
}

// fr[a]: the forward and the reverse keys of allele a (the forward ones come first); keep[a]: there are min_alt of them
__global__ __launch_bounds__(256) void k_pu_alleles(const unsigned long long *keys, const int *astart, int n_all, int min_alt, uint2 *fr, int *keep)
{
	const int a = blockIdx.x * 256 + threadIdx.x;
	if (a >= n_all) return;
	const int s = astart[a], e = astart[a + 1];
	int lo = s, hi = e;                                            // the first reverse key is in [lo, hi]
	while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (keys[mid] & 1) hi = mid; else lo = mid + 1; }
	fr[a] = make_uint2((unsigned)(lo - s), (unsigned)(e - lo));
	keep[a] = e - s >= min_alt;
}

__global__ __launch_bounds__(256) void k_pu_compact(const unsigned long long *keys, const int *astart, const uint2 *fr, const int *keep, const int64_t *kpos, int n_all, PuAllele *out)
{
	const int a = blockIdx.x * 256 + threadIdx.x;
	if (a >= n_all || !keep[a]) return;
	PuAllele x;
	int64_t g;
	pu_unkey(keys[astart[a]], &g, &x.kind, &x.len, &x.bases);
	x.gpos = (uint64_t)g; x.fwd = fr[a].x; x.rev = fr[a].y; x.pad = 0;
	out[kpos[a]] = x;
}

__global__ __launch_bounds__(256) void k_pu_site_heads(const PuAllele *al, int n_kept, int *flag)
{
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k < n_kept) flag[k] = k == 0 || al[k].gpos != al[k - 1].gpos;
}

__global__ __launch_bounds__(256) void k_pu_sites(const PuAllele *al, const int *flag, const int64_t *spos, int n_kept, const uint8_t *pac, int64_t pac_bytes, PuSite *sites)
{
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n_kept || !flag[k]) return;
	PuSite s;
	s.gpos = al[k].gpos; s.ref_base = pu_ref2_word(pac, pac_bytes, (int64_t)s.gpos); s.first = (uint32_t)k; s.n_cov = s.n_ref_fwd = s.n_ref_rev = s.pad = 0;
	sites[spos[k]] = s;
}

// One thread per record.  The sites ascend by position among all contigs' bases, so those inside a record's span are neighbours
__global__ __launch_bounds__(256) void k_pu_evidence(const uint8_t *rec, const int64_t *off, int64_t n_rec, int n_ref, const int64_t *ref_len, const int64_t *ref_off,
                                                     bwahip_pileup_opt_t opt, PuSite *sites, int n_sites)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_rec) return;
	PuRec r;
	const int64_t o = off[i];
	if (!pu_parse(rec + o, off[i + 1] - o, n_ref, &r) || r.q.ref < 0) return;   // (judged by k_pu_count)
	const int64_t L = ref_len[r.q.ref], g0 = ref_off[r.q.ref], g_end = g0 + L;
	int64_t p = r.q.pos, q = 0;
	if (p >= L) return;
	int lo = 0, hi = n_sites;                                      // the first site at or behind the record's first base
	while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if ((int64_t)sites[mid].gpos < g0 + p) lo = mid + 1; else hi = mid; }
	int s = lo;
	if (s >= n_sites || (int64_t)sites[s].gpos >= g_end || !pu_takes_part(r, opt)) return;
	const bool all_pass = r.qual[0] == 0xff;
	const uint32_t strand = r.q.flag >> 4 & 1;
	for (int32_t k = 0; k < r.q.n_cigar && s < n_sites && p < L; ++k) {
		const uint32_t w = bam_ld32(r.q.cig + 4 * k), op = w & 15;
		const int64_t n = w >> 4;
		const bool match = pu_is_match(op);
		if (match || op == 2 || op == 3) {
			const int64_t e = g0 + p + n < g_end ? g0 + p + n : g_end;   // the sites in [g0 + p, e) lie under this operation
			for (; s < n_sites && (int64_t)sites[s].gpos < e; ++s) {
				if (op == 3) continue;
				atomicAdd(&sites[s].n_cov, 1u);
				if (!match) continue;
				const int64_t qq = q + ((int64_t)sites[s].gpos - g0 - p);
				const int c2 = pu_code2(pu_base(r.seq, qq));
				if (c2 >= 0 && (all_pass || r.qual[qq] >= opt.min_baseq) && (uint32_t)c2 == sites[s].ref_base) atomicAdd(strand ? &sites[s].n_ref_rev : &sites[s].n_ref_fwd, 1u);
			}
			p += n;
			if (match) q += n;
		} else if (op == 1 || op == 4) q += n;
	}
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV; }
inline unsigned blocks(int64_t threads) { return (unsigned)((threads + 255) / 256); }

} // namespace

// The stage's buffers.  cnt and obs_off are what bwahip_pileup_hbm_need counts; the others are made at the finish, when their sizes are known
struct PileupStage final : RecordStage {
	Tally hbm;
	DevBuf cnt{hbm}, obs_off{hbm}, tab{hbm};
	DevBuf flag{hbm}, pos{hbm}, astart{hbm}, fr{hbm}, alleles{hbm}, sites{hbm};
	HostBuf h_tab;
	Event ev[4];                                                   // begin, the keys written, the sites made, end
	// what pu_stage_set gave
	bwahip_pileup_opt_t opt = { 0, 0, 1796, 2 };
	StageRef ref{hbm};
	bwahip_pileup_stats_t *stats = nullptr;
	// the call in flight
	int64_t n_records = 0;
	struct Run { const uint8_t *rec; const int64_t *off; int64_t n_rec, ord0; };
	std::vector<Run> runs;                                         // the runs that passed k_pu_count: emit and evidence read them again
	int64_t hbm_need(int64_t n) const override { return bwahip_pileup_hbm_need(n); }
	int begin(bwahip_ctx *c, int64_t n_records) override;
	int records(bwahip_ctx *c, const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0) override;
	int done(bwahip_ctx *c) override;
	int write() override { return write_all(fd, bytes.data(), (int64_t)bytes.size(), "writing the pileup"); }
	bool takes_windows() const override { return false; }          // emit and evidence read the runs again
};

RecordStage *pu_stage_new() { return new PileupStage; }

void pu_stage_set(RecordStage *rs, const bwahip_pileup_opt_t &opt, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, int fd, bwahip_pileup_stats_t *ps)
{
	PileupStage *s = static_cast<PileupStage*>(rs);
	s->opt = opt; s->fd = fd; s->stats = ps;
	s->ref.set(n_ref, ref_len, pac);
}

int PileupStage::begin(bwahip_ctx *c, int64_t n_records_)
{
	if (!c || n_records_ < 0 || n_records_ > 0x7fffffffll) return BWAHIP_EINVAL;
	int rc;
	n_records = n_records_;
	if ((rc = ref.begin(c))) return rc;
	runs.clear();
	if (!n_records) return 0;                                      // no record: nothing to launch, finish writes the file of no site
	HIP_TRY(hipSetDevice(c->device));
	for (auto &e : ev) if (!e && (rc = e.make())) return rc;
	hipStream_t q = c->stream;
	if ((rc = cnt.ensure(((size_t)n_records + 1) * 4)) || (rc = obs_off.ensure(((size_t)n_records + 1) * 8)) || (rc = tab.ensure(PU_T_WORDS * 8))) return rc;
	HIP_TRY(hipEventRecord(ev[0], q));
	if ((rc = ref.upload(q))) return rc;
	HIP_TRY(hipMemsetAsync(tab.p, 0, PU_T_WORDS * 8, q));
	HIP_TRY(hipMemsetAsync(tab.as<unsigned long long>() + PU_T_ERR, 0xff, 8, q));
	return 0;
}

// n_rec records of one run: record i = rec[off[i] .. off[i+1]) within the run's `len` bytes; ord0: the ordinal of its first record in the order
// given.  The run is counted here and read again by the finish: it stays where it is until then
int PileupStage::records(bwahip_ctx *c, const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0)
{
	if (!n_rec) return 0;
	if (ord0 < 0 || ord0 + n_rec > n_records) return BWAHIP_EINTERNAL;
	hipLaunchKernelGGL(k_pu_count, dim3(blocks(n_rec * 16)), dim3(256), 0, c->stream, rec, off, n_rec, len, ord0, (int)ref.n_ref, ref.d_len(), ref.d_off(), ref.d_pac, ref.pac_bytes, opt,
	                   cnt.as<int>(), tab.as<unsigned long long>());
	runs.push_back({ rec, off, n_rec, ord0 });
	return launched();
}

// everything behind the count, the download (awaited) and the file's bytes; BWAHIP_EINVAL when a record was refused
int PileupStage::done(bwahip_ctx *c)
{
	bwahip_pileup_stats_t st;
	memset(&st, 0, sizeof st);
	PuTables t;
	t.n_ref = ref.n_ref; t.ref_len = ref.len.data(); t.opt = opt;
	int rc;
	if (n_records) {
		hipStream_t q = c->stream;
		BamSort &bs = c->bs;
		int64_t counted = 0;
		for (const auto &r : runs) counted += r.n_rec;
		if (counted != n_records) return BWAHIP_EINTERNAL;        // a record nobody counted has no slot
		const int R = (int)n_records;
		if ((rc = launch_scan(cnt.as<int>(), obs_off.as<int64_t>(), R, c->d_scan, q))) return rc;
		unsigned long long tab[PU_T_WORDS];
		int64_t N = 0;
		HIP_TRY(hipMemcpyAsync(&N, obs_off.as<int64_t>() + R, 8, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipMemcpyAsync(tab, this->tab.p, sizeof tab, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (tab[PU_T_ERR] != ~0ull) return BWAHIP_EINVAL;
		if (N < 0 || N > PU_MAX_OBS) return BWAHIP_ECAPACITY;
		const int n = (int)N;
		int n_all = 0, n_kept = 0, n_sites = 0, cur = 0;            // cur: which of the sort's two key buffers holds the sorted keys
		if (n) {
			if ((rc = bs.keys[0].ensure((size_t)n * 8)) || (rc = bs.keys[1].ensure((size_t)n * 8)) || (rc = bs.idx[0].ensure((size_t)n * 4)) || (rc = bs.idx[1].ensure((size_t)n * 4)) ||
			    (rc = this->flag.ensure((size_t)n * 4)) || (rc = this->pos.ensure(((size_t)n + 1) * 8))) return rc;
			for (const auto &r : runs) {
				hipLaunchKernelGGL(k_pu_emit, dim3(blocks(r.n_rec * 16)), dim3(256), 0, q, r.rec, r.off, r.n_rec, r.ord0, (int)ref.n_ref, ref.d_len(), ref.d_off(), ref.d_pac, ref.pac_bytes, opt,
				                   obs_off.as<int64_t>(), bs.keys[0].as<unsigned long long>(), this->tab.as<unsigned long long>());
				if ((rc = launched())) return rc;
			}
			hipLaunchKernelGGL(k_pu_kinds, dim3(blocks(n) < 1024 ? blocks(n) : 1024), dim3(256), 0, q, bs.keys[0].as<unsigned long long>(), n, this->tab.as<unsigned long long>());
			if ((rc = launched())) return rc;
		}
		HIP_TRY(hipEventRecord(ev[1], q));
		if (n) {
			if ((rc = bam_sort_radix(c, n, 64, &cur))) return rc;       // the ordinals in bs.idx are moved along and never read
			const unsigned long long *keys = bs.keys[cur].as<unsigned long long>();
			int *flag = this->flag.as<int>();
			int64_t *pos = this->pos.as<int64_t>(), got = 0;
			hipLaunchKernelGGL(k_pu_heads, dim3(blocks(n)), dim3(256), 0, q, keys, n, flag);
			if ((rc = launched()) || (rc = launch_scan(flag, pos, n, c->d_scan, q))) return rc;
			HIP_TRY(hipMemcpyAsync(&got, pos + n, 8, hipMemcpyDeviceToHost, q));
			HIP_TRY(hipStreamSynchronize(q));
			if (got < 1 || got > n) return BWAHIP_EINTERNAL;
			n_all = (int)got;
			if ((rc = astart.ensure(((size_t)n_all + 1) * 4)) || (rc = fr.ensure((size_t)n_all * 8))) return rc;
			hipLaunchKernelGGL(k_pu_starts, dim3(blocks(n)), dim3(256), 0, q, flag, pos, n, astart.as<int>());
			if ((rc = launched())) return rc;
			hipLaunchKernelGGL(k_pu_alleles, dim3(blocks(n_all)), dim3(256), 0, q, keys, astart.as<int>(), n_all, opt.min_alt, fr.as<uint2>(), flag);   // flag: now `keep`
			if ((rc = launched()) || (rc = launch_scan(flag, pos, n_all, c->d_scan, q))) return rc;
			HIP_TRY(hipMemcpyAsync(&got, pos + n_all, 8, hipMemcpyDeviceToHost, q));
			HIP_TRY(hipStreamSynchronize(q));
			if (got < 0 || got > n_all) return BWAHIP_EINTERNAL;
			n_kept = (int)got;
		}
		if (n_kept) {
			if ((rc = alleles.ensure((size_t)n_kept * sizeof(PuAllele)))) return rc;
			const unsigned long long *keys = bs.keys[cur].as<unsigned long long>();
			int *flag = this->flag.as<int>();
			int64_t *pos = this->pos.as<int64_t>(), got = 0;
			hipLaunchKernelGGL(k_pu_compact, dim3(blocks(n_all)), dim3(256), 0, q, keys, astart.as<int>(), fr.as<uint2>(), flag, pos, n_all, alleles.as<PuAllele>());
			if ((rc = launched())) return rc;
			hipLaunchKernelGGL(k_pu_site_heads, dim3(blocks(n_kept)), dim3(256), 0, q, alleles.as<PuAllele>(), n_kept, flag);   // flag: now the sites' heads
			if ((rc = launched()) || (rc = launch_scan(flag, pos, n_kept, c->d_scan, q))) return rc;
			HIP_TRY(hipMemcpyAsync(&got, pos + n_kept, 8, hipMemcpyDeviceToHost, q));
			HIP_TRY(hipStreamSynchronize(q));
			if (got < 1 || got > n_kept) return BWAHIP_EINTERNAL;
			n_sites = (int)got;
			if ((rc = sites.ensure((size_t)n_sites * sizeof(PuSite)))) return rc;
			hipLaunchKernelGGL(k_pu_sites, dim3(blocks(n_kept)), dim3(256), 0, q, alleles.as<PuAllele>(), flag, pos, n_kept, ref.d_pac, ref.pac_bytes, sites.as<PuSite>());
			if ((rc = launched())) return rc;
		}
		HIP_TRY(hipEventRecord(ev[2], q));
		for (size_t k = 0; n_sites && k < runs.size(); ++k) {
			const auto &r = runs[k];
			hipLaunchKernelGGL(k_pu_evidence, dim3(blocks(r.n_rec)), dim3(256), 0, q, r.rec, r.off, r.n_rec, (int)ref.n_ref, ref.d_len(), ref.d_off(), opt, sites.as<PuSite>(), n_sites);
			if ((rc = launched())) return rc;
		}
		HIP_TRY(hipEventRecord(ev[3], q));
		const size_t a_bytes = (size_t)n_kept * sizeof(PuAllele), s_bytes = (size_t)n_sites * sizeof(PuSite);
		if ((rc = h_tab.ensure(a_bytes + s_bytes + 8))) return rc;
		uint8_t *h = (uint8_t*)h_tab.p;
		if (a_bytes) HIP_TRY(hipMemcpyAsync(h, alleles.p, a_bytes, hipMemcpyDeviceToHost, q));
		if (s_bytes) HIP_TRY(hipMemcpyAsync(h + a_bytes, sites.p, s_bytes, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipMemcpyAsync(tab, this->tab.p, sizeof tab, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (tab[PU_T_SLOTS] || (uint64_t)N != tab[0] + tab[1] + tab[2]) { fprintf(stderr, "[bwahip] pileup: a record's observations were counted and written differently\n"); return BWAHIP_EINTERNAL; }
		for (int k = 0; k < 3; ++k) t.n_obs[k] = tab[k];
		t.n_alleles = n_kept; t.alleles = (const PuAllele*)h; t.n_sites = n_sites; t.sites = (const PuSite*)(h + a_bytes);
		if ((rc = pu_serialise(t, &bytes))) return rc == BWAHIP_EINVAL ? BWAHIP_EINTERNAL : rc;
		float ms = 0;
		if (hipEventElapsedTime(&ms, ev[0], ev[3]) == hipSuccess) st.pileup_ms = ms;
		if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st.observe_ms = ms;
		if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) st.sort_ms = ms;
		if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) st.evidence_ms = ms;
		st.hbm_bytes = (int64_t)(hbm.bytes + (n ? bs.keys[0].cap + bs.keys[1].cap + bs.idx[0].cap + bs.idx[1].cap : 0));
	} else if ((rc = pu_serialise(t, &bytes))) return rc;
	st.n_sites = t.n_sites; st.n_alleles = t.n_alleles;
	for (int k = 0; k < 3; ++k) st.n_obs[k] = (int64_t)t.n_obs[k];
	st.pu_bytes = (int64_t)bytes.size();
	if (stats) *stats = st;
	return 0;
}

// Exactly the stage above on the caller's records and the caller's packed reference: both are uploaded, the records as one run
extern "C" int bwahip_kat_pileup(bwahip_ctx *c, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac,
                                 const bwahip_pileup_opt_t *opt, uint8_t *out, int64_t out_cap, int64_t *out_len)
{
	if (!c || !out_len || n_rec < 0 || n_rec > 0x7fffffffll || out_cap < 0 || (out_cap && !out) || (n_rec && (!rec || !rec_off))) return BWAHIP_EINVAL;
	*out_len = 0;
	bwahip_pileup_opt_t o;
	int64_t sum = 0;
	int rc;
	if ((rc = pu_resolve(opt, &o)) || (rc = check_refs(n_ref, ref_len, &sum, PU_MAX_SUM))) return rc;
	if (sum && !pac) return BWAHIP_EINVAL;
	PileupStage s;
	pu_stage_set(&s, o, n_ref, ref_len, sum ? pac : nullptr, -1, nullptr);
	return record_stage_kat(&s, c, rec, rec_off, n_rec, out, out_cap, out_len);
}
