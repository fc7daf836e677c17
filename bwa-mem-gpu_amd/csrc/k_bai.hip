// K9f -- the BAI index of the device-merged, coordinate-sorted BAM file, built where the records lie.  What a second
// program would inflate and parse again is in HBM when the merger's finish ends: the records in sorted order (addr[idx[i]]), their
// offsets in the uncompressed stream (out_off) and the length of every BGZF member.  The stage, all on the context's stream:
//
//   parse         k_bai_parse: one thread per sorted record -- bai_parse (bai_tables.h, shared with the host builder: every field bounded
//                 by the record's length) gives refID, pos, end, bin and 0x4; the order against the record before; the first offending
//                 record and its code through one 64-bit atomicMin; per reference the last window reached (atomicMin of its distance
//                 from the top of BAI's range) and the records with 0x4 (atomicAdd);
//   heads         k_bai_heads: 1 where (refID, bin) changes, first and last record of every reference (one writer each); a scan;
//   block offsets one scan over the members' lengths: c_b, 8 bytes per block;
//   chunks        k_bai_chunks: V(begin) of every head, V(end) of every run's last record; the stable radix sort of k_bamsort.hip by
//                 (refID, bin) -- its buffers are free once the last gather is queued, the stream orders the reuse; k_bai_join: a chunk
//                 that begins in the member in which its neighbour ends is joined (ends increase in file order, so the neighbour's end
//                 is the joined predecessor's); a scan; k_bai_compact;
//   linear index  k_bai_lin: a 64-bit atomicMin of the record's begin into every window it covers; k_bai_backfill: an empty window
//                 takes the next one to its right;
//   metadata      k_bai_meta: V of the first begin and the last end, the counts;
//   one download  of the compact tables, which go through bai_serialise (bai_host.cpp), the host builder's serialiser.
//
// No LDS.  The atomics are integer min and add: the result does not depend on the order in which wavefronts run.
#include "ctx_internal.h"
#include "bai_tables.h"

namespace {

constexpr uint64_t NO_KEY = ~0ull;               // a record without a reference, or a refused one
constexpr int TOP = 32767;                       // the last window of BAI's range: (2^29 - 1) >> 14

__global__ __launch_bounds__(256) void k_bai_addr(int n, const uint8_t *rec, const int64_t *rec_off, const uint8_t **addr, int64_t *out_off)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i > n) return;
	out_off[i] = rec_off[i] - rec_off[0];
	if (i < n) addr[i] = rec + rec_off[i];
}

// the sorted records [lo, n)
__global__ __launch_bounds__(256) void k_bai_parse(int lo, int n, const uint8_t *const *addr, const unsigned *idx, const int64_t *out_off, int n_ref,
                                                   uint64_t *rk, int *pos, int *end, uint8_t *unm, unsigned long long *err, int *top, unsigned *n_unm)
{
	const int i = lo + blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint8_t *p = addr[idx[i]];
	const int64_t len = out_off[i + 1] - out_off[i];
	BaiRec r;
	int bad = bai_parse(p, len, n_ref, &r);
	if (bad != BAI_BAD && i > 0 && out_off[i] - out_off[i - 1] >= 12) {   // the order, from fields both records hold within their lengths
		const uint8_t *q = addr[idx[i - 1]];
		if (bai_order_key((int32_t)bam_ld32(p + 4), (int32_t)bam_ld32(p + 8)) < bai_order_key((int32_t)bam_ld32(q + 4), (int32_t)bam_ld32(q + 8))) bad = BAI_BAD;
	}
	if (bad) atomicMin(err, (unsigned long long)i << 8 | (unsigned)bad);   // the first offending record decides
	const bool coor = !bad && r.ref >= 0;
	rk[i] = coor ? (uint64_t)r.ref << 16 | r.bin : NO_KEY;
	pos[i] = coor ? r.pos : 0; end[i] = coor ? r.e : 0; unm[i] = coor ? (uint8_t)r.unm : 0;
	if (!coor) return;
	const int t = TOP - ((r.e - 1) >> 14);
	if (t < top[r.ref]) atomicMin(&top[r.ref], t);                 // (the plain read only spares atomics: the value never rises)
	if (r.unm) atomicAdd(&n_unm[r.ref], 1u);
}

__global__ __launch_bounds__(256) void k_bai_heads(int n, const uint64_t *rk, int *head, int *first, int *last, int *n_coor)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint64_t k = rk[i], prev = i > 0 ? rk[i - 1] : NO_KEY, next = i + 1 < n ? rk[i + 1] : NO_KEY;
	const bool coor = k != NO_KEY;
	head[i] = coor && (i == 0 || prev != k);
	if (!coor) return;
	const int ref = (int)(k >> 16);
	if (prev == NO_KEY || (int)(prev >> 16) != ref) first[ref] = i;
	if (next == NO_KEY || (int)(next >> 16) != ref) last[ref] = i;
	if (next == NO_KEY) *n_coor = i + 1;                           // records without a reference are the tail of the order
}

__global__ __launch_bounds__(256) void k_bai_chunks(int n, const uint64_t *rk, const int64_t *hscan, const int64_t *out_off, int64_t total, const int64_t *coff, int64_t n_blocks,
                                                    int64_t base, uint64_t *ckey, uint64_t *cbeg, uint64_t *cend)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint64_t k = rk[i];
	if (k == NO_KEY) return;
	if (i == 0 || rk[i - 1] != k) { const int64_t c = hscan[i]; ckey[c] = k; cbeg[c] = bai_voffset(out_off[i], total, coff, n_blocks, base); }
	if (i == n - 1 || rk[i + 1] != k) cend[hscan[i + 1] - 1] = bai_voffset(out_off[i + 1], total, coff, n_blocks, base);
}

// chunks in (key, file order): skey[j] / sidx[j] = key and number of the j-th; keep[j] = 0 where it is joined to the one before
__global__ __launch_bounds__(256) void k_bai_join(int m, const uint64_t *skey, const unsigned *sidx, const uint64_t *cbeg, const uint64_t *cend, int *keep)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= m) return;
	keep[j] = !(j > 0 && skey[j] == skey[j - 1] && cbeg[sidx[j]] >> 16 <= cend[sidx[j - 1]] >> 16);
}

__global__ __launch_bounds__(256) void k_bai_compact(int m, const uint64_t *skey, const unsigned *sidx, const uint64_t *cbeg, const uint64_t *cend, const int *keep, const int64_t *kscan,
                                                     uint64_t *okey, uint64_t *obeg, uint64_t *oend, uint64_t *n_out)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= m) return;
	if (keep[j]) { const int64_t o = kscan[j]; okey[o] = skey[j]; obeg[o] = cbeg[sidx[j]]; }
	if (j == m - 1 || keep[j + 1]) oend[kscan[j + 1] - 1] = cend[sidx[j]];
	if (j == 0) *n_out = (uint64_t)kscan[m];
}

__global__ __launch_bounds__(256) void k_bai_lin(int n, const uint64_t *rk, const int *pos, const int *end, const int64_t *out_off, int64_t total, const int64_t *coff, int64_t n_blocks,
                                                 int64_t base, const int64_t *lin_off, unsigned long long *lin)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || rk[i] == NO_KEY) return;
	const unsigned long long vb = bai_voffset(out_off[i], total, coff, n_blocks, base);
	unsigned long long *L = lin + lin_off[rk[i] >> 16];
	for (int w = pos[i] >> 14; w <= (end[i] - 1) >> 14; ++w) if (vb < L[w]) atomicMin(&L[w], vb);
}

// the last window of every reference holds a record, so the walk to the right ends within the reference
__global__ __launch_bounds__(256) void k_bai_backfill(int64_t n_win, const unsigned long long *lin, uint64_t *lin_out)
{
	const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (w >= n_win) return;
	int64_t x = w;
	while (lin[x] == ~0ull && x + 1 < n_win) ++x;
	lin_out[w] = lin[x];
}

__global__ __launch_bounds__(256) void k_bai_meta(int n_ref, const int *first, const int *last, const unsigned *n_unm, const int64_t *out_off, int64_t total, const int64_t *coff,
                                                  int64_t n_blocks, int64_t base, uint64_t *meta)
{
	const int r = blockIdx.x * 256 + threadIdx.x;
	if (r >= n_ref) return;
	const int f = first[r], l = last[r];
	uint64_t *m = meta + 4 * (size_t)r;
	if (f < 0) { m[0] = m[1] = m[2] = m[3] = 0; return; }
	m[0] = bai_voffset(out_off[f], total, coff, n_blocks, base); m[1] = bai_voffset(out_off[l + 1], total, coff, n_blocks, base);
	m[3] = n_unm[r]; m[2] = (uint64_t)(l - f + 1) - n_unm[r];
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV; }
unsigned grid_of(int64_t n) { return (unsigned)((n + 255) / 256); }

} // namespace

// The stage's buffers beside the context's sort buffers: counted by bwahip_bam_devmerge_bai_hbm_need below
struct BaiStage {
	Tally hbm;
	DevBuf mlen{hbm}, coff{hbm};                                   // per member: 4 + 8
	DevBuf rk{hbm}, pos{hbm}, end{hbm}, unm{hbm}, head{hbm}, hscan{hbm};   // per record: 8 + 4 + 4 + 1 + 4 + 8
	DevBuf cbeg{hbm}, cend{hbm}, keep{hbm}, kscan{hbm};            // per chunk before the join: 8 + 8 + 4 + 8 (and 24 of tab)
	DevBuf first{hbm}, last{hbm}, top{hbm}, n_unm{hbm}, lin_off{hbm};   // per reference: 4 + 4 + 4 + 4 + 8 (and 32 of tab)
	DevBuf lin{hbm};                                               // per window: 8 (and 8 of tab)
	DevBuf err{hbm}, tab{hbm};                                     // tab: what is downloaded -- chunk count | metadata | linear index | chunk keys, begins, ends
	DevBuf addr{hbm}, idx{hbm}, off{hbm}, rec{hbm};                // bwahip_kat_bai alone: the caller's records as a merger would hold them
	HostBuf h_tab, h_top;
	Event ev[2];
};

extern "C" int64_t bwahip_bam_devmerge_bai_hbm_need(int64_t n_records, int64_t n_blocks, int64_t n_ref, int64_t n_windows)
{
	if (n_records < 0 || n_blocks < 0 || n_ref < 0 || n_windows < 0) return -1;
	const int64_t work = (29 + 52) * (n_records + 1) + 12 * (n_blocks + 1) + 56 * (n_ref + 1) + 16 * n_windows + 8192;
	return work + work / 8;
}

BaiStage *bai_stage_new() { return new BaiStage; }
void bai_stage_free(BaiStage *s) { delete s; }

int bai_stage_members(BaiStage *s, int64_t n_blocks, int **mlen)
{
	const int rc = s->mlen.ensure((size_t)(n_blocks ? n_blocks : 1) * 4);
	*mlen = s->mlen.as<int>();
	return rc;
}

// what the parse writes and what it adds to, cleared: queued on c->stream
int bai_stage_parse_begin(BaiStage *s, bwahip_ctx *c, int n, int64_t n_blocks, int32_t n_ref)
{
	if (!s || !c || n <= 0 || n_ref < 0) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t q = c->stream;
	const size_t N = (size_t)n, R = (size_t)(n_ref ? n_ref : 1);
	int rc;
	for (auto &e : s->ev) if (!e && (rc = e.make())) return rc;
	if ((rc = s->rk.ensure(N * 8)) || (rc = s->pos.ensure(N * 4)) || (rc = s->end.ensure(N * 4)) || (rc = s->unm.ensure(N)) || (rc = s->head.ensure(N * 4)) ||
	    (rc = s->hscan.ensure((N + 1) * 8)) || (rc = s->coff.ensure(((size_t)n_blocks + 1) * 8)) || (rc = s->first.ensure(R * 4)) || (rc = s->last.ensure(R * 4)) ||
	    (rc = s->top.ensure(R * 4)) || (rc = s->n_unm.ensure(R * 4)) || (rc = s->err.ensure(16)) || (rc = s->h_top.ensure(R * 4 + 32))) return rc;
	HIP_TRY(hipEventRecord(s->ev[0], q));
	HIP_TRY(hipMemsetAsync(s->err.p, 0xff, 8, q));
	HIP_TRY(hipMemsetAsync(s->err.as<uint8_t>() + 8, 0, 8, q));   // n_coor
	HIP_TRY(hipMemsetAsync(s->first.p, 0xff, R * 4, q));
	HIP_TRY(hipMemsetAsync(s->last.p, 0xff, R * 4, q));
	HIP_TRY(hipMemsetAsync(s->top.p, 0x7f, R * 4, q));             // above every window
	HIP_TRY(hipMemsetAsync(s->n_unm.p, 0, R * 4, q));
	return 0;
}

int bai_stage_parse(BaiStage *s, bwahip_ctx *c, int lo, int hi, const uint8_t *const *addr, const unsigned *idx, const int64_t *out_off, int32_t n_ref)
{
	if (hi <= lo) return 0;
	hipLaunchKernelGGL(k_bai_parse, dim3(grid_of((int64_t)hi - lo)), dim3(256), 0, c->stream, lo, hi, addr, idx, out_off, (int)n_ref, s->rk.as<uint64_t>(), s->pos.as<int>(), s->end.as<int>(),
	                   s->unm.as<uint8_t>(), s->err.as<unsigned long long>(), s->top.as<int>(), s->n_unm.as<unsigned>());
	return launched();
}

int bai_stage_run(BaiStage *s, bwahip_ctx *c, int n, const uint8_t *const *addr, const unsigned *idx, const int64_t *out_off, int64_t total, int64_t n_blocks, int64_t base,
                  int32_t n_ref, std::vector<uint8_t> *bytes, bwahip_bai_stats_t *bs, bool parsed)
{
	if (!s || !c || !bytes || n < 0 || n_ref < 0 || base < 0 || n_blocks != bgzf_blocks(total) || n_blocks > 0x7fffffffll) return BWAHIP_EINVAL;
	bwahip_bai_stats_t st;
	memset(&st, 0, sizeof st);
	std::vector<int64_t> lin_off((size_t)n_ref + 1, 0);
	BaiTables t;
	t.n_ref = n_ref; t.lin_off = lin_off.data();
	int rc;
	if (n == 0 || total == 0) {                                    // no record: nothing to launch
		if (n) return BWAHIP_EINVAL;                                // (records of no bytes)
		std::vector<uint64_t> meta(4 * (size_t)n_ref + 1, 0);
		t.meta = meta.data();
		if ((rc = bai_serialise(t, bytes))) return rc;
		st.bai_bytes = (int64_t)bytes->size();
		if (bs) *bs = st;
		return 0;
	}
	hipStream_t q = c->stream;
	if (!parsed && ((rc = bai_stage_parse_begin(s, c, n, n_blocks, n_ref)) || (rc = bai_stage_parse(s, c, 0, n, addr, idx, out_off, n_ref)))) return rc;
	int *n_coor_dev = (int*)(s->err.as<uint8_t>() + 8);
	hipLaunchKernelGGL(k_bai_heads, dim3(grid_of(n)), dim3(256), 0, q, n, s->rk.as<uint64_t>(), s->head.as<int>(), s->first.as<int>(), s->last.as<int>(), n_coor_dev);
	if ((rc = launched()) || (rc = launch_scan(s->head.as<int>(), s->hscan.as<int64_t>(), n, c->d_scan, q)) ||
	    (rc = launch_scan(s->mlen.as<int>(), s->coff.as<int64_t>(), (int)n_blocks, c->d_scan, q))) return rc;
	// ---- the first of two read-backs: refusals, the chunks before the join, the windows of every reference
	uint64_t h_err[2] = { 0, 0 }; int64_t m64 = 0, file_end = 0;
	int *h_top = (int*)s->h_top.p;
	HIP_TRY(hipMemcpyAsync(h_err, s->err.p, 16, hipMemcpyDeviceToHost, q));
	HIP_TRY(hipMemcpyAsync(&m64, s->hscan.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, q));
	HIP_TRY(hipMemcpyAsync(&file_end, s->coff.as<int64_t>() + n_blocks, 8, hipMemcpyDeviceToHost, q));
	if (n_ref) HIP_TRY(hipMemcpyAsync(h_top, s->top.p, (size_t)n_ref * 4, hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	if (h_err[0] != ~0ull) return (h_err[0] & 0xff) == BAI_BAD ? BWAHIP_EINVAL : BWAHIP_ECAPACITY;
	if (base + file_end >= (1ll << 48)) return BWAHIP_ECAPACITY;   // a virtual offset has 48 bits for the file offset
	const int n_coor = (int)(h_err[1] & 0xffffffffu);
	const int m = (int)m64;
	if (m64 < 0 || m64 > n || n_coor < 0 || n_coor > n) return BWAHIP_EINTERNAL;
	for (int32_t r = 0; r < n_ref; ++r) lin_off[(size_t)r + 1] = lin_off[(size_t)r] + (h_top[r] <= TOP ? TOP + 1 - h_top[r] : 0);
	const int64_t n_win = lin_off[(size_t)n_ref];
	const size_t M = (size_t)m, W = (size_t)n_win;
	const size_t tab_words = 1 + 4 * (size_t)n_ref + W + 3 * M;
	if ((rc = s->tab.ensure(tab_words * 8)) || (rc = s->h_tab.ensure(tab_words * 8)) || (rc = s->lin.ensure((W ? W : 1) * 8)) || (rc = dev_upload(s->lin_off, lin_off.data(), lin_off.size() * 8, q))) return rc;
	uint64_t *tab = s->tab.as<uint64_t>();
	uint64_t *d_meta = tab + 1, *d_lin = d_meta + 4 * (size_t)n_ref, *d_okey = d_lin + W, *d_obeg = d_okey + M, *d_oend = d_obeg + M;
	HIP_TRY(hipMemsetAsync(tab, 0, 8, q));
	// ---- chunks
	if (m) {
		BamSort &b = c->bs;
		if ((rc = b.keys[0].ensure(M * 8)) || (rc = b.keys[1].ensure(M * 8)) || (rc = b.idx[0].ensure(M * 4)) || (rc = b.idx[1].ensure(M * 4)) ||
		    (rc = s->cbeg.ensure(M * 8)) || (rc = s->cend.ensure(M * 8)) || (rc = s->keep.ensure(M * 4)) || (rc = s->kscan.ensure((M + 1) * 8))) return rc;
		hipLaunchKernelGGL(k_bai_chunks, dim3(grid_of(n)), dim3(256), 0, q, n, s->rk.as<uint64_t>(), s->hscan.as<int64_t>(), out_off, total, s->coff.as<int64_t>(), n_blocks, base,
		                   b.keys[0].as<uint64_t>(), s->cbeg.as<uint64_t>(), s->cend.as<uint64_t>());
		int cur = 0;
		if ((rc = launched()) || (rc = bam_sort_iota(b.idx[0].as<unsigned>(), m, q)) || (rc = bam_sort_radix(c, m, 48, &cur))) return rc;
		hipLaunchKernelGGL(k_bai_join, dim3(grid_of(m)), dim3(256), 0, q, m, b.keys[cur].as<uint64_t>(), b.idx[cur].as<unsigned>(), s->cbeg.as<uint64_t>(), s->cend.as<uint64_t>(), s->keep.as<int>());
		if ((rc = launched()) || (rc = launch_scan(s->keep.as<int>(), s->kscan.as<int64_t>(), m, c->d_scan, q))) return rc;
		hipLaunchKernelGGL(k_bai_compact, dim3(grid_of(m)), dim3(256), 0, q, m, b.keys[cur].as<uint64_t>(), b.idx[cur].as<unsigned>(), s->cbeg.as<uint64_t>(), s->cend.as<uint64_t>(), s->keep.as<int>(),
		                   s->kscan.as<int64_t>(), d_okey, d_obeg, d_oend, tab);
		if ((rc = launched())) return rc;
	}
	// ---- linear index, metadata
	if (n_win) {
		HIP_TRY(hipMemsetAsync(s->lin.p, 0xff, W * 8, q));
		hipLaunchKernelGGL(k_bai_lin, dim3(grid_of(n)), dim3(256), 0, q, n, s->rk.as<uint64_t>(), s->pos.as<int>(), s->end.as<int>(), out_off, total, s->coff.as<int64_t>(), n_blocks, base,
		                   s->lin_off.as<int64_t>(), s->lin.as<unsigned long long>());
		if ((rc = launched())) return rc;
		hipLaunchKernelGGL(k_bai_backfill, dim3(grid_of(n_win)), dim3(256), 0, q, n_win, s->lin.as<unsigned long long>(), d_lin);
		if ((rc = launched())) return rc;
	}
	if (n_ref) {
		hipLaunchKernelGGL(k_bai_meta, dim3(grid_of(n_ref)), dim3(256), 0, q, (int)n_ref, s->first.as<int>(), s->last.as<int>(), s->n_unm.as<unsigned>(), out_off, total, s->coff.as<int64_t>(), n_blocks,
		                   base, d_meta);
		if ((rc = launched())) return rc;
	}
	HIP_TRY(hipEventRecord(s->ev[1], q));
	// ---- the compact tables, in one download
	uint64_t *h = (uint64_t*)s->h_tab.p;
	HIP_TRY(hipMemcpyAsync(h, tab, tab_words * 8, hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	if (h[0] > (uint64_t)m || (m && !h[0])) return BWAHIP_EINTERNAL;
	t.n_chunks = (int64_t)h[0]; t.meta = h + 1; t.lin = h + 1 + 4 * (size_t)n_ref;
	t.ckey = t.lin + W; t.cbeg = t.ckey + M; t.cend = t.cbeg + M;
	t.n_no_coor = (uint64_t)(n - n_coor);
	if ((rc = bai_serialise(t, bytes))) return rc == BWAHIP_EINVAL ? BWAHIP_EINTERNAL : rc;
	float ms = 0;
	if (hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) st.index_ms = ms;
	st.n_chunks = t.n_chunks; st.n_windows = n_win; st.n_no_coor = (int64_t)t.n_no_coor; st.bai_bytes = (int64_t)bytes->size(); st.hbm_bytes = (int64_t)s->hbm.bytes;
	if (bs) *bs = st;
	return 0;
}

// Exactly the stage above on the caller's records and member lengths: the records are uploaded as one run, their addresses and the
// identity order stand for the merger's source table and sort
extern "C" int bwahip_kat_bai(bwahip_ctx *c, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, const int32_t *member_len, int64_t n_members, int64_t first_member_offset,
                              int32_t n_ref, uint8_t *out, int64_t out_cap, int64_t *out_len)
{
	if (!c || !out_len || n_rec < 0 || n_rec > 0x7fffffffll || n_members < 0 || n_ref < 0 || first_member_offset < 0 || first_member_offset >= (1ll << 48) || out_cap < 0 ||
	    (out_cap && !out) || (n_rec && (!rec || !rec_off)) || (n_members && !member_len)) return BWAHIP_EINVAL;
	*out_len = 0;
	int64_t total = 0;
	for (int64_t i = 0; i < n_rec; ++i) { if (rec_off[i] < 0 || rec_off[i + 1] < rec_off[i]) return BWAHIP_EINVAL; }
	if (n_rec) total = rec_off[n_rec] - rec_off[0];
	if (n_members != bgzf_blocks(total)) return BWAHIP_EINVAL;
	for (int64_t b = 0; b < n_members; ++b) if (member_len[b] < 1 || member_len[b] > 65536) return BWAHIP_EINVAL;
	if (n_rec && total == 0) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	BaiStage s;
	const int n = (int)n_rec;
	int rc, *d_mlen = nullptr;
	if (n) {
		if ((rc = bai_stage_members(&s, n_members, &d_mlen)) || (rc = s.rec.ensure((size_t)rec_off[n_rec])) || (rc = s.addr.ensure((size_t)n * 8)) || (rc = s.idx.ensure((size_t)n * 4)) ||
		    (rc = s.off.ensure(((size_t)n + 1) * 16))) return rc;
		int64_t *d_rec_off = s.off.as<int64_t>() + n + 1;           // the caller's offsets behind the stream's
		HIP_TRY(hipMemcpyAsync(s.rec.p, rec, (size_t)rec_off[n_rec], hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d_rec_off, rec_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d_mlen, member_len, (size_t)n_members * 4, hipMemcpyHostToDevice, c->stream));
		hipLaunchKernelGGL(k_bai_addr, dim3(grid_of((int64_t)n + 1)), dim3(256), 0, c->stream, n, s.rec.as<uint8_t>(), d_rec_off, s.addr.as<const uint8_t*>(), s.off.as<int64_t>());
		if ((rc = launched()) || (rc = bam_sort_iota(s.idx.as<unsigned>(), n, c->stream))) return rc;
	}
	std::vector<uint8_t> bytes;
	rc = bai_stage_run(&s, c, n, s.addr.as<const uint8_t*>(), s.idx.as<unsigned>(), s.off.as<int64_t>(), total, n_members, first_member_offset, n_ref, &bytes, nullptr);
	(void)hipStreamSynchronize(c->stream);                         // nothing of the stage's buffers is in use when they go
	if (rc) return rc;
	*out_len = (int64_t)bytes.size();
	if (*out_len > out_cap) return BWAHIP_ECAPACITY;
	memcpy(out, bytes.data(), bytes.size());
	return 0;
}
