// K9h -- the QC summary and the depth of coverage of the device-merged, coordinate-sorted BAM file, where the runs lie.  The
// rule is in include/bwahip.h; what one record counts for is qc_tables.h, shared with the host builder.  All on the context's stream:
//
//   clear          the tables, the error word and the difference array (len + 1 slots per reference, padded to whole tiles of 2048);
//   records        k_qc_rec: one thread per record of a run -- qc_parse (every field bounded by the record's length); the first offending
//                  record through one 64-bit atomicMin; the 33 counters and the per-reference pairs by ballots, one atomic per wavefront
//                  and counter (neighbours of a sorted file hit the same ones); the mapq and insert-size histograms in LDS, flushed per
//                  workgroup; the covered intervals of the CIGAR as +1 / -1 into the difference array (32-bit atomicAdd, int64 index).
//                  Both ends of an interval lie in its reference's slots, so every reference sums to zero and one prefix sum over
//                  the whole array is right across references;
//   scan           k_qc_tile_sum (a tile's sum), launch_scan over the tile sums (a prefix is a depth: it fits 32 bits), k_qc_tile_scan:
//                  the tile again from its prefix, a wavefront scan by __shfl_up -- the depth of every base feeds the depth histogram
//                  (LDS, one flush per workgroup; depth 0 is counted, not added one by one), the reference's covered bases and the
//                  windows: a workgroup walks consecutive tiles and adds what it gathered when the reference or the window changes (a
//                  window of at least a tile), a smaller window gets a segmented reduction by __shfl_xor and one 64-bit atomicAdd (two
//                  for a window of half a tile).  The slot behind
//                  the last base and the padding are masked out.  No kernel waits for another workgroup;
//   one download   of the compact tables, which go through qc_serialise (qc_host.cpp), the host builder's serialiser.
//
// Sums and a minimum: the result does not depend on the order in which wavefronts run.  __shared__ arrays are indexed inside the kernel
// that declares them; no pointer into LDS is passed on.
#include "ctx_internal.h"
#include "qc_tables.h"
#include "sidecar_host.h"

namespace {

__global__ __launch_bounds__(256) void k_qc_rec(const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0, int n_ref, const int64_t *ref_len,
                                                const int64_t *tile0, bwahip_qc_opt_t opt, unsigned long long *tab, int *diff, unsigned long long *err)
{
	__shared__ unsigned h_mapq[256], h_isize[1025];
	const int t = threadIdx.x, lane = t & 63;
	for (int k = t; k < 1025; k += 256) { h_isize[k] = 0; if (k < 256) h_mapq[k] = 0; }
	__syncthreads();
	const int64_t i = (int64_t)blockIdx.x * 256 + t;
	QcRec r;
	r.ref = -1; r.pos = 0; r.next_ref = -1; r.tlen = 0; r.flag = 0; r.mapq = 0; r.cig = nullptr; r.n_cigar = 0;
	bool live = false;
	if (i < n_rec) {
		const int64_t o = off[i], e = off[i + 1];
		live = o >= 0 && e >= o && e <= len && qc_parse(rec + o, e - o, n_ref, &r);
		if (!live) atomicMin(err, (unsigned long long)(ord0 + i) << 8 | 1u);   // the first offending record decides
	}
	// ---- the counters: every lane of the wavefront is here
	const uint32_t cat = live ? qc_categories(r) : 0u;
	const bool fail = (r.flag & 0x200) != 0;
	for (int q = 0; q < 2; ++q)
		for (int k = 0; k < 16; ++k) {
			const unsigned long long b = __ballot((cat >> k & 1) && fail == (q != 0));
			if (lane == 0 && b) atomicAdd(&tab[QC_COUNT + 16 * q + k], (unsigned long long)__popcll(b));
		}
	{
		const unsigned long long b = __ballot(live && r.ref < 0);
		if (lane == 0 && b) atomicAdd(&tab[QC_NO_COOR], (unsigned long long)__popcll(b));
	}
	// ---- the per-reference pairs: one round per reference the wavefront holds (one or two in a sorted file)
	const int my_ref = live ? r.ref : -1;
	const bool unm = (r.flag & 0x4) != 0;
	unsigned long long pend = __ballot(my_ref >= 0);
	while (pend) {
		const int lead = __ffsll((long long)pend) - 1;
		const int ref = __shfl(my_ref, lead);
		const bool same = my_ref == ref;
		const unsigned long long bm = __ballot(same && !unm), bu = __ballot(same && unm);
		if (lane == lead) {
			if (bm) atomicAdd(&tab[QC_FIXED + QC_PER_REF * (int64_t)ref], (unsigned long long)__popcll(bm));
			if (bu) atomicAdd(&tab[QC_FIXED + QC_PER_REF * (int64_t)ref + 1], (unsigned long long)__popcll(bu));
		}
		pend &= ~(bm | bu);
	}
	// ---- the histograms, private to the workgroup
	if (live && qc_in_mapq_hist(r)) atomicAdd(&h_mapq[r.mapq], 1u);
	if (live && qc_in_isize_hist(r)) atomicAdd(&h_isize[r.tlen < 1024 ? r.tlen : 1024], 1u);
	// ---- coverage
	if (live && qc_covers(r, opt)) {
		int *d = diff + tile0[r.ref] * QC_TILE;
		qc_intervals(r, ref_len[r.ref], [d](int64_t a, int64_t b) { atomicAdd(d + a, 1); atomicAdd(d + b, -1); });   // 0 <= a < b <= len: within the reference's len + 1 slots
	}
	__syncthreads();
	for (int k = t; k < 1025; k += 256) {
		if (k < 256 && h_mapq[k]) atomicAdd(&tab[QC_MAPQ + k], (unsigned long long)h_mapq[k]);
		if (h_isize[k]) atomicAdd(&tab[QC_ISIZE + k], (unsigned long long)h_isize[k]);
	}
}

// A workgroup takes `chunk` consecutive tiles, one after the other: 256 threads x 8 slots each
__global__ __launch_bounds__(256) void k_qc_tile_sum(const int *diff, int *tile_sum, int n_tiles, int chunk)
{
	__shared__ int part[4];
	const int64_t first = (int64_t)blockIdx.x * chunk, last = first + chunk < n_tiles ? first + chunk : n_tiles;
	for (int64_t tile = first; tile < last; ++tile) {
		const int4 *p = reinterpret_cast<const int4*>(diff + tile * QC_TILE + threadIdx.x * 8);
		const int4 a = p[0], b = p[1];
		int s = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
		for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
		if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
		__syncthreads();
		if (threadIdx.x == 0) tile_sum[tile] = part[0] + part[1] + part[2] + part[3];
		__syncthreads();                                            // part is written again
	}
}

// tile_pref: the exclusive scan of the tile sums.  tab: the tables (depth histogram, covered bases); win: the windows of all references.
// Thread 0 keeps the bases of depth 0, the reference's covered bases and the sum of a window of at least a tile in registers from tile
// to tile and adds them to the tables when the reference or the window changes: a handful of atomics per workgroup, not one per tile on
// the same few addresses.
__global__ __launch_bounds__(256) void k_qc_tile_scan(const int *diff, const int64_t *tile_pref, const int *tile_ref, const int64_t *ref_len, const int64_t *tile0,
                                                      const int64_t *win_off, int ws, unsigned long long *tab, unsigned long long *win, int n_tiles, int chunk)
{
	__shared__ unsigned hist[256];
	__shared__ int wave_tot[4];
	__shared__ unsigned long long red_sum[4];
	__shared__ unsigned red_cnt[4];
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
	hist[t] = 0;
	__syncthreads();
	unsigned long long acc_zero = 0, acc_cov = 0, acc_win = 0;      // thread 0 alone
	int acc_ref = -1; int64_t acc_w = -1;                           // the reference of acc_cov, the window (among all references') of acc_win
	const int64_t first = (int64_t)blockIdx.x * chunk, last = first + chunk < n_tiles ? first + chunk : n_tiles;
	for (int64_t tile = first; tile < last; ++tile) {
		const int ref = tile_ref[tile];
		const int64_t L = ref_len[ref];
		const int64_t xt = (tile - tile0[ref]) * QC_TILE, x0 = xt + t * 8;   // the first base of the tile, of this thread
		const int4 *p = reinterpret_cast<const int4*>(diff + tile * QC_TILE + t * 8);
		const int4 a = p[0], b = p[1];
		int incl[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
		for (int j = 1; j < 8; ++j) incl[j] += incl[j - 1];
		int scan = incl[7];
		for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(scan, d); if (lane >= d) scan += y; }
		if (lane == 63) wave_tot[wv] = scan;
		__syncthreads();
		int before = (int)tile_pref[tile] + scan - incl[7];
		for (int w = 0; w < wv; ++w) before += wave_tot[w];
		unsigned cov = 0, n_valid = 0, run_n = 0;
		int run_bin = 0;
		unsigned long long sum = 0;
#pragma unroll
		for (int j = 0; j < 8; ++j) {
			if (x0 + j >= L) continue;                                 // the slot behind the last base, the padding
			const int d = before + incl[j];
			++n_valid;
			if (d <= 0) continue;
			++cov; sum += (unsigned long long)d;
			const int bin = d < 255 ? d : 255;
			if (bin != run_bin) { if (run_n) atomicAdd(&hist[run_bin], run_n); run_bin = bin; run_n = 0; }
			++run_n;
		}
		if (run_n) atomicAdd(&hist[run_bin], run_n);
		if (ws < 11) {                                                 // windows smaller than the tile: 2 .. 128 threads each, aligned
			const int g = (1 << (ws - 3)) < 64 ? 1 << (ws - 3) : 64;
			unsigned long long s = sum;
			for (int d = 1; d < g; d <<= 1) s += __shfl_xor(s, d);
			if ((lane & (g - 1)) == 0 && x0 < L && s) atomicAdd(&win[win_off[ref] + (x0 >> ws)], s);
		}
		unsigned cnt = cov | n_valid << 16;                           // at most 2048 each in the whole tile
		for (int d = 32; d; d >>= 1) { cnt += __shfl_xor(cnt, d); sum += __shfl_xor(sum, d); }
		if (lane == 0) { red_cnt[wv] = cnt; red_sum[wv] = sum; }
		__syncthreads();
		if (t == 0) {
			cnt = red_cnt[0] + red_cnt[1] + red_cnt[2] + red_cnt[3]; sum = red_sum[0] + red_sum[1] + red_sum[2] + red_sum[3];
			const unsigned c = cnt & 0xffff, v = cnt >> 16;
			if (ref != acc_ref) { if (acc_cov) atomicAdd(&tab[QC_FIXED + QC_PER_REF * (int64_t)acc_ref + 2], acc_cov); acc_ref = ref; acc_cov = 0; }
			acc_cov += c; acc_zero += v - c;
			if (ws >= 11 && sum) {                                      // sum != 0: the tile has a base, so the window exists
				const int64_t w = win_off[ref] + (xt >> ws);
				if (w != acc_w) { if (acc_win) atomicAdd(&win[acc_w], acc_win); acc_w = w; acc_win = 0; }
				acc_win += sum;
			}
		}
		__syncthreads();                                            // wave_tot, red_cnt and red_sum are written again
	}
	if (t == 0) {
		if (acc_cov) atomicAdd(&tab[QC_FIXED + QC_PER_REF * (int64_t)acc_ref + 2], acc_cov);
		if (acc_zero) atomicAdd(&tab[QC_DEPTH], acc_zero);
		if (acc_win) atomicAdd(&win[acc_w], acc_win);
	} else if (hist[t]) atomicAdd(&tab[QC_DEPTH + t], (unsigned long long)hist[t]);   // (the loop's last barrier is behind every add to hist)
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV; }

} // namespace

// The stage's buffers: counted by bwahip_qc_hbm_need (qc_host.cpp)
struct QcStage final : RecordStage {
	Tally hbm;
	DevBuf diff{hbm}, tile_sum{hbm}, tile_pref{hbm}, tile_ref{hbm}, ref_tab{hbm}, tab{hbm}, err{hbm};
	HostBuf h_tab;
	Event ev[4];                                                   // begin, cleared, records done, end
	// what qc_stage_set gave
	bwahip_qc_opt_t opt = { 14, 1796, 0 };
	std::vector<int64_t> ref_len;
	int32_t n_ref = 0;
	bwahip_qc_stats_t *stats = nullptr;
	// the layout of the call in flight
	std::vector<int64_t> h_ref_tab;                                // lengths | first tile (n_ref + 1) | first window (n_ref + 1)
	std::vector<int> h_tile_ref;
	int64_t n_tiles = 0, n_win = 0, n_records = 0;
	const int64_t *d_len() const { return ref_tab.as<int64_t>(); }
	const int64_t *d_tile0() const { return ref_tab.as<int64_t>() + n_ref; }
	const int64_t *d_win_off() const { return ref_tab.as<int64_t>() + 2 * (size_t)n_ref + 1; }
	unsigned long long *d_win() const { return tab.as<unsigned long long>() + QC_FIXED + QC_PER_REF * (size_t)n_ref; }
	size_t tab_words() const { return (size_t)QC_FIXED + QC_PER_REF * (size_t)n_ref + (size_t)n_win; }
	int64_t hbm_need(int64_t) const override
	{
		int64_t sum = 0, windows = 0;
		for (int64_t L : ref_len) { sum += L; windows += qc_windows(L, opt.window_shift); }
		return bwahip_qc_hbm_need(n_ref, sum, windows, 0);
	}
	int begin(bwahip_ctx *c, int64_t n_records) override;
	int records(bwahip_ctx *c, const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0) override;
	int done(bwahip_ctx *c) override;
	int write() override { return write_all(fd, bytes.data(), (int64_t)bytes.size(), "writing the QC summary"); }
	bool takes_windows() const override { return true; }
};

RecordStage *qc_stage_new() { return new QcStage; }

void qc_stage_set(RecordStage *rs, const bwahip_qc_opt_t &opt, int32_t n_ref, const int64_t *ref_len, int fd, bwahip_qc_stats_t *qs)
{
	QcStage *s = static_cast<QcStage*>(rs);
	s->opt = opt; s->n_ref = n_ref; s->ref_len.assign(ref_len, ref_len + n_ref); s->fd = fd; s->stats = qs;
}

int QcStage::begin(bwahip_ctx *c, int64_t n_records_)
{
	if (!c || n_records_ < 0) return BWAHIP_EINVAL;
	int rc;
	n_records = n_records_;
	h_ref_tab.assign(3 * (size_t)n_ref + 2, 0);
	int64_t *tile0 = h_ref_tab.data() + n_ref, *win_off = tile0 + n_ref + 1;
	for (int32_t r = 0; r < n_ref; ++r) {
		h_ref_tab[(size_t)r] = ref_len[r];
		tile0[r + 1] = tile0[r] + (ref_len[r] + 1 + QC_TILE - 1) / QC_TILE;
		win_off[r + 1] = win_off[r] + qc_windows(ref_len[r], opt.window_shift);
	}
	n_tiles = tile0[n_ref]; n_win = win_off[n_ref];
	if (n_tiles > 0x7fffffffll) return BWAHIP_ECAPACITY;         // the scan of the tile sums takes an int
	if (!n_records) return 0;                                      // no record: nothing to launch, finish writes the empty summary
	h_tile_ref.resize((size_t)n_tiles);
	for (int32_t r = 0; r < n_ref; ++r) for (int64_t k = tile0[r]; k < tile0[r + 1]; ++k) h_tile_ref[(size_t)k] = r;
	HIP_TRY(hipSetDevice(c->device));
	for (auto &e : ev) if (!e && (rc = e.make())) return rc;
	hipStream_t q = c->stream;
	const size_t T = (size_t)n_tiles;                           // (0 without a reference: the records are still judged and counted)
	if ((rc = diff.ensure((T ? T : 1) * QC_TILE * 4)) || (rc = tile_sum.ensure(T * 4)) || (rc = tile_pref.ensure((T + 1) * 8)) || (rc = tab.ensure(tab_words() * 8)) ||
	    (rc = err.ensure(8)) || (rc = h_tab.ensure(tab_words() * 8 + 8))) return rc;
	HIP_TRY(hipEventRecord(ev[0], q));
	if ((rc = dev_upload(ref_tab, h_ref_tab.data(), h_ref_tab.size() * 8, q)) || (rc = dev_upload(tile_ref, h_tile_ref.data(), T * 4, q))) return rc;
	if (T) HIP_TRY(hipMemsetAsync(diff.p, 0, T * QC_TILE * 4, q));
	HIP_TRY(hipMemsetAsync(tab.p, 0, tab_words() * 8, q));
	HIP_TRY(hipMemsetAsync(err.p, 0xff, 8, q));
	HIP_TRY(hipEventRecord(ev[1], q));
	return 0;
}

// n_rec records of one run: record i = rec[off[i] .. off[i+1]) within the run's `len` bytes; ord0: the ordinal of its first record in the order given
int QcStage::records(bwahip_ctx *c, const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0)
{
	if (!n_rec) return 0;
	if (n_rec > 0x7fffffffll) return BWAHIP_ECAPACITY;
	hipLaunchKernelGGL(k_qc_rec, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, c->stream, rec, off, n_rec, len, ord0, (int)n_ref, d_len(), d_tile0(), opt,
	                   tab.as<unsigned long long>(), diff.as<int>(), err.as<unsigned long long>());
	return launched();
}

// the scan, the download (awaited) and the summary's bytes; BWAHIP_EINVAL when a record was refused
int QcStage::done(bwahip_ctx *c)
{
	bwahip_qc_stats_t st;
	memset(&st, 0, sizeof st);
	QcTables t;
	t.n_ref = n_ref; t.ref_len = ref_len.data(); t.opt = opt;
	int rc;
	if (!n_records) {                                           // every base has depth 0
		std::vector<uint64_t> z(tab_words(), 0);
		for (int64_t L : ref_len) z[QC_DEPTH] += (uint64_t)L;
		t.fixed = z.data(); t.per_ref = z.data() + QC_FIXED; t.win = z.data() + QC_FIXED + QC_PER_REF * (size_t)n_ref;
		if ((rc = qc_serialise(t, &bytes))) return rc;
	} else {
		hipStream_t q = c->stream;
		HIP_TRY(hipEventRecord(ev[2], q));
		const unsigned T = (unsigned)n_tiles;
		if (T) {
			const int chunk = T > 4 * 8192 ? (int)((T + 8191) / 8192) : 4;   // up to 8192 workgroups, each at least four tiles
			const unsigned grid = (T + (unsigned)chunk - 1) / (unsigned)chunk;
			hipLaunchKernelGGL(k_qc_tile_sum, dim3(grid), dim3(256), 0, q, diff.as<int>(), tile_sum.as<int>(), (int)T, chunk);
			if ((rc = launched()) || (rc = launch_scan(tile_sum.as<int>(), tile_pref.as<int64_t>(), (int)T, c->d_scan, q))) return rc;
			hipLaunchKernelGGL(k_qc_tile_scan, dim3(grid), dim3(256), 0, q, diff.as<int>(), tile_pref.as<int64_t>(), tile_ref.as<int>(), d_len(), d_tile0(), d_win_off(),
			                   opt.window_shift, tab.as<unsigned long long>(), d_win(), (int)T, chunk);
			if ((rc = launched())) return rc;
		}
		HIP_TRY(hipEventRecord(ev[3], q));
		uint64_t *h = (uint64_t*)h_tab.p;
		HIP_TRY(hipMemcpyAsync(h, tab.p, tab_words() * 8, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipMemcpyAsync(h + tab_words(), err.p, 8, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (h[tab_words()] != ~0ull) return BWAHIP_EINVAL;
		t.fixed = h; t.per_ref = h + QC_FIXED; t.win = h + QC_FIXED + QC_PER_REF * (size_t)n_ref;
		if ((rc = qc_serialise(t, &bytes))) return rc == BWAHIP_EINVAL ? BWAHIP_EINTERNAL : rc;
		float ms = 0;
		if (hipEventElapsedTime(&ms, ev[0], ev[3]) == hipSuccess) st.qc_ms = ms;
		if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) st.record_ms = ms;
		if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) st.scan_ms = ms;
		st.hbm_bytes = (int64_t)hbm.bytes;
	}
	st.n_windows = n_win; st.qc_bytes = (int64_t)bytes.size();
	if (stats) *stats = st;
	return 0;
}

// Exactly the stage above on the caller's records: they are uploaded as one run
extern "C" int bwahip_kat_qc(bwahip_ctx *c, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, int32_t n_ref, const int64_t *ref_len, const bwahip_qc_opt_t *opt,
                             uint8_t *out, int64_t out_cap, int64_t *out_len)
{
	if (!c || !out_len || n_rec < 0 || n_rec > 0x7fffffffll || out_cap < 0 || (out_cap && !out) || (n_rec && (!rec || !rec_off))) return BWAHIP_EINVAL;
	*out_len = 0;
	bwahip_qc_opt_t o;
	int rc;
	if ((rc = qc_resolve(opt, &o)) || (rc = check_refs(n_ref, ref_len, nullptr, NO_SUM_CAP))) return rc;
	QcStage s;
	qc_stage_set(&s, o, n_ref, ref_len, -1, nullptr);
	return record_stage_kat(&s, c, rec, rec_off, n_rec, out, out_cap, out_len);
}
