// K9e -- the merge of sorted runs on the GPU: what bwahip_bam_merger_* (bam_sort_host.cpp) does on one host thread in front of host zlib,
// for runs that stay in HBM.  A run = the sorted records of one batch, its keys and its n_rec + 1 record offsets, each in a device buffer
// of its own; no record is ever parsed.  finish():
//
//   order          the runs' keys, concatenated in run-number order, through the stable radix sort of k_bamsort.hip with the ordinals
//                  0 .. n - 1: concatenation order is (run, position in the run), the sort is stable, so the result is the order of the
//                  host merger's k-way merge -- (key, run_no, position) -- without a merge kernel.  All 64 bits of the key count, as in
//                  the host merger's comparison (the sort skips the digits that are the same in all keys);
//   source table   k_src_table: per ordinal the absolute device address of the record and its length (the run by binary search in the
//                  table of the runs' first ordinals);
//   output offsets k_sorted_len: the lengths in sorted order; an exclusive scan.  The last offset must be the sum of the runs' bytes;
//   pieces         the sorted byte stream is never made whole: it is cut every piece_blocks x 65 280 bytes, k_piece_first finds the
//                  record that holds every cut (binary search over the output offsets), one read-back brings them to the host;
//   windowed       k_gather_window: k_gather_copy's shape (16 lanes per record, single bytes to the destination's 16-byte boundary,
//   gather         unaligned 16-byte loads and aligned 16-byte stores, the ragged end), clipped to the piece's byte range at both ends;
//   deflate        bgzf_deflate (k_bgzf.hip) on the piece as it is.  Pieces are whole multiples of a block's input and blocks are
//                  independent, so the members are those of one deflate stage over all sorted records.
//
// Two piece inputs and two piece outputs: the gather and the deflate of piece k are queued on the context's stream while the 16-byte
// total and then the members of piece k - 1 come back on the copy stream and are written.  No kernel here uses LDS or atomics.
//
// Beside the members a finish runs the stages its FinishPlan names (ctx_internal.h) -- duplicate marking (k_markdup.hip: one bit of a record
// changes and no key), the BAI index (k_bai.hip, after the last piece) -- and the merger's armed record stages (RecordStage, ctx_internal.h: the
// QC summary, k_qc.hip, then the pileup, k_pileup.hip, resident runs only, then the recalibration table, k_recal.hip; they read and change nothing).  Marking and the record stages read
// every record.  That is the records pass: a resident run's records pass before the order is made, marking first, one stage after the other over
// all runs, and each stage is awaited there.  A spilled run (bwahip_bam_devmerger_set_spill, k_bamspill.hip) keeps its record bytes in a
// host-side store; they are staged one window of pieces at a time (spill_plan.h), the gather finds them in the staging buffer, and the slices
// pass the stages -- and the index parse -- in their window, so the await is deferred behind the last window.  A merger without a stage
// and without a spilled run queues exactly what is described above.  Finish::run is the list of steps, each a function of its own: the
// checks; the records pass over resident runs; the order; the source table and output offsets; the piece cuts; the piece buffers; the window
// plan, if spilled; the piece loop; the deferred await; the index; the record stages' files; the stats (an empty merger: the first two and
// what follows the piece loop).
#include "ctx_internal.h"
#include "bai_tables.h"
#include "qc_tables.h"
#include "pileup_tables.h"
#include "recal_tables.h"
#include "spill_plan.h"
#include "spill_store.h"
#include "sidecar_host.h"
#include <chrono>
#include <map>
#include <mutex>

namespace {

constexpr int64_t BLOCK_IN = 65280;
constexpr int MAX_PIECE_BLOCKS = 4096;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// first[r]: the ordinal of run r's first record (n_runs + 1 entries, the last = n).  Thread = ordinal.  err: offsets that decrease or leave
// the run's bytes (never expected: add() checked the host's, the sort stage produced the device's); such a record counts as empty.
__global__ __launch_bounds__(256) void k_src_table(int n, int n_runs, const int64_t *first, const uint8_t *const *run_rec, const int64_t *const *run_off, const int64_t *run_len,
                                                  const uint8_t **addr, int *len, int *err)
{
	const int g = blockIdx.x * 256 + threadIdx.x;
	if (g >= n) return;
	int lo = 0, hi = n_runs;                                       // the last run whose first ordinal is <= g: it is not empty, because the next one's is > g
	while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (first[mid] <= g) lo = mid; else hi = mid; }
	const int64_t j = g - first[lo];
	const int64_t o0 = run_off[lo][j], o1 = run_off[lo][j + 1];
	const bool ok = o0 >= 0 && o1 >= o0 && o1 <= run_len[lo] && o1 - o0 <= 0x7fffffff;
	if (!ok) *err = 1;                                             // every writer writes 1
	addr[g] = run_rec[lo] + (ok ? o0 : 0);
	len[g] = ok ? (int)(o1 - o0) : 0;
}

__global__ __launch_bounds__(256) void k_sorted_len(const unsigned *idx, const int *len, int n, int *len_sorted)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) len_sorted[i] = len[idx[i]];
}

// first_rec[p], p < n_pieces: the last record (in sorted order) whose first byte is at or before byte p * piece_bytes of the sorted stream --
// the record that holds that byte, or the one that begins there.  out_off: n + 1 offsets, out_off[0] = 0.
__global__ __launch_bounds__(256) void k_piece_first(const int64_t *out_off, int n, int64_t piece_bytes, int n_pieces, int *first_rec)
{
	const int p = blockIdx.x * 256 + threadIdx.x;
	if (p >= n_pieces) return;
	const int64_t b = (int64_t)p * piece_bytes;
	int lo = 0, hi = n;                                            // out_off[lo] <= b < out_off[hi] (b is below the stream's end)
	while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (out_off[mid] <= b) lo = mid; else hi = mid; }
	first_rec[p] = lo;
}

// Records [rec_lo, rec_lo + n_rec) of the sorted order, the bytes of each that fall into [byte_lo, byte_hi) of the sorted stream, to
// dst + (position - byte_lo).  16 lanes per record.  A record may begin before the piece, end behind it, or cover it whole.
__global__ __launch_bounds__(256) void k_gather_window(const uint8_t *const *addr, const unsigned *idx, const int64_t *out_off, int rec_lo, int n_rec, int64_t byte_lo, int64_t byte_hi,
                                                      uint8_t *dst_all)
{
	const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
	const int l = threadIdx.x & 15;
	if (g >= n_rec) return;
	const int64_t o = out_off[rec_lo + g], e = out_off[rec_lo + g + 1];
	const int64_t a = o > byte_lo ? o : byte_lo, b = e < byte_hi ? e : byte_hi;
	if (a >= b) return;
	const uint8_t *src = addr[idx[rec_lo + g]] + (a - o);
	uint8_t *dst = dst_all + (a - byte_lo);
	const int len = (int)(b - a);                                  // at most the piece: 4096 x 65 280 bytes
	int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
	if (head > len) head = len;
	if (l < head) dst[l] = src[l];
	const int body = (len - head) >> 4;
	for (int k = l; k < body; k += 16) {
		uint4 v;
		__builtin_memcpy(&v, src + head + 16 * k, 16);
		*reinterpret_cast<uint4*>(dst + head + 16 * k) = v;
	}
	for (int k = head + 16 * body + l; k < len; k += 16) dst[k] = src[k];
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV; }

// finish()'s buffers beside the context's (bs.keys / bs.idx / bs.hist*, bz.*): counted by bwahip_bam_devmerge_hbm_need below
struct Work {
	Tally hbm;
	DevBuf first{hbm}, run_rec{hbm}, run_off{hbm}, run_len{hbm};   // per run
	DevBuf addr{hbm}, len{hbm}, len_sorted{hbm}, out_off{hbm}, err{hbm};   // per record: 8 + 4 + 4 + 8 bytes
	DevBuf piece_first{hbm};                                       // per piece
	DevBuf in[2] = { DevBuf{hbm}, DevBuf{hbm} }, out[2] = { DevBuf{hbm}, DevBuf{hbm} }, tot[2] = { DevBuf{hbm}, DevBuf{hbm} };   // per piece of piece_blocks blocks: input, members (input + 31 per block), their total
	HostBuf h_out[2], h_tot;
	Event ev_gather[2], ev_deflate[2], ev_done[2], ev_down[2], ev_sort[2];
	int make_events()
	{
		int rc;
		for (Event *set : { ev_gather, ev_deflate, ev_done, ev_down, ev_sort }) for (int k = 0; k < 2; ++k) if (!set[k] && (rc = set[k].make())) return rc;
		return 0;
	}
};

// a merger with spilled runs: the staging of the windows (counted by bwahip_bam_devmerge_spill_hbm_need, k_bamspill.hip)
struct SpillWork {
	Tally hbm;
	DevBuf stage[2] = { DevBuf{hbm}, DevBuf{hbm} }, cut{hbm}, base{hbm}, flags{hbm}, scratch{hbm};   // two windows' slices; per run and window: the cuts, the slices' bases; per run: spilled or not; a counter nobody reads
	HostBuf bounce[2];                                             // file-backed runs: pread lands here, at the slice's place in the window
	Event ev_up0[2], ev_up[2], ev_used[2];                         // a window's upload begun / done (copy stream); its last reader queued (context's stream)
	int make_events()
	{
		int rc;
		for (Event *set : { ev_up0, ev_up, ev_used }) for (int k = 0; k < 2; ++k) if (!set[k] && (rc = set[k].make())) return rc;
		return 0;
	}
};

constexpr int DEFAULT_WINDOW_PIECES = 8;                          // with 1 024 blocks a piece: windows of 535 MB, two staging buffers of that

void *pinned_alloc(size_t bytes, void *ctx)
{
	void *p = hipSetDevice(((bwahip_ctx*)ctx)->device) == hipSuccess ? PinnedMem::alloc(bytes) : nullptr;
	if (p) PinnedMem::count_sync();
	return p;
}
void pinned_free(void *p, size_t bytes, void *) { if (p) { PinnedMem::free(p, bytes); PinnedMem::count_sync(); } }

} // namespace

// The HBM of a device merger: what the runs hold, and what finish() allocates for them -- next to the buffers it counts (Work above, the
// context's BamSort keys / ordinals and Bgzf slots).  Per record: two key and two ordinal buffers of the sort (24), address, length, sorted
// length and output offset (24).  Per block of a piece: two inputs, two outputs (input + 31), the slot, the member's length and offset.
// The deflate stage's per-workgroup words (one workgroup per compute unit, 261 120 bytes each) and the sort's histograms: 64 MiB covers
// 256 compute units.  The working buffers grow with an eighth of slack (DevBuf::ensure); the runs are allocated to size.
extern "C" int64_t bwahip_bam_devmerge_hbm_need(int64_t raw_bytes, int64_t n_records, int64_t n_runs, int piece_blocks)
{
	if (raw_bytes < 0 || n_records < 0 || n_runs < 0 || piece_blocks < 1 || piece_blocks > MAX_PIECE_BLOCKS) return -1;
	const int64_t runs = raw_bytes + 16 * n_records + 8 * n_runs;
	int64_t pb = bgzf_blocks(raw_bytes);
	if (pb > piece_blocks) pb = piece_blocks;
	const int64_t work = 48 * n_records + pb * (4 * BLOCK_IN + 2 * 31 + 65536 + 12) + (64ll << 20);
	return runs + work + work / 8;
}

struct bwahip_bam_devmerger {
	bwahip_ctx *c = nullptr;
	int piece_blocks = 0;
	std::mutex mu;
	std::map<int64_t, DevRun*> runs;                               // by run_no: the order of the concatenation
	int64_t n_records = 0, raw_bytes = 0;
	Work w;
	std::unique_ptr<BaiStage, void (*)(BaiStage*)> bai{ nullptr, bai_stage_free };   // the stages' buffers (k_bai.hip, k_markdup.hip): each made by the first finish that runs the stage
	std::unique_ptr<MarkdupStage> md;
	// The record stages (bwahip_bam_devmerger_set_qc, _set_pileup, _set_recal), in the order a finish runs the armed ones.  They live as long as the merger:
	// what a setter configured and the buffers a finish made stay for the next finish
	std::unique_ptr<RecordStage> qc{ qc_stage_new() }, pu{ pu_stage_new() }, rc{ recal_stage_new() };
	RecordStage *const stages[3] = { qc.get(), pu.get(), rc.get() };
	bool all_take_windows() const { for (const RecordStage *s : stages) if (s->armed && !s->takes_windows()) return false; return true; }
	// spilled runs (bwahip_bam_devmerger_set_spill): the store of their record bytes, the windows' staging
	HostBuf dl_bounce;                                             // bam_devmerger_adopt_spilled: a file-backed run's bytes on their way from HBM
	bool spill_armed = false, added = false; int window_pieces = 0; SpillStore *store = nullptr; SpillWork sw;
	int64_t n_spilled = 0, n_windows = 0; double download_s = 0, upload_ms = 0;
};

int bam_devrun_make(bwahip_ctx *c, const uint8_t *d_rec, int64_t len, const uint64_t *d_keys, const int64_t *d_rec_off, int64_t n_rec, hipStream_t st, DevRun **out)
{
	if (!c || !out || len < 0 || n_rec < 0 || (n_rec && (!d_rec || !d_keys || !d_rec_off)) || (!n_rec && len)) return BWAHIP_EINVAL;
	*out = nullptr;
	HIP_TRY(hipSetDevice(c->device));
	DevRun *r = new DevRun;
	r->n_rec = n_rec; r->len = len; r->device = c->device;
	if (n_rec) {
		int rc;
		if ((rc = r->d_rec.alloc_exact((size_t)len)) || (rc = r->d_keys.alloc_exact((size_t)n_rec * 8)) || (rc = r->d_off.alloc_exact((size_t)(n_rec + 1) * 8))) { bam_devrun_free(r); return rc; }
		hipError_t e = len ? hipMemcpyAsync(r->rec(), d_rec, (size_t)len, hipMemcpyDeviceToDevice, st) : hipSuccess;
		if (e == hipSuccess) e = hipMemcpyAsync(r->keys(), d_keys, (size_t)n_rec * 8, hipMemcpyDeviceToDevice, st);
		if (e == hipSuccess) e = hipMemcpyAsync(r->off(), d_rec_off, (size_t)(n_rec + 1) * 8, hipMemcpyDeviceToDevice, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e != hipSuccess) { fprintf(stderr, "[bwahip] sorted BAM: copying a run failed: %s\n", hipGetErrorString(e)); bam_devrun_free(r); return BWAHIP_ENODEV; }
	}
	*out = r;
	return 0;
}

int bam_devrun_download(const DevRun *r, uint8_t *rec, uint64_t *keys, int64_t *rec_off, hipStream_t st)
{
	if (!r || !rec_off) return BWAHIP_EINVAL;
	if (!r->n_rec) { rec_off[0] = 0; return 0; }
	if (!rec || !keys) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(r->device));
	if (r->len) HIP_TRY(hipMemcpyAsync(rec, r->rec(), (size_t)r->len, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(keys, r->keys(), (size_t)r->n_rec * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(rec_off, r->off(), (size_t)(r->n_rec + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

void bam_devrun_free(DevRun *r)
{
	if (!r) return;
	(void)hipSetDevice(r->device);
	delete r;
}

int bam_devrun_add_dup(DevRun *r, const uint32_t *d_tmpl, const bwahip_dup_desc_t *d_desc, int64_t n_tmpl, hipStream_t st)
{
	if (!r || r->has_dup || n_tmpl < 0 || (r->n_rec && !d_tmpl) || (n_tmpl && !d_desc)) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(r->device));
	DevBuf t, d;                                                   // the run's once both are filled
	int rc;
	if ((r->n_rec && (rc = t.alloc_exact((size_t)r->n_rec * 4))) || (n_tmpl && (rc = d.alloc_exact((size_t)n_tmpl * sizeof *d_desc)))) return rc;
	hipError_t e = r->n_rec ? hipMemcpyAsync(t.p, d_tmpl, (size_t)r->n_rec * 4, hipMemcpyDeviceToDevice, st) : hipSuccess;
	if (e == hipSuccess && n_tmpl) e = hipMemcpyAsync(d.p, d_desc, (size_t)n_tmpl * sizeof *d_desc, hipMemcpyDeviceToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) { fprintf(stderr, "[bwahip] sorted BAM: copying a run's templates failed: %s\n", hipGetErrorString(e)); return BWAHIP_ENODEV; }
	r->d_tmpl = std::move(t); r->d_desc = std::move(d); r->n_tmpl = n_tmpl; r->has_dup = true;
	return 0;
}

int bam_devmerger_adopt(bwahip_bam_devmerger *m, int64_t run_no, DevRun *r)
{
	if (!m || !r || run_no < 0 || r->device != m->c->device) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	if (m->runs.count(run_no)) return BWAHIP_EINVAL;
	if (m->n_records + r->n_rec > 0x7fffffffll) return BWAHIP_ECAPACITY;   // the sort's ordinals are 32-bit and it takes an int
	m->runs[run_no] = r;
	m->n_records += r->n_rec; m->raw_bytes += r->len; m->added = true;
	if (r->spilled) ++m->n_spilled;
	return 0;
}

int bam_devmerger_window_pieces(const bwahip_bam_devmerger *m) { return m && m->spill_armed ? m->window_pieces : 0; }

int bam_devmerger_adopt_spilled(bwahip_bam_devmerger *m, int64_t run_no, DevRun *r, hipStream_t st, int64_t *longest)
{
	if (!m || !r || run_no < 0 || r->spilled || r->device != m->c->device || !m->spill_armed) return BWAHIP_EINVAL;
	{
		std::lock_guard<std::mutex> lk(m->mu);
		if (m->runs.count(run_no)) return BWAHIP_EINVAL;
	}
	HIP_TRY(hipSetDevice(r->device));
	const double t0 = now_s();
	uint8_t *mem = nullptr;
	int rc = spill_store_reserve(m->store, run_no, r->len, &mem);
	if (rc) return rc;
	std::vector<int64_t> h_off((size_t)(r->n_rec ? r->n_rec + 1 : 0));
	hipError_t e = r->n_rec ? hipMemcpyAsync(h_off.data(), r->off(), h_off.size() * 8, hipMemcpyDeviceToHost, st) : hipSuccess;
	if (e == hipSuccess && mem) e = hipMemcpyAsync(mem, r->rec(), (size_t)r->len, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e == hipSuccess && !mem && r->len) {                       // a file: through the pinned bounce buffer, 64 MiB at a time
		const int64_t step = 64ll << 20;
		if (!(rc = m->dl_bounce.ensure((size_t)(r->len < step ? r->len : step))))
			for (int64_t at = 0; at < r->len && !rc && e == hipSuccess; at += step) {
				const int64_t part = r->len - at < step ? r->len - at : step;
				e = hipMemcpyAsync(m->dl_bounce.p, r->rec() + at, (size_t)part, hipMemcpyDeviceToHost, st);
				if (e == hipSuccess) e = hipStreamSynchronize(st);
				if (e == hipSuccess) rc = spill_store_write(m->store, run_no, at, (const uint8_t*)m->dl_bounce.p, part);
			}
	}
	if (e != hipSuccess) { fprintf(stderr, "[bwahip] sorted BAM: downloading a spilled run failed: %s\n", hipGetErrorString(e)); rc = BWAHIP_ENODEV; }
	if (rc) { (void)spill_store_drop(m->store, run_no); return rc; }
	r->spilled = true; r->h_off.swap(h_off);
	if ((rc = bam_devmerger_adopt(m, run_no, r))) { r->spilled = false; r->h_off.clear(); (void)spill_store_drop(m->store, run_no); return rc; }
	r->d_rec.release();                                            // adopted: only now do the record bytes leave HBM
	if (longest) { *longest = 0; for (int64_t i = 0; i < r->n_rec; ++i) if (r->h_off[(size_t)i + 1] - r->h_off[(size_t)i] > *longest) *longest = r->h_off[(size_t)i + 1] - r->h_off[(size_t)i]; }
	std::lock_guard<std::mutex> lk(m->mu);
	m->download_s += now_s() - t0;
	return 0;
}

int bam_devmerger_add_dev(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *d_rec, int64_t len, const uint64_t *d_keys, const int64_t *d_rec_off, int64_t n_rec, hipStream_t st)
{
	if (!m || run_no < 0) return BWAHIP_EINVAL;
	{
		std::lock_guard<std::mutex> lk(m->mu);                      // refused before anything is allocated (adopt checks again under the same lock)
		if (m->runs.count(run_no)) return BWAHIP_EINVAL;
		if (n_rec >= 0 && m->n_records + n_rec > 0x7fffffffll) return BWAHIP_ECAPACITY;
	}
	DevRun *r = nullptr;
	int rc = bam_devrun_make(m->c, d_rec, len, d_keys, d_rec_off, n_rec, st, &r);
	if (rc) return rc;
	if ((rc = bam_devmerger_adopt(m, run_no, r))) bam_devrun_free(r);
	return rc;
}

int bam_devmerger_take_runs(bwahip_bam_devmerger *m, std::vector<std::pair<int64_t, DevRun*>> *out)
{
	if (!m || !out) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	if (m->n_spilled) return BWAHIP_EINVAL;
	out->assign(m->runs.begin(), m->runs.end());
	m->runs.clear(); m->n_records = 0; m->raw_bytes = 0;
	return 0;
}

extern "C" int bwahip_bam_devmerger_open(bwahip_ctx *ctx, int piece_blocks, bwahip_bam_devmerger **out)
{
	if (!out) return BWAHIP_EINVAL;
	*out = nullptr;
	if (!ctx || piece_blocks > MAX_PIECE_BLOCKS) return BWAHIP_EINVAL;
	bwahip_bam_devmerger *m = new bwahip_bam_devmerger;
	m->c = ctx; m->piece_blocks = piece_blocks > 0 ? piece_blocks : ctx->knobs.sorted_piece_blocks;
	*out = m;
	return 0;
}

// tmpl / desc / n_tmpl: bwahip_bam_devmerger_add_dup (with_dup)
static int devmerger_add(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys, const int64_t *rec_off, int64_t n_rec,
                         bool with_dup, const uint32_t *tmpl, const bwahip_dup_desc_t *desc, int64_t n_tmpl, bool spill = false)
{
	if (!m || run_no < 0 || len < 0 || n_rec < 0 || (n_rec && (!rec || !keys || !rec_off)) || (!n_rec && len)) return BWAHIP_EINVAL;
	if (n_rec && (rec_off[0] != 0 || rec_off[n_rec] != len)) return BWAHIP_EINVAL;
	for (int64_t i = 0; i < n_rec; ++i) {
		if (rec_off[i + 1] < rec_off[i]) return BWAHIP_EINVAL;
		if (rec_off[i + 1] - rec_off[i] > 0x7fffffffll) return BWAHIP_ECAPACITY;   // lengths are scanned as int32
	}
	if (with_dup) {                                                // refused before anything is allocated
		if (n_tmpl < 0 || n_tmpl > 0x3fffffffll || (n_rec && !tmpl) || (n_tmpl && !desc)) return BWAHIP_EINVAL;
		for (int64_t i = 0; i < n_rec; ++i) if (tmpl[i] >= (uint64_t)n_tmpl) return BWAHIP_EINVAL;
		for (int64_t i = 0; i < n_tmpl; ++i) if (desc[i].kind > 2) return BWAHIP_EINVAL;
	}
	bwahip_ctx *c = m->c;
	{
		std::lock_guard<std::mutex> lk(m->mu);
		if (m->runs.count(run_no)) return BWAHIP_EINVAL;
		if (m->n_records + n_rec > 0x7fffffffll) return BWAHIP_ECAPACITY;
	}
	HIP_TRY(hipSetDevice(c->device));
	int rc = 0;
	if (spill) {                                                   // the record bytes to the store first: an unusable tmp_dir is refused before anything is allocated
		const double t0 = now_s();
		if ((rc = spill_store_put(m->store, run_no, rec, len))) return rc;
		std::lock_guard<std::mutex> lk(m->mu);
		m->download_s += now_s() - t0;
	}
	DevRun *r = new DevRun;
	r->n_rec = n_rec; r->len = len; r->device = c->device; r->spilled = spill;
	if (spill) r->h_off.assign(rec_off, rec_off + (n_rec ? n_rec + 1 : 0));
	struct Undo { bwahip_bam_devmerger *m; int64_t id; bool on; ~Undo() { if (on) (void)spill_store_drop(m->store, id); } } undo = { m, run_no, spill };   // a refused run leaves the store as it was
	if (n_rec) {
		if ((!spill && (rc = r->d_rec.alloc_exact((size_t)len))) || (rc = r->d_keys.alloc_exact((size_t)n_rec * 8)) || (rc = r->d_off.alloc_exact((size_t)(n_rec + 1) * 8))) { bam_devrun_free(r); return rc; }
		// plain copies: they return when the caller's memory has been read, whatever thread and stream
		hipError_t e = len && !spill ? hipMemcpy(r->rec(), rec, (size_t)len, hipMemcpyHostToDevice) : hipSuccess;
		if (e == hipSuccess) e = hipMemcpy(r->keys(), keys, (size_t)n_rec * 8, hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMemcpy(r->off(), rec_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice);
		if (e == hipSuccess && with_dup && (rc = r->d_tmpl.alloc_exact((size_t)n_rec * 4))) { bam_devrun_free(r); return rc; }
		if (e == hipSuccess && with_dup) e = hipMemcpy(r->tmpl(), tmpl, (size_t)n_rec * 4, hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipDeviceSynchronize();
		if (e != hipSuccess) { fprintf(stderr, "[bwahip] sorted BAM: uploading a run failed: %s\n", hipGetErrorString(e)); bam_devrun_free(r); return BWAHIP_ENODEV; }
	}
	if (with_dup && n_tmpl) {
		if ((rc = r->d_desc.alloc_exact((size_t)n_tmpl * sizeof *desc))) { bam_devrun_free(r); return rc; }
		if (hipMemcpy(r->desc(), desc, (size_t)n_tmpl * sizeof *desc, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { bam_devrun_free(r); return BWAHIP_ENODEV; }
	}
	r->has_dup = with_dup; r->n_tmpl = with_dup ? n_tmpl : 0;
	if ((rc = bam_devmerger_adopt(m, run_no, r))) bam_devrun_free(r);
	else undo.on = false;
	return rc;
}

extern "C" int bwahip_bam_devmerger_add(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys, const int64_t *rec_off, int64_t n_rec)
{
	return devmerger_add(m, run_no, rec, len, keys, rec_off, n_rec, false, nullptr, nullptr, 0);
}

extern "C" int bwahip_bam_devmerger_add_dup(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys, const int64_t *rec_off, int64_t n_rec,
                                            const uint32_t *tmpl, const bwahip_dup_desc_t *desc, int64_t n_tmpl)
{
	return devmerger_add(m, run_no, rec, len, keys, rec_off, n_rec, true, tmpl, desc, n_tmpl);
}

extern "C" int bwahip_bam_devmerger_set_spill(bwahip_bam_devmerger *m, const bwahip_spill_t *in)
{
	if (!m || !in || in->host_budget < 0 || in->window_pieces > 65536) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	if (m->added || m->spill_armed || !m->all_take_windows()) return BWAHIP_EINVAL;   // before the first add, once; the pileup reads resident runs only
	if (!(m->store = spill_store_new(in->host_budget, in->tmp_dir, pinned_alloc, pinned_free, m->c))) return BWAHIP_ENOMEM;
	m->window_pieces = in->window_pieces > 0 ? in->window_pieces : DEFAULT_WINDOW_PIECES;
	m->spill_armed = true;
	return 0;
}

// tmpl == NULL && desc == NULL: a run without descriptors (bwahip_bam_devmerger_add); otherwise bwahip_bam_devmerger_add_dup
extern "C" int bwahip_bam_devmerger_add_spilled(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys, const int64_t *rec_off, int64_t n_rec,
                                                const uint32_t *tmpl, const bwahip_dup_desc_t *desc, int64_t n_tmpl)
{
	if (!m || !m->spill_armed || !m->all_take_windows()) return BWAHIP_EINVAL;
	const bool with_dup = tmpl || desc;
	if (!with_dup && n_tmpl) return BWAHIP_EINVAL;
	return devmerger_add(m, run_no, rec, len, keys, rec_off, n_rec, with_dup, tmpl, desc, n_tmpl, true);
}

extern "C" int bwahip_bam_devmerger_spill_stats(bwahip_bam_devmerger *m, bwahip_spill_t *out)
{
	if (!m || !out) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	out->n_spilled_runs = m->n_spilled; out->first_spilled_run = -1;
	for (auto &kv : m->runs) if (kv.second->spilled) { out->first_spilled_run = kv.first; break; }
	out->host_bytes = spill_store_host_bytes(m->store); out->file_bytes = spill_store_file_bytes(m->store);
	out->n_windows = m->n_windows; out->window_hbm_bytes = (int64_t)m->sw.hbm.bytes;
	out->download_s = m->download_s; out->upload_ms = m->upload_ms;
	return 0;
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------
namespace {

// ---- the stages that read records: marking (k_markdup.hip), then the armed record stages
// Marking's own beginning, on the context's stream: the runs' descriptors concatenated in run order, the decision, the counts
int mark_decide(bwahip_bam_devmerger *m)
{
	bwahip_ctx *c = m->c;
	MarkdupStage &s = *m->md;
	int64_t T = 0;
	for (auto &kv : m->runs) T += kv.second->n_tmpl;
	if (T > 0x3fffffffll) return BWAHIP_ECAPACITY;
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	for (auto &e : s.ev) if (!e && (rc = e.make())) return rc;
	if ((rc = s.desc.ensure((size_t)(T ? T : 1) * sizeof(bwahip_dup_desc_t)))) return rc;
	HIP_TRY(hipEventRecord(s.ev[0], c->stream));
	int64_t at = 0;
	for (auto &kv : m->runs) {
		const DevRun *r = kv.second;
		if (r->n_tmpl) HIP_TRY(hipMemcpyAsync(s.desc.as<bwahip_dup_desc_t>() + at, r->desc(), (size_t)r->n_tmpl * sizeof(bwahip_dup_desc_t), hipMemcpyDeviceToDevice, c->stream));
		at += r->n_tmpl;
	}
	if ((rc = markdup_decide(&s, c, T))) return rc;
	HIP_TRY(hipEventRecord(s.ev[1], c->stream));
	if ((rc = markdup_counters_reset(&s, c))) return rc;
	return markdup_count(&s, c, T);
}

// marking's end: the stream is awaited, the counters come back
int mark_end(bwahip_bam_devmerger *m, bwahip_markdup_stats_t *ms)
{
	bwahip_ctx *c = m->c;
	MarkdupStage &s = *m->md;
	int64_t run_bytes = 0;
	for (auto &kv : m->runs) run_bytes += 4 * kv.second->n_rec + 24 * kv.second->n_tmpl;
	HIP_TRY(hipEventRecord(s.ev[2], c->stream));
	unsigned long long cnt[8] = { 0 };
	HIP_TRY(hipMemcpyAsync(cnt, s.cnt.p, 64, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if ((int)cnt[7]) { fprintf(stderr, "[bwahip] duplicate marking: a record's offset or template index lies outside its run\n"); return BWAHIP_EINTERNAL; }
	if (ms) {
		for (int k = 0; k < 3; ++k) { ms->n_templates[k] = (int64_t)cnt[k]; ms->n_dup_templates[k] = (int64_t)cnt[3 + k]; }
		ms->n_marked = (int64_t)cnt[6];
		const BamSort &bs = c->bs;
		ms->hbm_bytes = run_bytes + (int64_t)(s.hbm.bytes + bs.keys[0].cap + bs.keys[1].cap + bs.idx[0].cap + bs.idx[1].cap);
		float t = 0;
		if (hipEventElapsedTime(&t, s.ev[0], s.ev[2]) == hipSuccess) ms->markdup_ms = t;
		if (hipEventElapsedTime(&t, s.ev[0], s.ev[1]) == hipSuccess) ms->decide_ms = t;
		if (hipEventElapsedTime(&t, s.ev[1], s.ev[2]) == hipSuccess) ms->mark_ms = t;
	}
	return 0;
}

// One finish: the merger, the plan, the locals the steps hand on, and the steps themselves -- run() at the end is their list
struct Finish {
	bwahip_bam_devmerger *const m; FinishPlan plan; const int fd; const double t0 = now_s();
	bwahip_ctx *const c = m->c; Work &w = m->w; SpillWork &sw = m->sw;
	bwahip_devmerge_stats_t s;
	int n = 0, n_runs = 0; int64_t total = 0;                      // records, runs, bytes of the sorted stream
	std::vector<int64_t> first, run_len;                           // per run, for k_src_table: the first ordinal (n_runs + 1 entries), the bytes
	std::vector<const uint8_t*> run_rec; std::vector<const int64_t*> run_off;
	const unsigned *idx = nullptr;                                 // the order: the ordinal at every sorted place
	int64_t piece_bytes = 0; int n_pieces = 0; std::vector<int> piece_first;
	int *mlen_all = nullptr;                                       // the whole stream's member lengths, for the index
	std::vector<RecordStage*> rs;                                  // the armed record stages, in the order they run (after marking)
	// spilled runs: the window plan; by index in run order the run, its number, its first ordinal and template; [window][run] the slices' bases
	SpillPlan sp; int wp = 1; bool parsed = false;                 // parsed: the index parse ran window by window
	std::vector<DevRun*> runv; std::vector<int64_t> run_id, rec_at, tmpl_at, base; std::vector<uint8_t> flags;
	Finish(bwahip_bam_devmerger *m_, const FinishPlan &p, int fd_) : m(m_), plan(p), fd(fd_)
	{
		plan.spill = m->n_spilled > 0;
		for (RecordStage *s : m->stages) if (s->armed) rs.push_back(s);
	}
	int64_t piece_len(int p) const { const int64_t lo = (int64_t)p * piece_bytes; return total - lo < piece_bytes ? total - lo : piece_bytes; }
	// The records pass: positions [lo, hi) of run r, on the context's stream.  rec + r->off[i] is record i: rec is the run's bytes, or the base of a
	// staged slice.  [lo, counted) are counted; a record in [counted, hi) -- the next window stages it again -- is marked too, into a counter
	// nobody reads, and passes no record stage.  ord0 / tmpl0: the run's first record and template among all runs'
	int mark_pass(const DevRun *r, uint8_t *rec, int64_t lo, int64_t counted, int64_t hi, int64_t tmpl0)
	{
		int rc;
		if ((rc = markdup_mark_run(m->md.get(), c, rec, r->off() + lo, counted - lo, r->len, r->tmpl() + lo, tmpl0, r->n_tmpl))) return rc;
		return hi > counted ? markdup_mark_run(m->md.get(), c, rec, r->off() + counted, hi - counted, r->len, r->tmpl() + counted, tmpl0, r->n_tmpl, sw.scratch.as<unsigned long long>()) : 0;
	}
	int stage_pass(RecordStage *s, const DevRun *r, const uint8_t *rec, int64_t lo, int64_t counted, int64_t ord0) { return s->records(c, rec, r->off() + lo, counted - lo, r->len, ord0 + lo); }
	int checks()
	{
		if (plan.mark) for (auto &kv : m->runs) if (!kv.second->has_dup) return BWAHIP_EINVAL;   // before a byte is written
		if (plan.mark && !m->md) m->md.reset(new MarkdupStage);
		if (plan.spill) for (const RecordStage *s : rs) if (!s->takes_windows()) return BWAHIP_EINVAL;   // (the setters keep the two apart)
		if (plan.index && !m->bai) m->bai.reset(bai_stage_new());
		memset(&s, 0, sizeof s);
		s.n_records = m->n_records; s.n_runs = (int64_t)m->runs.size(); s.raw_bytes = m->raw_bytes; s.n_blocks = bgzf_blocks(m->raw_bytes);
		for (auto &kv : m->runs) s.hbm_bytes += kv.second->n_rec ? (kv.second->spilled ? 0 : kv.second->len) + 16 * kv.second->n_rec + 8 : 0;
		n = (int)m->n_records; n_runs = (int)m->runs.size(); total = m->raw_bytes;
		return 0;
	}
	// One stage over all resident runs: it begins, every run passes (ord / tmpl: the run's first record and template among all runs'), and
	// without a spilled run it ends here -- it awaits the stream, its counters or tables come back; with one, after the last window (tail)
	template <class Begin, class Pass, class End> int resident_stage(Begin begin, Pass pass, End end)
	{
		int rc = begin();
		int64_t ord = 0, tmpl = 0;
		for (auto &kv : m->runs) {
			const DevRun *r = kv.second;
			if (!rc && !r->spilled) rc = pass(r, ord, tmpl);
			ord += r->n_rec; tmpl += r->n_tmpl;
		}
		if (!rc && !plan.spill) rc = end();
		return rc;
	}
	// the resident runs' records pass, one stage after the other over all runs: marking, which writes into the records, then the record stages
	// (a spilled run's records pass in the windows that stage them)
	int resident_pass()
	{
		int rc = 0;
		if (plan.mark)
			rc = resident_stage([&] { return mark_decide(m); }, [&](const DevRun *r, int64_t, int64_t tmpl) { return mark_pass(r, r->rec(), 0, r->n_rec, r->n_rec, tmpl); },
			                    [&] { return mark_end(m, plan.ms); });
		for (RecordStage *s : rs)
			if (!rc) rc = resident_stage([&] { return s->begin(c, m->n_records); }, [&](const DevRun *r, int64_t ord, int64_t) { return stage_pass(s, r, r->rec(), 0, r->n_rec, ord); },
			                             [&] { return s->done(c); });
		return rc;
	}
	// the order: the runs' keys in run order through the stable radix sort, with the ordinals 0 .. n - 1
	int order()
	{
		BamSort &bs = c->bs;
		HIP_TRY(hipSetDevice(c->device));
		int rc;
		if ((rc = w.make_events())) return rc;
		if ((rc = bs.keys[0].ensure((size_t)n * 8)) || (rc = bs.keys[1].ensure((size_t)n * 8)) || (rc = bs.idx[0].ensure((size_t)n * 4)) || (rc = bs.idx[1].ensure((size_t)n * 4))) return rc;
		HIP_TRY(hipEventRecord(w.ev_sort[0], c->stream));
		int64_t at = 0;
		for (auto &kv : m->runs) {
			const DevRun *r = kv.second;
			first.push_back(at); run_rec.push_back(r->rec()); run_off.push_back(r->off()); run_len.push_back(r->len);
			if (r->n_rec) HIP_TRY(hipMemcpyAsync(bs.keys[0].as<uint64_t>() + at, r->keys(), (size_t)r->n_rec * 8, hipMemcpyDeviceToDevice, c->stream));
			at += r->n_rec;
		}
		first.push_back(at);
		int cur = 0;
		if ((rc = bam_sort_iota(bs.idx[0].as<unsigned>(), n, c->stream)) || (rc = bam_sort_radix(c, n, 64, &cur))) return rc;
		HIP_TRY(hipEventRecord(w.ev_sort[1], c->stream));
		idx = bs.idx[cur].as<unsigned>();
		return 0;
	}
	// the source table (per ordinal the record's address and length) and the records' offsets in the sorted stream
	int offsets()
	{
		int rc;
		if ((rc = dev_upload(w.first, first.data(), first.size() * 8, c->stream)) || (rc = dev_upload(w.run_rec, run_rec.data(), run_rec.size() * 8, c->stream)) ||
		    (rc = dev_upload(w.run_off, run_off.data(), run_off.size() * 8, c->stream)) || (rc = dev_upload(w.run_len, run_len.data(), run_len.size() * 8, c->stream))) return rc;
		if ((rc = w.addr.ensure((size_t)n * 8)) || (rc = w.len.ensure((size_t)n * 4)) || (rc = w.len_sorted.ensure((size_t)n * 4)) || (rc = w.out_off.ensure(((size_t)n + 1) * 8)) || (rc = w.err.ensure(4))) return rc;
		HIP_TRY(hipMemsetAsync(w.err.p, 0, 4, c->stream));
		const int grid_n = (n + 255) / 256;
		hipLaunchKernelGGL(k_src_table, dim3(grid_n), dim3(256), 0, c->stream, n, n_runs, w.first.as<int64_t>(), w.run_rec.as<const uint8_t*>(), w.run_off.as<const int64_t*>(), w.run_len.as<int64_t>(),
		                   w.addr.as<const uint8_t*>(), w.len.as<int>(), w.err.as<int>());
		if ((rc = launched())) return rc;
		hipLaunchKernelGGL(k_sorted_len, dim3(grid_n), dim3(256), 0, c->stream, idx, w.len.as<int>(), n, w.len_sorted.as<int>());
		if ((rc = launched())) return rc;
		return launch_scan(w.len_sorted.as<int>(), w.out_off.as<int64_t>(), n, c->d_scan, c->stream);
	}
	// the piece cuts: the record that holds every cut, read back with the stream's length and the source table's error word, and verified
	int cuts()
	{
		piece_bytes = (int64_t)m->piece_blocks * BLOCK_IN;
		const int64_t n_pieces64 = (total + piece_bytes - 1) / piece_bytes;
		if (n_pieces64 > 0x7fffffffll / 2) return BWAHIP_ECAPACITY;
		n_pieces = (int)n_pieces64;
		int rc;
		if ((rc = w.piece_first.ensure((size_t)n_pieces * 4))) return rc;
		hipLaunchKernelGGL(k_piece_first, dim3((n_pieces + 255) / 256), dim3(256), 0, c->stream, w.out_off.as<int64_t>(), n, piece_bytes, n_pieces, w.piece_first.as<int>());
		if ((rc = launched())) return rc;
		piece_first.resize((size_t)n_pieces);
		int64_t sum = 0; int err = 0;
		HIP_TRY(hipMemcpyAsync(piece_first.data(), w.piece_first.p, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipMemcpyAsync(&sum, w.out_off.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipMemcpyAsync(&err, w.err.p, 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		if (err || sum != total) { fprintf(stderr, "[bwahip] sorted BAM: the runs' offsets give %lld bytes, the runs hold %lld\n", (long long)sum, (long long)total); return BWAHIP_EINTERNAL; }
		for (int p = 0; p < n_pieces; ++p) if (piece_first[(size_t)p] < 0 || piece_first[(size_t)p] >= n || (p && piece_first[(size_t)p] < piece_first[(size_t)p - 1])) return BWAHIP_EINTERNAL;
		return 0;
	}
	// the piece buffers, once: input, and the bound of the members ("input + 31 per block", as bgzf_deflate grows its output to)
	int buffers()
	{
		const int64_t in_cap = total < piece_bytes ? total : piece_bytes, out_cap = in_cap + bgzf_blocks(in_cap) * 31 + 64;
		int rc;
		for (int k = 0; k < 2; ++k)
			if ((rc = w.in[k].ensure((size_t)in_cap)) || (rc = w.out[k].ensure((size_t)out_cap)) || (rc = w.tot[k].ensure(16)) || (rc = w.h_out[k].ensure((size_t)out_cap))) return rc;
		if ((rc = w.h_tot.ensure(32))) return rc;
		return plan.index ? bai_stage_members(m->bai.get(), s.n_blocks, &mlen_all) : 0;
	}
	// spilled runs: the windows' cuts, the plan of the slices every window stages, the staging buffers and the slices' bases
	int windows()
	{
		const size_t NR = (size_t)n_runs;
		int rc;
		if ((rc = sw.make_events())) return rc;
		std::vector<SpillRun> runs;
		int64_t ord = 0, tmpl = 0;
		for (auto &kv : m->runs) {
			DevRun *r = kv.second;
			runv.push_back(r); run_id.push_back(kv.first); rec_at.push_back(ord); tmpl_at.push_back(tmpl); flags.push_back(r->spilled);
			runs.push_back({ r->spilled, r->n_rec, r->h_off.data() });
			ord += r->n_rec; tmpl += r->n_tmpl;
		}
		wp = m->window_pieces > 0 ? m->window_pieces : 1;
		if ((rc = spill_plan_begin(&sp, runs, n_pieces, wp, piece_first.data(), n))) return rc;
		const size_t cells = (size_t)sp.n_windows * (NR + 1);
		if ((rc = dev_upload(sw.flags, flags.data(), NR, c->stream)) || (rc = sw.cut.ensure(cells * 4)) || (rc = sw.scratch.ensure(8)) ||
		    (rc = spill_window_cuts(c->stream, n, n_runs, w.first.as<int64_t>(), sw.flags.as<uint8_t>(), idx, w.piece_first.as<int>(), wp, sp.n_windows, sw.cut.as<int>()))) return rc;
		std::vector<int> cut(cells);
		HIP_TRY(hipMemcpyAsync(cut.data(), sw.cut.p, cells * 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		if ((rc = spill_plan_cuts(&sp, cut.data()))) return rc;
		bool files = false;
		for (size_t r = 0; r < NR; ++r) if (flags[r] && runv[r]->len && !spill_store_mem(m->store, run_id[r])) files = true;
		for (int k = 0; k < 2; ++k) if ((rc = sw.stage[k].ensure((size_t)(sp.cap ? sp.cap : 1))) || (files && (rc = sw.bounce[k].ensure((size_t)(sp.cap ? sp.cap : 1))))) return rc;
		base.assign((size_t)sp.n_windows * NR, 0);                   // + an offset of the run = the record in the staging buffer
		for (int wd = 0; wd < sp.n_windows; ++wd)
			for (size_t r = 0; r < NR; ++r) {
				if (!flags[r] || !runv[r]->n_rec) continue;
				const int64_t lo = sp.S[(size_t)wd * NR + r];
				base[(size_t)wd * NR + r] = (int64_t)(uintptr_t)sw.stage[wd & 1].p + sp.slice_at[(size_t)wd * NR + r] - runv[r]->h_off[(size_t)lo];
			}
		if ((rc = dev_upload(sw.base, base.data(), base.size() * 8, c->stream))) return rc;
		if (plan.index) { if ((rc = bai_stage_parse_begin(m->bai.get(), c, n, s.n_blocks, plan.n_ref))) return rc; parsed = true; }
		m->n_windows = sp.n_windows; m->upload_ms = 0;
		return 0;
	}
	// window wd's slices to its staging buffer, on the copy stream: memory-backed runs from their (pinned) memory, file-backed ones through the bounce buffer
	int window_upload(int wd)
	{
		const int b = wd & 1;
		float t = 0;
		if (wd >= 2) {
			HIP_TRY(hipStreamWaitEvent(c->stream_copy, sw.ev_used[b], 0));   // window wd - 2 has been read
			HIP_TRY(hipEventSynchronize(sw.ev_up[b]));                       // and has left the bounce buffer
			if (hipEventElapsedTime(&t, sw.ev_up0[b], sw.ev_up[b]) == hipSuccess) m->upload_ms += t;
		}
		HIP_TRY(hipEventRecord(sw.ev_up0[b], c->stream_copy));
		for (size_t r = 0; r < runv.size(); ++r) {
			const int64_t bytes = sp.slice_bytes(wd, r), at = sp.slice_at[(size_t)wd * runv.size() + r];
			if (!bytes) continue;
			const int64_t from = runv[r]->h_off[(size_t)sp.S[(size_t)wd * runv.size() + r]];
			const uint8_t *src = spill_store_mem(m->store, run_id[r]);
			if (src) src += from;
			else {
				uint8_t *bounce = (uint8_t*)sw.bounce[b].p + at;
				const int rc = spill_store_get(m->store, run_id[r], from, bytes, bounce);
				if (rc) return rc;
				src = bounce;
			}
			HIP_TRY(hipMemcpyAsync(sw.stage[b].as<uint8_t>() + at, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream_copy));
		}
		HIP_TRY(hipEventRecord(sw.ev_up[b], c->stream_copy));
		return 0;
	}
	// window wd begins, on the context's stream: its slices pass the record-reading stages, its records' source addresses are rebuilt
	int window_begin(int wd)
	{
		const size_t NR = runv.size();
		HIP_TRY(hipStreamWaitEvent(c->stream, sw.ev_up[wd & 1], 0));
		for (size_t r = 0; r < NR; ++r) {
			int64_t lo, counted, hi;
			sp.slice(wd, r, &lo, &counted, &hi);
			if (!runv[r]->spilled || hi <= lo) continue;
			uint8_t *rec = reinterpret_cast<uint8_t*>((uintptr_t)base[(size_t)wd * NR + r]);
			int rc = plan.mark ? mark_pass(runv[r], rec, lo, counted, hi, tmpl_at[r]) : 0;
			for (RecordStage *s : rs) if (!rc) rc = stage_pass(s, runv[r], rec, lo, counted, rec_at[r]);
			if (rc) return rc;
		}
		const int rec_lo = sp.first[(size_t)wd], rec_hi = wd + 1 < sp.n_windows ? sp.first[(size_t)wd + 1] : n - 1;
		return spill_window_addr(c->stream, rec_lo, rec_hi - rec_lo + 1, n_runs, w.first.as<int64_t>(), w.run_off.as<const int64_t*>(), sw.flags.as<uint8_t>(), sw.base.as<int64_t>() + (size_t)wd * NR, idx,
		                         w.addr.as<const uint8_t*>());
	}
	// window wd's last piece is queued: the index parse of the records it holds whole with their predecessors; the staging buffer is free behind it
	int window_end(int wd)
	{
		int rc;
		if (plan.index && (rc = bai_stage_parse(m->bai.get(), c, sp.first[(size_t)wd] + (wd > 0), wd + 1 < sp.n_windows ? sp.first[(size_t)wd + 1] + 1 : n, w.addr.as<const uint8_t*>(), idx,
		                                        w.out_off.as<int64_t>(), plan.n_ref))) return rc;
		HIP_TRY(hipEventRecord(sw.ev_used[wd & 1], c->stream));
		return 0;
	}
	// piece k: gathered and deflated on the context's stream; the windows begin, end and travel around their pieces
	int piece_queue(int k)
	{
		const int b = k & 1, wd = k / wp;
		int rc;
		if (k >= 2) HIP_TRY(hipStreamWaitEvent(c->stream, w.ev_down[b], 0));   // piece k - 2 has left out[b] (in[b]: the deflate of k - 2 is earlier in this stream)
		const int64_t lo = (int64_t)k * piece_bytes, hi = lo + piece_len(k);
		const int rec_lo = piece_first[(size_t)k];
		const int rec_hi = k + 1 < n_pieces ? piece_first[(size_t)k + 1] : n - 1;   // inclusive: the record that holds the next cut begins in this piece or at the cut
		const int n_rec = rec_hi - rec_lo + 1;
		if (plan.spill && k % wp == 0) {
			if (k == 0 && (rc = window_upload(0))) return rc;
			if ((rc = window_begin(wd))) return rc;
		}
		HIP_TRY(hipEventRecord(w.ev_gather[b], c->stream));
		hipLaunchKernelGGL(k_gather_window, dim3((unsigned)(((int64_t)n_rec * 16 + 255) / 256)), dim3(256), 0, c->stream, w.addr.as<const uint8_t*>(), idx, w.out_off.as<int64_t>(),
		                   rec_lo, n_rec, lo, hi, w.in[b].as<uint8_t>());
		if ((rc = launched())) return rc;
		HIP_TRY(hipEventRecord(w.ev_deflate[b], c->stream));
		if ((rc = bgzf_deflate(c, w.in[b].as<uint8_t>(), hi - lo, w.out[b], w.tot[b].as<int64_t>(), c->stream))) return rc;
		HIP_TRY(hipEventRecord(w.ev_done[b], c->stream));
		if (plan.index)                                             // the piece's member lengths, before the next piece reuses the deflate stage's buffers: same stream
			HIP_TRY(hipMemcpyAsync(mlen_all + (int64_t)k * m->piece_blocks, c->bz.mlen.p, (size_t)bgzf_blocks(hi - lo) * 4, hipMemcpyDeviceToDevice, c->stream));
		if (plan.spill && (k % wp == wp - 1 || k == n_pieces - 1) && (rc = window_end(wd))) return rc;
		if (plan.spill && k % wp == 0 && wd + 1 < sp.n_windows && (rc = window_upload(wd + 1))) return rc;   // the next window travels while this one is gathered and deflated
		return 0;
	}
	// piece k: its total, then its members, come back on the copy stream and are written
	int piece_write(int k)
	{
		const int b = k & 1;
		int64_t *h_tot = (int64_t*)w.h_tot.p;
		HIP_TRY(hipStreamWaitEvent(c->stream_copy, w.ev_done[b], 0));
		HIP_TRY(hipMemcpyAsync(h_tot + 2 * b, w.tot[b].p, 16, hipMemcpyDeviceToHost, c->stream_copy));
		HIP_TRY(hipStreamSynchronize(c->stream_copy));
		const int64_t got = h_tot[2 * b], plen = piece_len(k);
		if (got < 0 || got > plen + bgzf_blocks(plen) * 31) return BWAHIP_EINTERNAL;
		if (got) HIP_TRY(hipMemcpyAsync(w.h_out[b].p, w.out[b].p, (size_t)got, hipMemcpyDeviceToHost, c->stream_copy));
		HIP_TRY(hipEventRecord(w.ev_down[b], c->stream_copy));
		HIP_TRY(hipEventSynchronize(w.ev_down[b]));
		float ms = 0;
		if (hipEventElapsedTime(&ms, w.ev_gather[b], w.ev_deflate[b]) == hipSuccess) s.gather_ms += ms;
		if (hipEventElapsedTime(&ms, w.ev_deflate[b], w.ev_done[b]) == hipSuccess) s.deflate_ms += ms;
		s.bgzf_bytes += got; s.n_stored += h_tot[2 * b + 1];
		int rc;
		if ((rc = write_all(fd, w.h_out[b].p, got, "sorted BAM: writing the members"))) { (void)hipStreamSynchronize(c->stream); return rc; }
		return 0;
	}
	// the piece loop: piece k is queued while piece k - 1 comes back and is written; then what the events and the buffers say
	int pieces()
	{
		int rc = 0;
		for (int k = 0; k <= n_pieces; ++k)
			if ((k < n_pieces && (rc = piece_queue(k))) || (k >= 1 && (rc = piece_write(k - 1)))) return rc;
		HIP_TRY(hipStreamSynchronize(c->stream));
		const BamSort &bs = c->bs;
		float ms = 0;
		if (hipEventElapsedTime(&ms, w.ev_sort[0], w.ev_sort[1]) == hipSuccess) s.sort_ms = ms;
		s.hbm_bytes += (int64_t)(w.hbm.bytes + bs.keys[0].cap + bs.keys[1].cap + bs.idx[0].cap + bs.idx[1].cap + bs.hist.cap + bs.hist_base.cap +
		                           c->bz.slots.cap + c->bz.mlen.cap + c->bz.moff.cap + c->bz.md.cap + c->bz.cnt.cap);
		for (int k = 0, nw = sp.n_windows; plan.spill && k < 2 && k < nw; ++k)   // the last two windows' uploads: no later one has read their events
			if (hipEventElapsedTime(&ms, sw.ev_up0[(nw - 1 - k) & 1], sw.ev_up[(nw - 1 - k) & 1]) == hipSuccess) m->upload_ms += ms;
		return 0;
	}
	// What follows the members, for the empty merger as well: the deferred end of the records pass, the index, the record stages' files, the stats
	int tail(bwahip_devmerge_stats_t *st)
	{
		int rc = plan.spill && plan.mark ? mark_end(m, plan.ms) : 0;   // what the resident finish awaits before the order
		for (RecordStage *s : rs) if (!rc && plan.spill) rc = s->done(c);
		if (!rc && plan.index) {
			std::vector<uint8_t> bytes;
			if (!total && n) rc = BWAHIP_EINVAL;                    // records without a byte cannot be indexed
			else rc = bai_stage_run(m->bai.get(), c, n, w.addr.as<const uint8_t*>(), idx, w.out_off.as<int64_t>(), total, bgzf_blocks(total), plan.base, plan.n_ref, &bytes, plan.bs, parsed);
			if (!rc) rc = write_all(plan.bai_fd, bytes.data(), (int64_t)bytes.size(), "writing the BAI index");
		}
		for (RecordStage *s : rs) if (!rc) rc = s->write();
		s.finish_s = now_s() - t0;
		if (st) *st = s;
		return rc;
	}
	int run(bwahip_devmerge_stats_t *st)
	{
		int rc;
		if ((rc = checks()) || (rc = resident_pass())) return rc;
		if (st) *st = s;
		if (n == 0 || total == 0) return tail(st);                  // nothing to write: no member
		if ((rc = order()) || (rc = offsets()) || (rc = cuts()) || (rc = buffers()) || (plan.spill && (rc = windows())) || (rc = pieces())) return rc;
		return tail(st);
	}
};

} // namespace

int bam_devmerger_finish(bwahip_bam_devmerger *m, int fd, bwahip_devmerge_stats_t *st, FinishPlan plan)
{
	if (!m) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	return Finish(m, plan, fd).run(st);
}

extern "C" int bwahip_bam_devmerger_finish(bwahip_bam_devmerger *m, int fd, bwahip_devmerge_stats_t *st) { return bam_devmerger_finish(m, fd, st, FinishPlan()); }

extern "C" int bwahip_bam_devmerger_finish_bai(bwahip_bam_devmerger *m, int fd, int bai_fd, int64_t first_member_offset, int32_t n_ref, bwahip_devmerge_stats_t *st, bwahip_bai_stats_t *bs)
{
	if (n_ref < 0 || first_member_offset < 0 || first_member_offset >= (1ll << 48)) return BWAHIP_EINVAL;
	if (bs) memset(bs, 0, sizeof *bs);
	return bam_devmerger_finish(m, fd, st, FinishPlan{ true, bai_fd, first_member_offset, n_ref, bs });
}

extern "C" int bwahip_bam_devmerger_finish_markdup(bwahip_bam_devmerger *m, int fd, int bai_fd, int64_t first_member_offset, int32_t n_ref, bwahip_devmerge_stats_t *st,
                                                   bwahip_bai_stats_t *bs, bwahip_markdup_stats_t *ms)
{
	if (first_member_offset < 0 || first_member_offset >= (1ll << 48)) return BWAHIP_EINVAL;
	if (bs) memset(bs, 0, sizeof *bs);
	if (ms) memset(ms, 0, sizeof *ms);
	return bam_devmerger_finish(m, fd, st, FinishPlan{ n_ref >= 0, bai_fd, first_member_offset, n_ref, bs, true, ms });   // n_ref < 0: no index
}

int record_stage_kat(RecordStage *s, bwahip_ctx *c, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, uint8_t *out, int64_t out_cap, int64_t *out_len)
{
	for (int64_t i = 0; i < n_rec; ++i) if (rec_off[i] < 0 || rec_off[i + 1] < rec_off[i]) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf d_rec, d_off;                                           // the caller's records
	int rc = s->begin(c, n_rec);
	if (!rc && n_rec) {
		const size_t len = (size_t)rec_off[n_rec];
		if (!(rc = d_rec.ensure(len + 1)) && !(rc = d_off.ensure(((size_t)n_rec + 1) * 8))) {
			if ((len && hipMemcpyAsync(d_rec.p, rec, len, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
			    hipMemcpyAsync(d_off.p, rec_off, ((size_t)n_rec + 1) * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = BWAHIP_ENODEV;
			if (!rc) rc = s->records(c, d_rec.as<uint8_t>(), d_off.as<int64_t>(), n_rec, (int64_t)len, 0);
		}
	}
	if (!rc) rc = s->done(c);
	(void)hipStreamSynchronize(c->stream);                         // nothing of the stage's buffers, or of these, is in use when they go
	if (rc) return rc;
	*out_len = (int64_t)s->bytes.size();
	if (*out_len > out_cap) return BWAHIP_ECAPACITY;
	memcpy(out, s->bytes.data(), s->bytes.size());
	return 0;
}

extern "C" int bwahip_bam_devmerger_set_qc(bwahip_bam_devmerger *m, const bwahip_qc_opt_t *opt, int32_t n_ref, const int64_t *ref_len, int qc_fd, bwahip_qc_stats_t *qs)
{
	if (!m) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	if (!opt) { m->qc->armed = false; return 0; }
	bwahip_qc_opt_t o;
	int rc;
	if ((rc = qc_resolve(opt, &o)) || (rc = check_refs(n_ref, ref_len, nullptr, NO_SUM_CAP))) return rc;   // the merger is as before
	qc_stage_set(m->qc.get(), o, n_ref, ref_len, qc_fd, qs);
	m->qc->armed = true;
	if (qs) memset(qs, 0, sizeof *qs);
	return 0;
}

int64_t bam_devmerger_record_stages_need(bwahip_bam_devmerger *m, int64_t n_records)
{
	std::lock_guard<std::mutex> lk(m->mu);
	int64_t need = 0;
	for (const RecordStage *s : m->stages) if (s->armed) need += s->hbm_need(n_records);
	return need;
}

// the contig lengths of a stage that reads the reference; pac null: the context's index, so these must be its contigs
static int check_stage_ref(const bwahip_ctx *c, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac)
{
	int64_t sum = 0;
	const int rc = check_refs(n_ref, ref_len, &sum, PU_MAX_SUM);
	if (rc || pac) return rc;
	const bwahip_bns_t &bns = c->host.bns;
	if (n_ref != bns.n_seqs || sum != bns.l_pac || !c->d_pac.p) return BWAHIP_EINVAL;
	for (int32_t r = 0; r < n_ref; ++r) if (ref_len[r] != bns.anns[r].len) return BWAHIP_EINVAL;
	return 0;
}

extern "C" int bwahip_bam_devmerger_set_pileup(bwahip_bam_devmerger *m, const bwahip_pileup_opt_t *opt, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, int pu_fd,
                                               bwahip_pileup_stats_t *ps)
{
	if (!m) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	if (!opt) { m->pu->armed = false; return 0; }
	if (m->spill_armed && !m->pu->takes_windows()) return BWAHIP_EINVAL;   // the evidence pass reads resident runs only
	bwahip_pileup_opt_t o;
	int rc;
	if ((rc = pu_resolve(opt, &o)) || (rc = check_stage_ref(m->c, n_ref, ref_len, pac))) return rc;   // the merger is as before
	pu_stage_set(m->pu.get(), o, n_ref, ref_len, pac, pu_fd, ps);   // (the stage copies pac and uploads the copy once)
	m->pu->armed = true;
	if (ps) memset(ps, 0, sizeof *ps);
	return 0;
}

// As set_pileup, with the mask of known sites (copied; null: none).  The stage takes windows: armed for spilling or not, the merger takes it
extern "C" int bwahip_bam_devmerger_set_recal(bwahip_bam_devmerger *m, const bwahip_recal_opt_t *opt, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const uint8_t *mask,
                                              int rc_fd, bwahip_recal_stats_t *rs)
{
	if (!m) return BWAHIP_EINVAL;
	std::lock_guard<std::mutex> lk(m->mu);
	if (!opt) { m->rc->armed = false; return 0; }
	bwahip_recal_opt_t o;
	int rc;
	if ((rc = rc_resolve(opt, &o)) || (rc = check_stage_ref(m->c, n_ref, ref_len, pac))) return rc;   // the merger is as before
	recal_stage_set(m->rc.get(), o, n_ref, ref_len, pac, mask, rc_fd, rs);   // (the stage copies pac and the mask and uploads the copies once)
	m->rc->armed = true;
	if (rs) memset(rs, 0, sizeof *rs);
	return 0;
}

extern "C" void bwahip_bam_devmerger_close(bwahip_bam_devmerger *m)
{
	if (!m) return;
	(void)hipSetDevice(m->c->device);
	for (const Stream *q : { &m->c->stream_copy, &m->c->stream }) if (*q) (void)hipStreamSynchronize(*q);   // after a failed finish work may still be queued on the buffers
	for (auto &kv : m->runs) bam_devrun_free(kv.second);
	spill_store_free(m->store);
	delete m;                                                      // the stages, the work buffers and their events go with it
}
