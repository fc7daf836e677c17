// The batch driver behind the C ABI: FASTQ files in -> SAM text or a BAM file out, over any number of contexts.  What superBatchMain
// (cuda/superbatch_process.cpp:133: read || process, double buffered, one GPU) and process() / kt_pipeline of fastmap.c
// (read -> mem_process_seqs -> fputs, fastmap.c:46,307) do in the reference, for N GPUs and several batches in flight per GPU:
//
//   one reader      bwahip_fastq_* (its own parse / inflate threads) cuts batches exactly as bseq_read does (-K bases);
//   N contexts      (on N devices, or clones sharing one device's index), each a software pipeline of three threads working on
//                   three different batches (stream_pipe.h):
//                     stager   takes the next batch under the reader's lock -- which also fixes the batch's number and its true
//                              n_processed (the global index of its first read: hash_64 tie-breaks, bwamem.c:534/1204, and the
//                              per-batch mem_pestat then come out as in a serial run) -- gathers it into a pinned buffer and copies
//                              it to HBM (batch k+1);
//                     compute  queues k_nt4_conv, the hot path and the finalisation (batch k);
//                     drainer  takes the batch off the context as the run's sink says (a download, mostly) and hands it to the writer (batch k-1);
//   one writer      hands the batches in batch order to the run's sink (below: SAM text or one of four ways to a BAM file on the caller's
//                   file descriptor), and gives every buffer back to the context it came from once the sink has taken its bytes.
//
// A context has two sets of input buffers and two of output buffers; a set is reused only when its consumer has said it is done with
// it (Pipe::in_free / out_free below).  A stager asks for a batch when it has a free input set, so batches go to whichever context
// frees first and staging runs ahead of a context that still computes; results do not depend on which context took a batch
// (tests/test_gpu_multi.py).  No data-path collective: SURVEY.md 8(e).
#include "../../include/bwahip.h"
#include "qc_tables.h"                                          // the size of a QC summary
#include "stream_pipe.h"                                        // with ctx_internal.h: the contexts' devices, the runs a device merger holds (k_bammerge.hip)
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One finished batch on its way from its drainer to the writer
struct Item {
	const char *p = nullptr; int64_t len = 0;                    // the bytes, in the pinned buffer of output set `out` of context `ctx`
	int ctx = 0, out = 0; bool holds_set = true;                 // holds_set: the set is the writer's until the bytes are taken; false: it went back to its context already (a run kept in HBM)
	const uint64_t *keys = nullptr; const int64_t *rec_off = nullptr; int64_t n_rec = 0;   // coordinate-sorted records
	int64_t raw_len = 0;                                         // what the batch counts for in st->sam_bytes: the bytes of its text or records, deflated or not
	DevRun *run = nullptr;                                       // the batch as a run in HBM: no bytes
	double gpu_ms = 0; int64_t n_blocks = 0, n_stored = 0;       // the sort or the deflate stage on the GPU; BGZF members
};

// Where the batches of a run go.  The driver is the same for every output: a sink says what the contexts compute, how a drainer takes a
// batch off its context, and what the writer does with it.  This one is SAM text, written as it comes.
struct Sink {
	OutForm form = OutForm::Sam;                                 // what the contexts compute
	bool host_deflates = false;                                  // half of the host threads deflate for the writer, the other half stages (else: all stage)
	int fd = -1, n_threads = 1, n_deflate = 0;                   // from the driver, before open: the descriptor, opt->n_threads, the deflating share of it
	virtual ~Sink() {}                                           // clean-up on every path: mergers, their files, buffers
	virtual int open(bwahip_ctx *const *ctxs, int n_ctx) { return 0; }   // argument checks and set-up, before the reader is opened
	// a drainer: batch `out` of context c leaves its context (*t_kernels_end: from here on its input set is free) and becomes an item
	virtual int stage_out(bwahip_ctx *c, int out, Item &it, double *t_kernels_end) { const int r = pipe_stage_out(c, out, &it.p, &it.len, t_kernels_end); it.raw_len = it.len; return r; }
	virtual int write(int64_t seq_no, Item &it)                  // the writer: batch seq_no, in batch order
	{
		for (int64_t o = 0; fd >= 0 && o < it.len;) {
			const ssize_t w = ::write(fd, it.p + o, (size_t)(it.len - o > (1ll << 30) ? (1ll << 30) : it.len - o));
			if (w < 0) { if (errno == EINTR) continue; fprintf(stderr, "[bwahip] writing the SAM text failed: %s\n", strerror(errno)); return BWAHIP_EIO; }
			o += w;
		}
		return 0;
	}
	virtual void drop(Item &it) {}                               // an item nobody will write (after a failure)
	virtual int finish() { return 0; }                           // after the last batch of a run without failure: what the file still lacks
};

// BAM in input order: the header before the first batch, every batch's records through the host's BGZF writer, the end-of-file block.
// With bs: the members of the records are made on the GPU (k_bgzf.hip), so the batches arrive deflated and are only written; no host
// thread deflates, and the header goes through the host writer at level 1.
struct BamSink : Sink {
	const char *hdr_line; int level; bwahip_bgzf_stats_t *bs;
	BamSink(const char *h, int lv, bwahip_bgzf_stats_t *b = nullptr) : hdr_line(h), level(lv), bs(b) { form = bs ? OutForm::Bgzf : OutForm::Bam; host_deflates = !bs; }
	int open(bwahip_ctx *const *ctxs, int) override
	{
		if (level < 0 || level > 9) return BWAHIP_EINVAL;
		uint8_t *hdr = nullptr; int64_t hlen = 0;
		int r = bwahip_bam_header(bwahip_bns(ctxs[0]), hdr_line, &hdr, &hlen);
		if (!r) { r = bwahip_bgzf_write(fd, hdr, hlen, level, 1); free(hdr); }
		return r;
	}
	int stage_out(bwahip_ctx *c, int out, Item &it, double *t_end) override { const int r = Sink::stage_out(c, out, it, t_end); return r || !bs ? r : pipe_stage_out_bgzf(c, out, &it.raw_len, &it.n_blocks, &it.n_stored, &it.gpu_ms); }
	int write(int64_t seq_no, Item &it) override
	{
		if (!bs) return bwahip_bgzf_write(fd, it.p, it.len, level, n_deflate);
		bs->raw_bytes += it.raw_len; bs->bgzf_bytes += it.len; bs->n_blocks += it.n_blocks; bs->n_stored += it.n_stored; bs->deflate_ms += it.gpu_ms;
		return Sink::write(seq_no, it);
	}
	int finish() override { return bwahip_bgzf_eof(fd); }
};

// Coordinate-sorted BAM merged on the host: every batch leaves its context sorted and becomes a run of the merger (the batch number is
// the run number), which copies or spills it; after the last batch: header, the merge of the runs through the BGZF writer, the
// end-of-file block.  The statistics go to the caller's bwahip_sort_t, or to the same fields of a bwahip_sort_dev_t.
struct SortedSink : Sink {
	const char *hdr_line, *tmp_dir; int64_t mem_budget; int level;
	int64_t *n_records, *n_runs, *spilled_bytes; double *sort_ms_out, *merge_s;
	uint8_t *hdr = nullptr; int64_t hlen = 0; bwahip_bam_merger *m = nullptr; double sort_ms = 0;
	bool with_bai = false; int bai_fd = -1; int32_t n_ref = 0;   // the BAI index beside the file (bwahip_stream_run_bam_sorted_bai): a builder listens to the merge
	template <class S> SortedSink(const char *h, int lv, S *so) : hdr_line(h), tmp_dir(so->tmp_dir), mem_budget(so->mem_budget), level(lv),
		n_records(&so->n_records), n_runs(&so->n_runs), spilled_bytes(&so->spilled_bytes), sort_ms_out(&so->sort_ms), merge_s(&so->merge_s) { form = OutForm::BamSorted; host_deflates = true; }
	~SortedSink() { free(hdr); bwahip_bam_merger_close(m); }    // the merger and its files go whatever happens
	int prepare(bwahip_ctx *c0)                                  // everything but the merger: the header waits for the merge
	{
		if (level < 0 || level > 9) return BWAHIP_EINVAL;
		*n_records = *n_runs = *spilled_bytes = 0; *sort_ms_out = *merge_s = 0;
		if (with_bai) { const int r = bwahip_bai_check_contigs(bwahip_bns(c0)); if (r) return r; n_ref = bwahip_bns(c0)->n_seqs; }   // a contig BAI cannot hold: before anything starts
		return bwahip_bam_header_sorted(bwahip_bns(c0), hdr_line, &hdr, &hlen);
	}
	// the header's members; with the index their bytes are counted: the offset of the first member of the records
	int write_header(int lv, int64_t *first_member_offset)
	{
		if (!with_bai) return bwahip_bgzf_write(fd, hdr, hlen, lv, 1);
		std::vector<int32_t> lens((size_t)((hlen + 65279) / 65280));
		int64_t n_mem = 0;
		const int r = bwahip_bgzf_write_lens(fd, hdr, hlen, lv, 1, lens.data(), (int64_t)lens.size(), &n_mem);
		*first_member_offset = 0;
		for (int64_t k = 0; k < n_mem; ++k) *first_member_offset += lens[(size_t)k];
		return r;
	}
	int open(bwahip_ctx *const *ctxs, int) override { const int r = prepare(ctxs[0]); return r ? r : bwahip_bam_merger_open(tmp_dir, mem_budget, &m); }
	int stage_out(bwahip_ctx *c, int out, Item &it, double *t_end) override { const int r = Sink::stage_out(c, out, it, t_end); return r ? r : pipe_stage_out_sorted(c, out, &it.keys, &it.rec_off, &it.n_rec, &it.gpu_ms); }
	int write(int64_t seq_no, Item &it) override { sort_ms += it.gpu_ms; return bwahip_bam_merger_add(m, seq_no, (const uint8_t*)it.p, it.len, it.keys, it.rec_off, it.n_rec); }
	int finish() override
	{
		int64_t base = 0;
		int r = write_header(level, &base);
		bwahip_bai_builder *bb = nullptr;
		if (!r && with_bai) r = bwahip_bai_builder_open(n_ref, base, &bb);
		// the staging threads have ended, so the merge's BGZF writer gets all host threads (the bytes do not depend on the number of threads)
		if (!r) r = bb ? bwahip_bam_merger_finish_bai(m, fd, level, n_threads > 1 ? n_threads : 1, bb) : bwahip_bam_merger_finish(m, fd, level, n_threads > 1 ? n_threads : 1);
		bwahip_bam_merger_stats(m, n_records, n_runs, spilled_bytes, merge_s);
		*sort_ms_out = sort_ms;
		if (!r) r = bwahip_bgzf_eof(fd);
		if (!r && bb) r = bwahip_bai_builder_finish(bb, bai_fd);    // the index last: nothing of it is written unless the file is whole
		bwahip_bai_builder_close(bb);
		return r;
	}
};

// What a device-merged entry point asks of its sink: the products beside the file (an options pointer arms the product, its stats struct may
// be null) and the two things that are no product.
//   fall_back  a run that does not fit sd->hbm_budget ends the call on the host, as bwahip_stream_run_bam_sorted does, at sd->level.  Only
//              what the host can also make may ask for it: _dev, _dev_bai, and _dev_qc unmarked.  Without it the header is written at level 1,
//              sd->level has no reader, and such a run ends the call (BWAHIP_ECAPACITY) or, with sp, is held spilled: _dev_markdup,
//              _dev_qc marked, _dev_pileup (even unmarked), _dev_spill, _dev_recal.
//   index      with_index(bai_fd), for every entry point that takes a bai_fd: a run that may fall back indexes whatever bai_fd is (the
//              host-merged run would); one that may not, if and only if bai_fd >= 0.  _dev takes none and does not index.
struct SortedDevReq {
	bwahip_sort_dev_t *sd = nullptr;
	bool fall_back = false, index = false; int bai_fd = -1;
	bool mark = false; bwahip_markdup_stats_t *ms = nullptr;       // the runs carry templates (OutForm::BamSortedDup), the finish marks
	const bwahip_qc_opt_t *qc = nullptr; int qc_fd = -1; bwahip_qc_stats_t *qs = nullptr;
	const bwahip_pileup_opt_t *pu = nullptr; int pu_fd = -1; bwahip_pileup_stats_t *ps = nullptr;
	const bwahip_recal_opt_t *rc = nullptr; const uint8_t *mask = nullptr; int rc_fd = -1; bwahip_recal_stats_t *rs = nullptr;
	bwahip_spill_t *sp = nullptr;                                  // SpillSortedSink (null: DevSortedSink)
	void with_index(int fd) { bai_fd = fd; index = fall_back || fd >= 0; }
};

// Coordinate-sorted BAM merged on the device: every batch is a run of the device merger, copied device to device into buffers of its own,
// while the HBM budget holds; from the first run that does not fit (or came back downloaded because its buffers could not be allocated)
// the run ends as the host-merged one: the runs held so far go to its merger in run order, every later one is downloaded.  No host thread
// deflates.  Without a fall-back the header is written at level 1 and the device merger writes the rest (k_bammerge.hip).
struct DevSortedSink : Sink {
	const SortedDevReq rq; bwahip_sort_dev_t *sd; SortedSink host;
	bwahip_bam_devmerger *dm = nullptr; bwahip_ctx *ctx0 = nullptr;
	int64_t hbm_budget = 0, held_raw = 0, held_rec = 0, held_tmpl = 0; int piece_blocks = 0;
	int64_t bai_windows = 0;                                     // with the index: the 16 Kbp windows of the contig table, for the stage's share of the budget
	std::vector<int64_t> ref_len; bwahip_qc_builder *qb = nullptr;   // the contigs' lengths; the fall-back's QC builder
	std::atomic<bool> fell_back{false};                          // read by the drainers: from now on they download
	Stream fb_stream; HostBuf fb_rec, fb_keys, fb_off;   // the fall-back's downloads: their stream, one pinned buffer each for records, keys and offsets
	DevSortedSink(const char *h, const SortedDevReq &r) : rq(r), sd(r.sd), host(h, r.fall_back ? r.sd->level : 1, r.sd)
	{ form = rq.mark ? OutForm::BamSortedDup : OutForm::BamSorted; host.with_bai = rq.index; host.bai_fd = rq.bai_fd; }
	~DevSortedSink()
	{
		if (ctx0) (void)hipSetDevice(ctx0->device);
		bwahip_bam_devmerger_close(dm);
		bwahip_qc_builder_close(qb);
	}
	int open(bwahip_ctx *const *ctxs, int n_ctx) override
	{
		for (int i = 1; i < n_ctx; ++i) if (ctxs[i]->device != ctxs[0]->device) return BWAHIP_EINVAL;   // the runs of all contexts meet in one device's merger
		if (sd->piece_blocks > 4096 || sd->hbm_budget < 0) return BWAHIP_EINVAL;
		host.fd = fd; host.n_threads = n_threads;
		int r = host.prepare(ctxs[0]);                              // the host merger itself is opened only at a fall-back: tmp_dir is not looked at before
		if (r) return r;
		sd->fell_back = 0; sd->fell_back_at_run = 0; memset(&sd->dev, 0, sizeof sd->dev);
		const bwahip_bns_t *bns = bwahip_bns(ctxs[0]);
		for (int32_t i = 0; i < bns->n_seqs; ++i) ref_len.push_back(bns->anns[i].len);
		if (host.with_bai) for (int64_t L : ref_len) bai_windows += (L + 16383) >> 14;
		if ((r = bwahip_bam_devmerger_open(ctxs[0], sd->piece_blocks, &dm))) return r;
		// the merger is armed for what was asked: bad options are refused here, before anything starts.  Pileup and table read the contexts' reference
		const int32_t n_ref = (int32_t)ref_len.size();
		if (rq.qc && (r = bwahip_bam_devmerger_set_qc(dm, rq.qc, n_ref, ref_len.data(), rq.qc_fd, rq.qs))) return r;
		if (rq.pu && (r = bwahip_bam_devmerger_set_pileup(dm, rq.pu, n_ref, ref_len.data(), nullptr, rq.pu_fd, rq.ps))) return r;
		if (rq.rc && (r = bwahip_bam_devmerger_set_recal(dm, rq.rc, n_ref, ref_len.data(), nullptr, rq.mask, rq.rc_fd, rq.rs))) return r;
		ctx0 = ctxs[0]; hbm_budget = sd->hbm_budget;
		piece_blocks = sd->piece_blocks > 0 ? sd->piece_blocks : ctx0->knobs.sorted_piece_blocks;
		if (!hbm_budget) {                                          // half of what the device has free now
			size_t mem_free = 0, mem_total = 0;
			HIP_TRY(hipSetDevice(ctx0->device));
			HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
			hbm_budget = (int64_t)(mem_free / 2);
		}
		return 0;
	}
	int stage_out(bwahip_ctx *c, int out, Item &it, double *t_end) override
	{
		if (!fell_back) {                                           // the run stays in HBM: no download, the writer gets an item without bytes and both sets go back at once
			const int r = pipe_stage_out_devrun(c, out, &it.run, &it.raw_len, &it.n_rec, &it.gpu_ms, t_end);
			if (r || it.run) { it.len = it.raw_len; it.holds_set = false; return r; }
			if (!rq.fall_back) return BWAHIP_ECAPACITY;              // the run's buffers could not be allocated, and this run does not end on the host
		}                                                           // (its buffers could not be allocated: downloaded as any run after a fall-back, which it causes)
		return host.stage_out(c, out, it, t_end);
	}
	// the HBM the enabled stages take beside the merger's own, for this many records, raw bytes and templates: what the armed record stages
	// say they will take, and the shares of the index and of the marking, which are the finish plan's and no record stages
	int64_t stages_need(int64_t n_rec, int64_t raw, int64_t n_tmpl) const
	{
		int64_t need = bam_devmerger_record_stages_need(dm, n_rec);
		if (host.with_bai) need += bwahip_bam_devmerge_bai_hbm_need(n_rec, bgzf_blocks(raw), host.n_ref, bai_windows);
		if (rq.mark) need += bwahip_bam_devmerge_markdup_hbm_need(n_rec, n_tmpl);
		return need;
	}
	// a run in HBM -> the host merger, through the pinned buffers; the run is freed whatever happens
	int run_to_host(int64_t run_no, DevRun *r, double sort_ms)
	{
		int rc = hipSetDevice(ctx0->device) == hipSuccess ? 0 : BWAHIP_ENODEV;
		if (!rc && !fb_stream) rc = fb_stream.make();
		if (!rc && ((rc = fb_rec.ensure((size_t)r->len + 1)) || (rc = fb_keys.ensure((size_t)(r->n_rec + 1) * 8)) || (rc = fb_off.ensure((size_t)(r->n_rec + 1) * 8)))) {}
		if (!rc) rc = bam_devrun_download(r, (uint8_t*)fb_rec.p, (uint64_t*)fb_keys.p, (int64_t*)fb_off.p, fb_stream);
		Item h; h.p = (const char*)fb_rec.p; h.len = r->len; h.keys = (const uint64_t*)fb_keys.p; h.rec_off = (const int64_t*)fb_off.p; h.n_rec = r->n_rec; h.gpu_ms = sort_ms;
		if (!rc) rc = host.write(run_no, h);
		bam_devrun_free(r);
		return rc;
	}
	// run `at` does not fit: the host merger is opened and takes the runs held so far, in run order
	int fall_back(int64_t at)
	{
		int rc = bwahip_bam_merger_open(host.tmp_dir, host.mem_budget, &host.m);
		if (!rc && rq.qc && !(rc = bwahip_qc_builder_open((int32_t)ref_len.size(), ref_len.data(), rq.qc, &qb))) rc = bwahip_bam_merger_set_qc(host.m, qb);   // the host builder listens to the host merge
		std::vector<std::pair<int64_t, DevRun*>> held;
		bam_devmerger_take_runs(dm, &held);
		for (auto &h : held) { if (!rc) rc = run_to_host(h.first, h.second, 0); else bam_devrun_free(h.second); }
		fell_back = true; sd->fell_back = 1; sd->fell_back_at_run = at;
		return rc;
	}
	int write(int64_t seq_no, Item &it) override
	{
		int r = 0;
		if (!fell_back) {                                           // in input order, so the decision depends on the input and the budget alone
			const int64_t need = bwahip_bam_devmerge_hbm_need(held_raw + it.raw_len, held_rec + it.n_rec, seq_no + 1, piece_blocks) +
			                     stages_need(held_rec + it.n_rec, held_raw + it.raw_len, held_tmpl + (it.run ? it.run->n_tmpl : 0));
			const bool fits = it.run && need <= hbm_budget;
			if (!fits) r = rq.fall_back ? fall_back(seq_no) : BWAHIP_ECAPACITY;
		}
		if (!r && !fell_back) { if (!(r = bam_devmerger_adopt(dm, seq_no, it.run))) { held_tmpl += it.run->n_tmpl; it.run = nullptr; held_raw += it.raw_len; held_rec += it.n_rec; host.sort_ms += it.gpu_ms; } }
		else if (!r && it.run) { r = run_to_host(seq_no, it.run, it.gpu_ms); it.run = nullptr; }
		else if (!r) r = host.write(seq_no, it);
		drop(it);                                                   // refused, or the fall-back failed before its turn
		return r;
	}
	void drop(Item &it) override { if (it.run) bam_devrun_free(it.run); it.run = nullptr; }
	int finish() override
	{
		if (fell_back) {                                            // from here on this is the host-merged run at sd->level
			int r = host.finish();
			if (!r && qb) r = bwahip_qc_builder_finish(qb, rq.qc_fd);   // the summary last, as the index: nothing of it unless the file is whole
			if (!r && qb && rq.qs) {
				bwahip_qc_opt_t o;
				(void)qc_resolve(rq.qc, &o);                             // (the builder took them)
				memset(rq.qs, 0, sizeof *rq.qs);
				for (int64_t L : ref_len) rq.qs->n_windows += qc_windows(L, o.window_shift);
				rq.qs->qc_bytes = qc_file_bytes((int64_t)ref_len.size(), rq.qs->n_windows);
			}
			return r;
		}
		return finish_on_device();
	}
	// the header at level 1, the device merger's finish with the stages the request names, the end-of-file block.  The plan goes
	// straight to the internal finish: what the C entry points check or clear holds here already (n_ref is the contig table's, base the
	// header's bytes, ms was cleared by the entry point, no index stats are asked for)
	int finish_on_device()
	{
		FinishPlan plan;
		plan.index = host.with_bai; plan.bai_fd = host.bai_fd; plan.n_ref = host.n_ref; plan.mark = rq.mark; plan.ms = rq.mark ? rq.ms : nullptr;
		int r = host.write_header(1, &plan.base);
		if (!r) r = bam_devmerger_finish(dm, fd, &sd->dev, plan);
		if (!r) { sd->n_records = sd->dev.n_records; sd->n_runs = sd->dev.n_runs; sd->merge_s = sd->dev.finish_s; }
		sd->sort_ms = host.sort_ms;
		return r ? r : bwahip_bgzf_eof(fd);
	}
};

// DevSortedSink for samples whose record bytes outgrow HBM (k_bamspill.hip): no fall-back.  Runs are decided in input order: a run stays
// resident while bwahip_bam_devmerge_spill_hbm_need of the resident bytes so far -- with one full window of staging reserved as spilled
// bytes, longest_record 0 -- plus the enabled stages' needs is within the budget; from the first run that is not, every run is held
// spilled: its record bytes travel device -> host store on the sink's copy stream, its small arrays stay where the drainer put them.
// A spilled run after which the need of what is held (now with the real spilled bytes and longest record) exceeds the budget ends the call
// with BWAHIP_ECAPACITY; nothing of the records has been written then (the merger writes at the finish).
struct SpillSortedSink : DevSortedSink {
	bwahip_spill_t *sp; bool spilling = false;
	int64_t spilled_raw = 0, longest = 0, all_rec = 0, all_tmpl = 0; int wp = 0;
	SpillSortedSink(const char *h, const SortedDevReq &r) : DevSortedSink(h, r), sp(r.sp) {}
	int open(bwahip_ctx *const *ctxs, int n_ctx) override
	{
		if (sp->host_budget < 0 || sp->window_pieces > 65536) return BWAHIP_EINVAL;
		int r = DevSortedSink::open(ctxs, n_ctx);
		if (!r) r = bwahip_bam_devmerger_set_spill(dm, sp);
		if (!r) r = hipSetDevice(ctx0->device) == hipSuccess ? fb_stream.make() : BWAHIP_ENODEV;
		if (!r) wp = bam_devmerger_window_pieces(dm);               // the merger resolves the default
		return r;
	}
	int stage_out(bwahip_ctx *c, int out, Item &it, double *t_end) override
	{
		const int r = pipe_stage_out_devrun(c, out, &it.run, &it.raw_len, &it.n_rec, &it.gpu_ms, t_end);
		it.len = it.raw_len; it.holds_set = false;
		return r ? r : it.run ? 0 : BWAHIP_ECAPACITY;               // not even one batch's run fits beside what is held
	}
	int write(int64_t seq_no, Item &it) override
	{
		int r = it.run ? 0 : BWAHIP_ECAPACITY;
		if (!r) {
			const int64_t n_rec = all_rec + it.n_rec, n_tmpl = all_tmpl + it.run->n_tmpl, raw = held_raw + spilled_raw + it.raw_len;
			if (!spilling) {
				const int64_t need = bwahip_bam_devmerge_spill_hbm_need(held_raw + it.raw_len, (int64_t)wp * piece_blocks * 65280, 0, n_rec, seq_no + 1, piece_blocks, wp) + stages_need(n_rec, raw, n_tmpl);
				if (need > hbm_budget) spilling = true;
			}
			if (!spilling) { if (!(r = bam_devmerger_adopt(dm, seq_no, it.run))) held_raw += it.raw_len; }
			else {
				int64_t run_longest = 0;
				if (!(r = bam_devmerger_adopt_spilled(dm, seq_no, it.run, fb_stream, &run_longest))) {
					spilled_raw += it.raw_len;
					if (run_longest > longest) longest = run_longest;
					if (bwahip_bam_devmerge_spill_hbm_need(held_raw, spilled_raw, longest, n_rec, seq_no + 1, piece_blocks, wp) + stages_need(n_rec, raw, n_tmpl) > hbm_budget) {
						fprintf(stderr, "[bwahip] sorted BAM: what stays in HBM of %lld records exceeds the budget of %lld bytes\n", (long long)n_rec, (long long)hbm_budget);
						it.run = nullptr;                                   // the merger owns it
						return BWAHIP_ECAPACITY;
					}
				}
			}
			if (!r) { all_rec = n_rec; all_tmpl = n_tmpl; it.run = nullptr; host.sort_ms += it.gpu_ms; }
		}
		drop(it);
		return r;
	}
	int finish() override { const int r = finish_on_device(); (void)bwahip_bam_devmerger_spill_stats(dm, sp); return r; }
};

struct Driver {
	// reader side
	std::mutex mu_read;
	bwahip_fastq *rd = nullptr;
	int64_t n_processed = 0, next_seq = 0, max_reads = 0;
	bool eof = false;
	// writer side
	std::mutex mu;
	std::condition_variable cv_item;
	std::map<int64_t, Item> ready;                               // finished batches waiting for their turn
	int64_t written = 0;                                         // batches [0, written) are with the sink
	int workers_left = 0;
	int rc = 0;                                                  // first error (the stages and the writer stop on it)
	std::atomic<bool> stop{false};                               // rc != 0, readable without the lock
	std::function<void()> wake_all;                              // wakes every context's threads (failure)
	int64_t sam_bytes = 0;
	double t_last_write = 0, write_s = 0;

	void fail(int code) { { std::lock_guard<std::mutex> lk(mu); if (!rc) rc = code; stop = true; } cv_item.notify_all(); if (wake_all) wake_all(); }
	bool failed() { return stop.load(); }
};

// Closing the reader (joining its threads, unmapping gigabytes of input: tens of milliseconds of page-table work) is nobody's critical path:
// it runs on a thread of its own, joined by the next run or when the library is unloaded.  (Putting it off by 200 ms, so that a run that
// follows at once does not open its files beside it -- 20-60 ms instead of 0.5 -- only moved the cost into that run: measured, no gain.)
struct Reaper {
	std::mutex mu; std::thread t;
	void close_later(bwahip_fastq *rd) { std::lock_guard<std::mutex> lk(mu); if (t.joinable()) t.join(); t = std::thread([rd] { bwahip_fastq_close(rd); }); }
	~Reaper() { if (t.joinable()) t.join(); }
};
Reaper g_reaper;

} // namespace

// One run of the driver into `sink` (above: SAM text, BAM through the host's BGZF writer, BAM deflated on the GPU, coordinate-sorted BAM
// merged on the host or on the device)
static int stream_run(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                      const char *fq1, const char *fq2, int out_fd, bwahip_stream_t *st, Sink &sink)
{
	if (!ctxs || n_ctx < 1 || n_ctx > 256 || !opt || !fq1 || !st) return BWAHIP_EINVAL;
	for (int i = 0; i < n_ctx; ++i) if (!ctxs[i]) return BWAHIP_EINVAL;
	// actual_chunk_size (fastmap.c:304): -K when given, else chunk_size * n_threads
	const int64_t chunk = st->chunk_bases > 0 ? st->chunk_bases : (int64_t)opt->chunk_size * (opt->n_threads > 0 ? opt->n_threads : 1);
	bwahip_opt_t o = *opt;
	if (fq2) o.flag |= BWAHIP_F_PE;
	// opt->n_threads is the host-thread budget of the whole run: where the sink deflates on the host, half of it does, and the rest stages the batches
	const int n_deflate = sink.host_deflates ? (opt->n_threads / 2 > 1 ? opt->n_threads / 2 : 1) : 0;
	const int n_stage = opt->n_threads > n_deflate ? opt->n_threads - n_deflate : opt->n_threads;
	o.n_threads = n_stage / n_ctx > 1 ? n_stage / n_ctx : 1;
	Driver d;
	d.max_reads = st->max_reads;
	sink.fd = out_fd; sink.n_threads = opt->n_threads; sink.n_deflate = n_deflate;
	int rc = sink.open(ctxs, n_ctx);
	if (rc) return rc;
	const double t_call = now_s();
	rc = bwahip_fastq_open_mt(fq1, fq2, st->reader_threads, &d.rd);
	if (rc) return rc;
	st->n_reads = st->n_batches = st->sam_bytes = 0; st->seconds = st->reader_wait_s = st->write_s = st->gpu_busy_s = 0;
	const double t_start = now_s();
	d.workers_left = n_ctx;
	d.t_last_write = t_start;
	const int keep_comments = st->keep_comments;
	const bool log = getenv("BWAHIP_STREAM_LOG") != nullptr;
	const long reallocs0 = pipe_realloc_count();
	// One batch on its way through a context, and the context's hand-over state.  The sets are numbered; who holds which is written down
	// here and nowhere inferred.
	struct Job { int n = 0; int64_t seq_no = 0, np0 = 0; int in = -1, out = -1; double t_final = 0; };
	struct Pipe {
		std::mutex mu; std::condition_variable cv;
		bool in_free[PIPE_SETS], out_free[PIPE_SETS];
		std::deque<Job> staged, computed;                          // stager -> compute -> drainer
		bool staged_end = false, computed_end = false;
		double wait_s = 0, busy_s = 0;
		Pipe() { for (int i = 0; i < PIPE_SETS; ++i) in_free[i] = out_free[i] = true; }
	};
	std::vector<Pipe> pipes(n_ctx);
	// the timeline (BWAHIP_STREAM_LOG): begin and end of every stage of every batch, printed when the pass is over (scripts/stream_timeline.py)
	struct Span { const char *stage; int64_t batch; int ctx; double t0, t1; };
	std::mutex mu_log; std::vector<Span> spans;
	auto span = [&](const char *stage, int64_t batch, int ctx, double t0, double t1) { if (log) { std::lock_guard<std::mutex> lk(mu_log); spans.push_back({ stage, batch, ctx, t0, t1 }); } };
	d.wake_all = [&] { for (auto &p : pipes) { { std::lock_guard<std::mutex> lk(p.mu); } p.cv.notify_all(); } };
	int n_open = 0;
	for (; n_open < n_ctx; ++n_open) if ((rc = pipe_open(ctxs[n_open], o.n_threads))) break;
	if (rc) { for (int w = 0; w <= n_open && w < n_ctx; ++w) pipe_close(ctxs[w]); bwahip_fastq_close(d.rd); return rc; }
	auto take_free = [](bool *f) { for (int i = 0; i < PIPE_SETS; ++i) if (f[i]) { f[i] = false; return i; } return -1; };
	auto any_free = [](const bool *f) { for (int i = 0; i < PIPE_SETS; ++i) if (f[i]) return true; return false; };

	auto stager = [&](int w) {
		Pipe &p = pipes[w];
		for (;;) {
			Job j;
			{
				std::unique_lock<std::mutex> lk(p.mu);
				p.cv.wait(lk, [&] { return d.failed() || any_free(p.in_free); });
				if (d.failed()) break;
				j.in = take_free(p.in_free);
			}
			bwahip_fastq_batch *b = nullptr; bwahip_seq_t *seqs = nullptr;
			bool eof = false;
			const double t0 = now_s();
			{
				std::lock_guard<std::mutex> lk(d.mu_read);
				if (d.failed() || d.eof || (d.max_reads > 0 && d.n_processed >= d.max_reads)) { d.eof = true; eof = true; }
				else {
					const int r = bwahip_fastq_next_batch(d.rd, chunk, keep_comments, &b, &seqs, &j.n);
					if (r) { d.eof = true; eof = true; d.fail(r); }
					else if (j.n == 0) { d.eof = true; eof = true; }
					else { j.seq_no = d.next_seq++; j.np0 = d.n_processed; d.n_processed += j.n; }
				}
			}
			const double t1 = now_s();
			p.wait_s += t1 - t0;
			if (eof) break;
			span("take", j.seq_no, w, t0, t1);
			double t_copy = t1;
			const int r = pipe_stage_in(ctxs[w], j.in, &o, j.n, seqs, sink.form, &t_copy);
			bwahip_fastq_batch_release(b);                          // names, bases and qualities are in HBM
			const double t2 = now_s();
			if (r) { d.fail(r); break; }
			span("stage", j.seq_no, w, t1, t_copy); span("h2d", j.seq_no, w, t_copy, t2);
			{ std::lock_guard<std::mutex> lk(p.mu); p.staged.push_back(j); }
			p.cv.notify_all();
		}
		{ std::lock_guard<std::mutex> lk(p.mu); p.staged_end = true; }
		p.cv.notify_all();
	};
	auto compute = [&](int w) {
		Pipe &p = pipes[w];
		for (;;) {
			Job j;
			{
				std::unique_lock<std::mutex> lk(p.mu);
				p.cv.wait(lk, [&] { return d.failed() || (!p.staged.empty() && any_free(p.out_free)) || (p.staged.empty() && p.staged_end); });
				if (d.failed() || p.staged.empty()) break;
				j = p.staged.front(); p.staged.pop_front();
				j.out = take_free(p.out_free);
			}
			const double t0 = now_s();
			double t_hot = t0;
			const int r = pipe_compute(ctxs[w], j.in, j.out, &o, j.np0, pes0, sink.form, &t_hot);
			if (r) { d.fail(r); break; }
			span("hot", j.seq_no, w, t0, t_hot);
			j.t_final = t_hot;
			p.busy_s += now_s() - t0;
			{ std::lock_guard<std::mutex> lk(p.mu); p.computed.push_back(j); }
			p.cv.notify_all();
		}
		{ std::lock_guard<std::mutex> lk(p.mu); p.computed_end = true; }
		p.cv.notify_all();
	};
	auto drainer = [&](int w) {
		Pipe &p = pipes[w];
		for (;;) {
			Job j;
			{
				std::unique_lock<std::mutex> lk(p.mu);
				p.cv.wait(lk, [&] { return d.failed() || !p.computed.empty() || p.computed_end; });
				if (d.failed() || p.computed.empty()) break;
				j = p.computed.front(); p.computed.pop_front();
			}
			Item it; it.ctx = w; it.out = j.out;
			double t_end = 0;
			const int r = sink.stage_out(ctxs[w], j.out, it, &t_end);
			const double t1 = now_s();
			if (r) { d.fail(r); break; }
			{ std::lock_guard<std::mutex> lk(p.mu); p.in_free[j.in] = true; if (!it.holds_set) p.out_free[j.out] = true; }   // the kernels that read the input set have ended; an output set the item does not hold was copied from
			p.cv.notify_all();
			span("final", j.seq_no, w, j.t_final, t_end); span(it.holds_set ? "d2h" : "d2d", j.seq_no, w, t_end, t1);
			{ std::lock_guard<std::mutex> lk(d.mu); if (d.rc) sink.drop(it); else d.ready[j.seq_no] = it; }   // (dropped: the writer has gone, nobody would take it)
			d.cv_item.notify_all();
		}
		// the buffers must outlive their write
		{ std::unique_lock<std::mutex> lk(p.mu); p.cv.wait(lk, [&] { if (d.failed()) return true; for (int i = 0; i < PIPE_SETS; ++i) if (!p.out_free[i]) return false; return true; }); }
		{ std::lock_guard<std::mutex> lk(d.mu); --d.workers_left; }
		d.cv_item.notify_all();
	};
	auto writer = [&] {
		for (;;) {
			Item it;
			{
				std::unique_lock<std::mutex> lk(d.mu);
				d.cv_item.wait(lk, [&] { return d.rc || d.ready.count(d.written) || (d.workers_left == 0 && d.ready.empty()); });
				if (d.rc || !d.ready.count(d.written)) return;
				it = d.ready[d.written];
				d.ready.erase(d.written);
			}
			const double t0 = now_s();
			const int r = sink.write(d.written, it);
			if (r) { d.fail(r); return; }
			int64_t seq_no;
			{ std::lock_guard<std::mutex> lk(d.mu); seq_no = d.written++; d.sam_bytes += it.raw_len; d.t_last_write = now_s(); d.write_s += d.t_last_write - t0; }
			if (it.holds_set) {                                        // the bytes are taken: the output set goes back to its context
				Pipe &p = pipes[it.ctx];
				{ std::lock_guard<std::mutex> lk(p.mu); p.out_free[it.out] = true; }
				p.cv.notify_all();
			}
			span("write", seq_no, it.ctx, t0, d.t_last_write);
		}
	};
	std::thread wr(writer);
	std::vector<std::thread> th;
	for (int w = 0; w < n_ctx; ++w) { th.emplace_back(stager, w); th.emplace_back(compute, w); th.emplace_back(drainer, w); }
	for (auto &t : th) t.join();
	wr.join();
	for (int w = 0; w < n_ctx; ++w) pipe_close(ctxs[w]);           // after a failure kernels and copies may still be queued: nothing is left running
	for (auto &kv : d.ready) sink.drop(kv.second);                 // after a failure: items nobody took
	if (!d.rc) {                                                  // what the file still lacks: header and merge of a sorted one, the end-of-file block
		const double t0 = now_s();
		d.rc = sink.finish();
		d.write_s += now_s() - t0;
		if (is_bam(sink.form) && !d.rc) d.t_last_write = now_s();
	}
	const double t_joined = now_s();
	g_reaper.close_later(d.rd);
	if (log) {
		for (const Span &x : spans) fprintf(stderr, "[bwahip] span %s batch %lld ctx %d %.3f %.3f\n", x.stage, (long long)x.batch, x.ctx, (x.t0 - t_call) * 1e3, (x.t1 - t_call) * 1e3);
		fprintf(stderr, "[bwahip] stream: %lld batches on %d contexts, %ld buffer reallocations in this pass\n", (long long)d.next_seq, n_ctx, pipe_realloc_count() - reallocs0);
		fprintf(stderr, "[bwahip] stream: open %.1f ms, first batch in -> last SAM byte out %.1f ms, joining the threads %.1f ms, handing the reader to the closer %.1f ms\n",
		        (t_start - t_call) * 1e3, (d.t_last_write - t_start) * 1e3, (t_joined - d.t_last_write) * 1e3, (now_s() - t_joined) * 1e3);
	}
	st->n_reads = d.n_processed; st->n_batches = d.next_seq; st->sam_bytes = d.sam_bytes;
	st->seconds = d.t_last_write - t_call; st->write_s = d.write_s;
	for (const Pipe &p : pipes) { st->reader_wait_s += p.wait_s; st->gpu_busy_s += p.busy_s; }
	return d.rc;
}

extern "C" int bwahip_stream_run(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                 const char *fq1, const char *fq2, int out_fd, bwahip_stream_t *st)
{
	Sink sink;
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, sink);
}

// FASTQ files in -> a BAM file out: bwahip_stream_run with bwahip_process_seqs_bam in the workers and the BGZF writer behind them
extern "C" int bwahip_stream_run_bam(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                     const char *fq1, const char *fq2, int out_fd, const char *hdr_line, int level, bwahip_stream_t *st)
{
	BamSink sink(hdr_line, level);
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, sink);
}

// FASTQ files in -> a coordinate-sorted BAM file out: every batch is sorted on its context (bwahip_process_seqs_bam_sorted's kernels) and
// merged on the host (bwahip_bam_merger_*); the bytes depend on the input and the options alone
extern "C" int bwahip_stream_run_bam_sorted(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                            const char *fq1, const char *fq2, int out_fd, const char *hdr_line, int level, bwahip_stream_t *st, bwahip_sort_t *so)
{
	if (!so) return BWAHIP_EINVAL;
	SortedSink sink(hdr_line, level, so);
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, sink);
}

// FASTQ files in -> a BAM file out with the BGZF blocks of the records made on the GPU (k_bgzf.hip): the header through the host writer,
// every batch's members written as they come back, the end-of-file block; no deflate workers, all host threads stage
extern "C" int bwahip_stream_run_bam_dev(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                         const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_bgzf_stats_t *bs)
{
	if (!bs) return BWAHIP_EINVAL;
	memset(bs, 0, sizeof *bs);
	BamSink sink(hdr_line, 1, bs);
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, sink);
}

// One device-merged run as the request says (SortedDevReq): the stats structs it names are cleared, the sink is the spilling one when it names a store
static int stream_run_sorted_dev(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0, const char *fq1, const char *fq2, int out_fd,
                                 const char *hdr_line, bwahip_stream_t *st, const SortedDevReq &r)
{
	if (!r.sd) return BWAHIP_EINVAL;
	if (r.ms) memset(r.ms, 0, sizeof *r.ms);
	if (r.qs) memset(r.qs, 0, sizeof *r.qs);
	if (r.ps) memset(r.ps, 0, sizeof *r.ps);
	if (r.rs) memset(r.rs, 0, sizeof *r.rs);
	if (r.sp) { SpillSortedSink sink(hdr_line, r); return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, sink); }
	DevSortedSink sink(hdr_line, r);
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, sink);
}

// FASTQ files in -> a coordinate-sorted BAM file out with the runs kept in HBM: every batch is sorted on its context as above, copied device
// to device into buffers of its own and merged, gathered and deflated on ctxs[0]'s device after the last batch (k_bammerge.hip); when the
// runs outgrow sd->hbm_budget the run ends as bwahip_stream_run_bam_sorted does, on the host
extern "C" int bwahip_stream_run_bam_sorted_dev(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd)
{
	SortedDevReq r;
	r.sd = sd; r.fall_back = true;
	return stream_run_sorted_dev(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, hdr_line, st, r);
}

// The two coordinate-sorted entry points with the BAI index of the file on bai_fd: the same sinks, which then count the header's member
// bytes and let a builder listen to the host merge, or run the device merger's index stage (k_bai.hip)
extern "C" int bwahip_stream_run_bam_sorted_bai(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                const char *fq1, const char *fq2, int out_fd, const char *hdr_line, int level, bwahip_stream_t *st, bwahip_sort_t *so, int bai_fd)
{
	if (!so) return BWAHIP_EINVAL;
	SortedSink sink(hdr_line, level, so);
	sink.with_bai = true; sink.bai_fd = bai_fd;
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, sink);
}

extern "C" int bwahip_stream_run_bam_sorted_dev_bai(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                    const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, int bai_fd)
{
	SortedDevReq r;
	r.sd = sd; r.fall_back = true; r.with_index(bai_fd);
	return stream_run_sorted_dev(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, hdr_line, st, r);
}

// bwahip_stream_run_bam_sorted_dev_bai with duplicate marking (k_markdup.hip): the batches leave their contexts with templates and descriptors,
// the finish marks before it gathers; a run that does not fit ends the call (no host fall-back)
extern "C" int bwahip_stream_run_bam_sorted_dev_markdup(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                        const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, int bai_fd,
                                                        bwahip_markdup_stats_t *ms)
{
	SortedDevReq r;
	r.sd = sd; r.with_index(bai_fd); r.mark = true; r.ms = ms;
	return stream_run_sorted_dev(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, hdr_line, st, r);
}

// The two entry points above with the QC summary of the file on qc_fd (k_qc.hip): the merger is armed, so its finish runs the stage after the
// marking and before the first gather; after a fall-back (markdup == 0 only) a host builder listens to the host merge
extern "C" int bwahip_stream_run_bam_sorted_dev_qc(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                   const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, int bai_fd,
                                                   bwahip_markdup_stats_t *ms, int markdup, const bwahip_qc_opt_t *qo, int qc_fd, bwahip_qc_stats_t *qs)
{
	if (!sd || !qo) return BWAHIP_EINVAL;
	SortedDevReq r;
	r.sd = sd; r.fall_back = !markdup; r.with_index(bai_fd); r.mark = markdup != 0; r.ms = ms;
	r.qc = qo; r.qc_fd = qc_fd; r.qs = qs;
	return stream_run_sorted_dev(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, hdr_line, st, r);
}

// The device-merged entry points with the pileup of the file on pu_fd (k_pileup.hip), over the contexts' reference: marking, index and QC
// summary as asked, never a fall-back
extern "C" int bwahip_stream_run_bam_sorted_dev_pileup(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                       const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, int bai_fd,
                                                       int mark, bwahip_markdup_stats_t *ms, const bwahip_qc_opt_t *qc, int qc_fd, bwahip_qc_stats_t *qs,
                                                       const bwahip_pileup_opt_t *pu, int pu_fd, bwahip_pileup_stats_t *ps)
{
	if (!sd || !pu) return BWAHIP_EINVAL;
	SortedDevReq r;
	r.sd = sd; r.with_index(bai_fd); r.mark = mark != 0; r.ms = ms;
	r.qc = qc; r.qc_fd = qc_fd; r.qs = qs;
	r.pu = pu; r.pu_fd = pu_fd; r.ps = ps;
	return stream_run_sorted_dev(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, hdr_line, st, r);
}

// The device-merged entry points in one, for samples whose record bytes outgrow HBM: runs that do not fit sd->hbm_budget are held spilled
// (SpillSortedSink); mark, bai_fd >= 0 and qc != NULL choose the stages.  Never a host fall-back: sd->tmp_dir, mem_budget and level are
// not looked at
extern "C" int bwahip_stream_run_bam_sorted_dev_spill(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                      const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, bwahip_spill_t *sp,
                                                      int bai_fd, int mark, bwahip_markdup_stats_t *ms, const bwahip_qc_opt_t *qc, int qc_fd, bwahip_qc_stats_t *qs)
{
	if (!sd || !sp) return BWAHIP_EINVAL;
	SortedDevReq r;
	r.sd = sd; r.sp = sp; r.with_index(bai_fd); r.mark = mark != 0; r.ms = ms;
	r.qc = qc; r.qc_fd = qc_fd; r.qs = qs;
	return stream_run_sorted_dev(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, hdr_line, st, r);
}

// bwahip_stream_run_bam_sorted_dev_spill with the recalibration table of the file on rc_fd (k_recal.hip): the same sink, its merger armed for the
// table over the contexts' reference and the caller's mask
extern "C" int bwahip_stream_run_bam_sorted_dev_recal(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                      const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, bwahip_spill_t *sp,
                                                      int bai_fd, int mark, bwahip_markdup_stats_t *ms, const bwahip_qc_opt_t *qc, int qc_fd, bwahip_qc_stats_t *qs,
                                                      const bwahip_recal_opt_t *rc, const uint8_t *mask, int rc_fd, bwahip_recal_stats_t *rs)
{
	if (!sd || !sp || !rc) return BWAHIP_EINVAL;
	SortedDevReq r;
	r.sd = sd; r.sp = sp; r.with_index(bai_fd); r.mark = mark != 0; r.ms = ms;
	r.qc = qc; r.qc_fd = qc_fd; r.qs = qs;
	r.rc = rc; r.mask = mask; r.rc_fd = rc_fd; r.rs = rs;
	return stream_run_sorted_dev(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, hdr_line, st, r);
}
