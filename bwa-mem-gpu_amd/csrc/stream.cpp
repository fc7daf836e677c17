// The batch driver behind the C ABI: FASTQ files in -> SAM text out, over any number of contexts.  What superBatchMain
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
//                     drainer  copies the SAM text back and hands it to the writer (batch k-1);
//   one writer      writes the batches' SAM in batch order to the caller's file descriptor, and gives every buffer back to the
//                   context it came from once its bytes are on the descriptor.
//
// A context has two sets of input buffers and two of output buffers; a set is reused only when its consumer has said it is done with
// it (Pipe::in_free / out_free below).  A stager asks for a batch when it has a free input set, so batches go to whichever context
// frees first and staging runs ahead of a context that still computes; results do not depend on which context took a batch
// (tests/test_gpu_multi.py).  No data-path collective: SURVEY.md 8(e).
#include "../../include/bwahip.h"
#include "stream_pipe.h"
#include "ctx_internal.h"                                       // the contexts' devices, the runs a device merger holds (k_bammerge.hip)
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

struct Driver {
	// reader side
	std::mutex mu_read;
	bwahip_fastq *rd = nullptr;
	int64_t n_processed = 0, next_seq = 0, max_reads = 0;
	bool eof = false;
	// writer side
	std::mutex mu;
	std::condition_variable cv_item, cv_done;
	struct Item { const char *p; int64_t len; int ctx, out; const uint64_t *keys; const int64_t *rec_off; int64_t n_rec; int64_t raw_len; DevRun *run; };   // ctx / out: the output set the bytes sit in; keys, rec_off: coordinate-sorted BAM; run (bam == 4): the batch as a run in HBM -- no bytes, and the output set went back to its context already
	std::map<int64_t, Item> ready;                               // finished batches waiting for their turn
	int64_t written = 0;                                         // batches [0, written) are on the descriptor
	int workers_left = 0;
	int rc = 0;                                                  // first error (the stages and the writer stop on it)
	std::atomic<bool> stop{false};                               // rc != 0, readable without the lock
	std::function<void()> wake_all;                              // wakes every context's threads (failure)
	std::function<void(const Item&, int64_t, double, double)> on_written;   // gives the output set back to its context
	int fd = -1;
	int bam = 0, level = 0, deflate_threads = 1;                 // bwahip_stream_run_bam: the batches' records go through the BGZF writer
	bwahip_bam_merger *merger = nullptr;                         // bam == 2 (bwahip_stream_run_bam_sorted): every batch is a sorted run of the merger instead
	double sort_ms = 0;
	// bam == 4 (bwahip_stream_run_bam_sorted_dev): every batch is a run of the device merger while the HBM budget holds; from the first run
	// that does not fit (or came back downloaded because its buffers could not be allocated) every run goes to the host merger
	bwahip_bam_devmerger *devm = nullptr;
	bwahip_sort_dev_t *sd = nullptr;
	bwahip_ctx *ctx0 = nullptr;
	int64_t hbm_budget = 0, held_raw = 0, held_rec = 0;
	int piece_blocks = 0;
	std::atomic<bool> fell_back{false};                          // read by the drainers: from now on they download
	hipStream_t fb_stream = nullptr;                             // the fall-back's downloads: one pinned buffer each for records, keys and offsets
	HostBuf fb_rec, fb_keys, fb_off;
	bwahip_bgzf_stats_t bz = { 0, 0, 0, 0, 0 };                  // bam == 3 (bwahip_stream_run_bam_dev): the batches arrive as BGZF members and are only written
	int64_t sam_bytes = 0;
	double t_last_write = 0, write_s = 0;

	void fail(int code) { { std::lock_guard<std::mutex> lk(mu); if (!rc) rc = code; stop = true; } cv_item.notify_all(); cv_done.notify_all(); if (wake_all) wake_all(); }
	bool failed() { return stop.load(); }

	// a run in HBM -> the host merger, through the pinned buffers; the run is freed whatever happens
	int run_to_host(int64_t run_no, DevRun *r)
	{
		int rc = hipSetDevice(ctx0->device) == hipSuccess ? 0 : BWAHIP_ENODEV;
		if (!rc && !fb_stream && hipStreamCreateWithFlags(&fb_stream, hipStreamNonBlocking) != hipSuccess) rc = BWAHIP_ENODEV;
		if (!rc && ((rc = fb_rec.ensure((size_t)r->len + 1)) || (rc = fb_keys.ensure((size_t)(r->n_rec + 1) * 8)) || (rc = fb_off.ensure((size_t)(r->n_rec + 1) * 8)))) {}
		if (!rc) rc = bam_devrun_download(r, (uint8_t*)fb_rec.p, (uint64_t*)fb_keys.p, (int64_t*)fb_off.p, fb_stream);
		if (!rc) rc = bwahip_bam_merger_add(merger, run_no, (const uint8_t*)fb_rec.p, r->len, (const uint64_t*)fb_keys.p, (const int64_t*)fb_off.p, r->n_rec);
		bam_devrun_free(r);
		return rc;
	}
	// run `at` does not fit: the host merger is opened (only now is tmp_dir looked at) and takes the runs held so far, in run order
	int fall_back(int64_t at)
	{
		int rc = bwahip_bam_merger_open(sd->tmp_dir, sd->mem_budget, &merger);
		std::vector<std::pair<int64_t, DevRun*>> held;
		bam_devmerger_take_runs(devm, &held);
		for (auto &h : held) { if (!rc) rc = run_to_host(h.first, h.second); else bam_devrun_free(h.second); }
		fell_back = true; sd->fell_back = 1; sd->fell_back_at_run = at;
		return rc;
	}
	void fb_release()
	{
		if (ctx0) (void)hipSetDevice(ctx0->device);
		if (fb_stream) { (void)hipStreamDestroy(fb_stream); fb_stream = nullptr; }
		fb_rec.release(); fb_keys.release(); fb_off.release();
	}

	void writer()
	{
		for (;;) {
			Item it;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv_item.wait(lk, [&] { return rc || ready.count(written) || (workers_left == 0 && ready.empty()); });
				if (rc || !ready.count(written)) return;
				it = ready[written];
				ready.erase(written);
			}
			const double t0 = now_s();
			int64_t o = 0;
			if (bam == 4) {
				int r = 0;
				if (!fell_back) {                                       // in input order, so the decision depends on the input and the budget alone
					const bool fits = it.run && bwahip_bam_devmerge_hbm_need(held_raw + it.raw_len, held_rec + it.n_rec, written + 1, piece_blocks) <= hbm_budget;
					if (!fits) r = fall_back(written);
				}
				if (!r && !fell_back) { if (!(r = bam_devmerger_adopt(devm, written, it.run))) { it.run = nullptr; held_raw += it.raw_len; held_rec += it.n_rec; } }
				else if (!r && it.run) { r = run_to_host(written, it.run); it.run = nullptr; }
				else if (!r) r = bwahip_bam_merger_add(merger, written, (const uint8_t*)it.p, it.len, it.keys, it.rec_off, it.n_rec);
				if (it.run) bam_devrun_free(it.run);                    // refused, or the fall-back failed before its turn
				if (r) { fail(r); return; }
				o = it.len;
			} else if (bam == 2) {                                       // the merger copies (or spills) the run: the set goes back at once
				const int r = bwahip_bam_merger_add(merger, written, (const uint8_t*)it.p, it.len, it.keys, it.rec_off, it.n_rec);
				if (r) { fail(r); return; }
				o = it.len;
			} else if (bam == 1) {
				const int r = bwahip_bgzf_write(fd, it.p, it.len, level, deflate_threads);
				if (r) { fail(r); return; }
				o = it.len;
			}
			while (fd >= 0 && o < it.len) {
				const ssize_t w = write(fd, it.p + o, (size_t)(it.len - o > (1ll << 30) ? (1ll << 30) : it.len - o));
				if (w < 0) { if (errno == EINTR) continue; fprintf(stderr, "[bwahip] writing the SAM text failed: %s\n", strerror(errno)); fail(BWAHIP_EIO); return; }
				o += w;
			}
			int64_t seq_no;
			{
				std::lock_guard<std::mutex> lk(mu);
				seq_no = written++; sam_bytes += bam == 3 ? it.raw_len : it.len; t_last_write = now_s(); write_s += t_last_write - t0;
			}
			cv_done.notify_all();
			on_written(it, seq_no, t0, t_last_write);
		}
	}
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

// bam: 0 = SAM text as it comes; 1 = BAM: header, every batch's records through the BGZF writer in input order, the EOF block;
// 2 = coordinate-sorted BAM: every batch leaves its context sorted and becomes a run of the merger (the batch number is the run number);
// after the last batch: header, the merge of the runs through the BGZF writer, the EOF block
static int stream_run(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                      const char *fq1, const char *fq2, int out_fd, bwahip_stream_t *st, int bam, const char *hdr_line, int level, bwahip_sort_t *so = nullptr, bwahip_bgzf_stats_t *bs = nullptr,
                      bwahip_sort_dev_t *sd = nullptr)
{
	if (!ctxs || n_ctx < 1 || n_ctx > 256 || !opt || !fq1 || !st || (bam == 2 && !so) || (bam == 3 && !bs) || (bam == 4 && !sd)) return BWAHIP_EINVAL;
	for (int i = 0; i < n_ctx; ++i) if (!ctxs[i]) return BWAHIP_EINVAL;
	if (bam && (level < 0 || level > 9)) return BWAHIP_EINVAL;
	if (bam == 4) {
		for (int i = 1; i < n_ctx; ++i) if (ctxs[i]->device != ctxs[0]->device) return BWAHIP_EINVAL;   // the runs of all contexts meet in one device's merger
		if (sd->piece_blocks > 4096 || sd->hbm_budget < 0 || sd->level < 0 || sd->level > 9) return BWAHIP_EINVAL;
	}
	const int bam_pipe = bam == 4 ? 2 : bam;                       // what the contexts compute: mode 4 is mode 2 up to the stage-out
	// actual_chunk_size (fastmap.c:304): -K when given, else chunk_size * n_threads
	const int64_t chunk = st->chunk_bases > 0 ? st->chunk_bases : (int64_t)opt->chunk_size * (opt->n_threads > 0 ? opt->n_threads : 1);
	bwahip_opt_t o = *opt;
	if (fq2) o.flag |= BWAHIP_F_PE;
	// opt->n_threads is the host-thread budget of the whole run; BAM: half of it deflates, the other half stages the batches
	// (bam == 3: the GPU deflates, all of it stages)
	const int n_deflate = bam && bam != 3 && bam != 4 ? (opt->n_threads / 2 > 1 ? opt->n_threads / 2 : 1) : 0;
	const int n_stage = bam && opt->n_threads > n_deflate ? opt->n_threads - n_deflate : opt->n_threads;
	o.n_threads = n_stage / n_ctx > 1 ? n_stage / n_ctx : 1;
	Driver d;
	d.fd = out_fd; d.max_reads = st->max_reads;
	d.bam = bam; d.level = level; d.deflate_threads = n_deflate;
	struct Sorted {                                              // the header waits for the merge; the merger and its files go whatever happens
		uint8_t *hdr = nullptr; int64_t hlen = 0; bwahip_bam_merger *m = nullptr; bwahip_bam_devmerger *dm = nullptr;
		~Sorted() { free(hdr); bwahip_bam_merger_close(m); bwahip_bam_devmerger_close(dm); }
	} sorted;
	if (bam == 4) {
		sd->fell_back = 0; sd->fell_back_at_run = 0; sd->n_records = sd->n_runs = sd->spilled_bytes = 0; sd->sort_ms = sd->merge_s = 0;
		memset(&sd->dev, 0, sizeof sd->dev);
		int hr = bwahip_bam_header_sorted(bwahip_bns(ctxs[0]), hdr_line, &sorted.hdr, &sorted.hlen);
		if (!hr) hr = bwahip_bam_devmerger_open(ctxs[0], sd->piece_blocks, &sorted.dm);
		if (hr) return hr;
		d.devm = sorted.dm; d.sd = sd; d.ctx0 = ctxs[0];
		d.piece_blocks = sd->piece_blocks > 0 ? sd->piece_blocks : ctxs[0]->knobs.sorted_piece_blocks;
		d.hbm_budget = sd->hbm_budget;
		if (!d.hbm_budget) {                                         // half of what the device has free now
			size_t mem_free = 0, mem_total = 0;
			HIP_TRY(hipSetDevice(ctxs[0]->device));
			HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
			d.hbm_budget = (int64_t)(mem_free / 2);
		}
	}
	if (bam == 2) {
		so->n_records = so->n_runs = so->spilled_bytes = 0; so->sort_ms = so->merge_s = 0;
		int hr = bwahip_bam_header_sorted(bwahip_bns(ctxs[0]), hdr_line, &sorted.hdr, &sorted.hlen);
		if (!hr) hr = bwahip_bam_merger_open(so->tmp_dir, so->mem_budget, &sorted.m);
		if (hr) return hr;
		d.merger = sorted.m;
	}
	if (bam == 1 || bam == 3) {
		uint8_t *hdr = nullptr; int64_t hlen = 0;
		int hr = bwahip_bam_header(bwahip_bns(ctxs[0]), hdr_line, &hdr, &hlen);
		if (!hr) { hr = bwahip_bgzf_write(out_fd, hdr, hlen, level, 1); free(hdr); }
		if (hr) return hr;
	}
	const double t_call = now_s();
	int rc = bwahip_fastq_open_mt(fq1, fq2, st->reader_threads, &d.rd);
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
	d.on_written = [&](const Driver::Item &it, int64_t seq_no, double t0, double t1) {
		Pipe &p = pipes[it.ctx];
		if (it.p) {                                                  // (a run that stayed in HBM: its drainer gave the set back, and it may be in use again)
			{ std::lock_guard<std::mutex> lk(p.mu); p.out_free[it.out] = true; }
			p.cv.notify_all();
		}
		span("write", seq_no, it.ctx, t0, t1);
	};
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
			const int r = pipe_stage_in(ctxs[w], j.in, &o, j.n, seqs, bam_pipe, &t_copy);
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
			const int r = pipe_compute(ctxs[w], j.in, j.out, &o, j.np0, pes0, bam_pipe, &t_hot);
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
			const char *sam = nullptr; int64_t len = 0;
			double t_end = 0;
			if (bam == 4 && !d.fell_back) {                           // the run stays in HBM: no download, the writer gets an item without bytes
				DevRun *run = nullptr; int64_t raw = 0, nr = 0; double sort_ms = 0;
				const int r4 = pipe_stage_out_devrun(ctxs[w], j.out, &run, &raw, &nr, &sort_ms, &t_end);
				if (r4) { d.fail(r4); break; }
				if (run) {
					const double t1 = now_s();
					{ std::lock_guard<std::mutex> lk(p.mu); p.in_free[j.in] = true; p.out_free[j.out] = true; }   // the copies have ended: both sets go back at once
					p.cv.notify_all();
					span("final", j.seq_no, w, j.t_final, t_end); span("d2d", j.seq_no, w, t_end, t1);
					{
						std::lock_guard<std::mutex> lk(d.mu);
						if (d.rc) bam_devrun_free(run);                     // the writer has gone: nobody would take it
						else d.ready[j.seq_no] = { nullptr, raw, w, j.out, nullptr, nullptr, nr, raw, run };
						d.sort_ms += sort_ms;
					}
					d.cv_item.notify_all();
					continue;
				}
			}                                                         // (its buffers could not be allocated: downloaded as any run after a fall-back, which it causes)
			const int r = pipe_stage_out(ctxs[w], j.out, &sam, &len, &t_end);
			const double t1 = now_s();
			if (r) { d.fail(r); break; }
			{ std::lock_guard<std::mutex> lk(p.mu); p.in_free[j.in] = true; }   // the kernels that read the input set have ended
			p.cv.notify_all();
			span("final", j.seq_no, w, j.t_final, t_end); span("d2h", j.seq_no, w, t_end, t1);
			const uint64_t *keys = nullptr; const int64_t *rec_off = nullptr; int64_t n_rec = 0;
			double sort_ms = 0;
			if (bam_pipe == 2) { const int r2 = pipe_stage_out_sorted(ctxs[w], j.out, &keys, &rec_off, &n_rec, &sort_ms); if (r2) { d.fail(r2); break; } }
			int64_t raw_len = len, n_blocks = 0, n_stored = 0;
			double deflate_ms = 0;
			if (bam == 3) { const int r3 = pipe_stage_out_bgzf(ctxs[w], j.out, &raw_len, &n_blocks, &n_stored, &deflate_ms); if (r3) { d.fail(r3); break; } }
			{
				std::lock_guard<std::mutex> lk(d.mu);
				d.ready[j.seq_no] = { sam, len, w, j.out, keys, rec_off, n_rec, raw_len, nullptr };
				d.sort_ms += sort_ms;
				if (bam == 3) { d.bz.raw_bytes += raw_len; d.bz.bgzf_bytes += len; d.bz.n_blocks += n_blocks; d.bz.n_stored += n_stored; d.bz.deflate_ms += deflate_ms; }
			}
			d.cv_item.notify_all();
		}
		// the buffers must outlive their write
		{ std::unique_lock<std::mutex> lk(p.mu); p.cv.wait(lk, [&] { if (d.failed()) return true; for (int i = 0; i < PIPE_SETS; ++i) if (!p.out_free[i]) return false; return true; }); }
		{ std::lock_guard<std::mutex> lk(d.mu); --d.workers_left; }
		d.cv_item.notify_all();
	};
	std::thread wr([&] { d.writer(); });
	std::vector<std::thread> th;
	for (int w = 0; w < n_ctx; ++w) { th.emplace_back(stager, w); th.emplace_back(compute, w); th.emplace_back(drainer, w); }
	for (auto &t : th) t.join();
	wr.join();
	for (int w = 0; w < n_ctx; ++w) pipe_close(ctxs[w]);           // after a failure kernels and copies may still be queued: nothing is left running
	std::vector<double> wait_s(n_ctx), busy_s(n_ctx);
	for (int w = 0; w < n_ctx; ++w) { wait_s[w] = pipes[w].wait_s; busy_s[w] = pipes[w].busy_s; }
	if (bam == 2 && !d.rc) {                                     // every run is with the merger: header, merge, end-of-file block
		const double t0 = now_s();
		int r = bwahip_bgzf_write(out_fd, sorted.hdr, sorted.hlen, level, 1);
		// the staging threads have ended, so the merge's BGZF writer gets all host threads, not the n_deflate the unsorted writer
		// shares the host with them for (the bytes do not depend on the number of threads)
		if (!r) r = bwahip_bam_merger_finish(sorted.m, out_fd, level, opt->n_threads > 1 ? opt->n_threads : 1);
		if (r) d.rc = r;
		d.write_s += now_s() - t0;
		bwahip_bam_merger_stats(sorted.m, &so->n_records, &so->n_runs, &so->spilled_bytes, &so->merge_s);
		so->sort_ms = d.sort_ms;
	}
	if (bam == 4) {
		for (auto &kv : d.ready) if (kv.second.run) bam_devrun_free(kv.second.run);   // after a failure: runs nobody took
		d.ready.clear();
		d.fb_release();
		sorted.m = d.merger;                                        // closed (and its files removed) whatever happens
	}
	if (bam == 4 && !d.rc) {                                     // every run is with one of the two mergers: header, merge, end-of-file block
		const double t0 = now_s();
		const bool fb = d.fell_back;
		int r = bwahip_bgzf_write(out_fd, sorted.hdr, sorted.hlen, fb ? sd->level : 1, 1);
		if (!r && fb) {                                             // from here on this is bwahip_stream_run_bam_sorted at sd->level
			r = bwahip_bam_merger_finish(sorted.m, out_fd, sd->level, opt->n_threads > 1 ? opt->n_threads : 1);
			bwahip_bam_merger_stats(sorted.m, &sd->n_records, &sd->n_runs, &sd->spilled_bytes, &sd->merge_s);
		} else if (!r) {
			r = bwahip_bam_devmerger_finish(sorted.dm, out_fd, &sd->dev);
			sd->n_records = sd->dev.n_records; sd->n_runs = sd->dev.n_runs; sd->merge_s = sd->dev.finish_s;
		}
		if (r) d.rc = r;
		d.write_s += now_s() - t0;
		sd->sort_ms = d.sort_ms;
	}
	if (bam && !d.rc) { const int r = bwahip_bgzf_eof(out_fd); if (r) d.rc = r; d.t_last_write = now_s(); }
	const double t_joined = now_s();
	g_reaper.close_later(d.rd);
	if (log) {
		for (const Span &x : spans) fprintf(stderr, "[bwahip] span %s batch %lld ctx %d %.3f %.3f\n", x.stage, (long long)x.batch, x.ctx, (x.t0 - t_call) * 1e3, (x.t1 - t_call) * 1e3);
		fprintf(stderr, "[bwahip] stream: %lld batches on %d contexts, %ld buffer reallocations in this pass\n", (long long)d.next_seq, n_ctx, pipe_realloc_count() - reallocs0);
	}
	if (log)
		fprintf(stderr, "[bwahip] stream: open %.1f ms, first batch in -> last SAM byte out %.1f ms, joining the threads %.1f ms, handing the reader to the closer %.1f ms\n",
		        (t_start - t_call) * 1e3, (d.t_last_write - t_start) * 1e3, (t_joined - d.t_last_write) * 1e3, (now_s() - t_joined) * 1e3);
	if (bs) *bs = d.bz;
	st->n_reads = d.n_processed; st->n_batches = d.next_seq; st->sam_bytes = d.sam_bytes;
	st->seconds = d.t_last_write - t_call; st->write_s = d.write_s;
	for (int w = 0; w < n_ctx; ++w) { st->reader_wait_s += wait_s[w]; st->gpu_busy_s += busy_s[w]; }
	return d.rc;
}

extern "C" int bwahip_stream_run(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                 const char *fq1, const char *fq2, int out_fd, bwahip_stream_t *st)
{
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, 0, nullptr, 0);
}

// FASTQ files in -> a BAM file out: bwahip_stream_run with bwahip_process_seqs_bam in the workers and the BGZF writer behind them
extern "C" int bwahip_stream_run_bam(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                     const char *fq1, const char *fq2, int out_fd, const char *hdr_line, int level, bwahip_stream_t *st)
{
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, 1, hdr_line, level);
}

// FASTQ files in -> a coordinate-sorted BAM file out: every batch is sorted on its context (bwahip_process_seqs_bam_sorted's kernels) and
// merged on the host (bwahip_bam_merger_*); the bytes depend on the input and the options alone
extern "C" int bwahip_stream_run_bam_sorted(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                            const char *fq1, const char *fq2, int out_fd, const char *hdr_line, int level, bwahip_stream_t *st, bwahip_sort_t *so)
{
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, 2, hdr_line, level, so);
}

// FASTQ files in -> a BAM file out with the BGZF blocks of the records made on the GPU (k_bgzf.hip): the header through the host writer,
// every batch's members written as they come back, the end-of-file block; no deflate workers, all host threads stage
extern "C" int bwahip_stream_run_bam_dev(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                         const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_bgzf_stats_t *bs)
{
	if (!bs) return BWAHIP_EINVAL;
	memset(bs, 0, sizeof *bs);
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, 3, hdr_line, 1, nullptr, bs);
}

// FASTQ files in -> a coordinate-sorted BAM file out with the runs kept in HBM: every batch is sorted on its context as above, copied device
// to device into buffers of its own and merged, gathered and deflated on ctxs[0]'s device after the last batch (k_bammerge.hip); when the
// runs outgrow sd->hbm_budget the run ends as bwahip_stream_run_bam_sorted does, on the host
extern "C" int bwahip_stream_run_bam_sorted_dev(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                                const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd)
{
	if (!sd) return BWAHIP_EINVAL;
	return stream_run(ctxs, n_ctx, opt, pes0, fq1, fq2, out_fd, st, 4, hdr_line, 1, nullptr, nullptr, sd);
}
