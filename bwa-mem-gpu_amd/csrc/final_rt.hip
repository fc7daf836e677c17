// Host sequencing of the GPU finalisation (regions of mem_align1_core in HBM -> SAM text in HBM) and the C ABI entry
// bwahip_process_seqs == mem_process_seqs (bwamem.h:69).  Kernels: k_final.hip (mark primary, selection, CIGAR/NM/MD/mapQ),
// k_sam.hip (SAM text), k_pair.hip (insert sizes, mate rescue, pairing).
#include "ctx_internal.h"
#include <atomic>
#include <thread>
#include <math.h>
#include <algorithm>
#include <chrono>

#include <dlfcn.h>
// The host finalisation is test infrastructure (csrc/host_final.cpp, built as libbwahip_hostfinal.so beside this library) and not linked
// in: the knobs gpu_final = 0 / gpu_pair = 0 load it on demand.  Without it those knobs are an error -- there is no CPU path in the product.
typedef int (*host_final_fn)(bwahip_ctx*, const bwahip_opt_t*, int64_t, int, bwahip_seq_t*, const bwahip_pestat_t*);
static host_final_fn load_host_final()
{
	static host_final_fn fn = nullptr;
	static bool tried = false;
	if (tried) return fn;
	tried = true;
	Dl_info di;
	std::string path = "libbwahip_hostfinal.so";
	if (dladdr((const void*)&bwahip_version, &di) && di.dli_fname) {
		const std::string self = di.dli_fname;
		const size_t sl = self.rfind('/');
		if (sl != std::string::npos) path = self.substr(0, sl + 1) + path;
	}
	void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
	if (h) fn = (host_final_fn)dlsym(h, "bwahip_process_seqs_host");
	if (!fn) fprintf(stderr, "[bwahip] gpu_final / gpu_pair = 0 need the test library %s (%s)\n", path.c_str(), h ? "symbol missing" : dlerror());
	return fn;
}

// contig names and annotations as flat byte tables (RNAME, SA / XA entries, XR)
int final_setup(bwahip_ctx *c)
{
	const bwahip_bns_t &bns = c->host.bns;
	std::vector<uint8_t> names, anno;
	std::vector<int> noff(bns.n_seqs + 1, 0), aoff(bns.n_seqs + 1, 0);
	for (int i = 0; i < bns.n_seqs; ++i) {
		const char *nm = bns.anns[i].name ? bns.anns[i].name : "", *an = bns.anns[i].anno ? bns.anns[i].anno : "";
		names.insert(names.end(), nm, nm + strlen(nm)); noff[i + 1] = (int)names.size();
		anno.insert(anno.end(), an, an + strlen(an)); aoff[i + 1] = (int)anno.size();
	}
	names.resize(names.size() + 64, 0); anno.resize(anno.size() + 64, 0);
	int rc;
	if ((rc = dev_upload(c->d_ctg_names, names.data(), names.size(), c->stream)) || (rc = dev_upload(c->d_ctg_name_off, noff.data(), noff.size() * 4, c->stream)) ||
	    (rc = dev_upload(c->d_ctg_anno, anno.data(), anno.size(), c->stream)) || (rc = dev_upload(c->d_ctg_anno_off, aoff.data(), aoff.size() * 4, c->stream)) ||
	    (rc = c->d_fmisc.ensure(256))) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	return 0;
}

// mem_pestat (bwamem_pair.c:72-134) from the insert-size histogram the GPU collected: the sorted list of the reference is the
// histogram read in ascending order, so percentiles, mean and (added in the same order) the sum of squares come out the same.
static void pestat_from_hist(const bwahip_opt_t *opt, const std::vector<unsigned> &hist, bwahip_pestat_t pes[4])
{
	const int W = opt->max_ins + 1;
	uint64_t cnt[4] = { 0, 0, 0, 0 };
	memset(pes, 0, 4 * sizeof(bwahip_pestat_t));
	for (int d = 0; d < 4; ++d) for (int v = 1; v < W; ++v) cnt[d] += hist[(size_t)d * W + v];
	for (int d = 0; d < 4; ++d) {
		bwahip_pestat_t *r = &pes[d];
		const unsigned *h = &hist[(size_t)d * W];
		const uint64_t nq = cnt[d];
		if (nq < 10) { r->failed = 1; continue; }                    // MIN_DIR_CNT
		auto at = [&](uint64_t idx) { uint64_t run = 0; for (int v = 1; v < W; ++v) { run += h[v]; if (run > idx) return v; } return W - 1; };
		const int p25 = at((uint64_t)(int)(.25 * nq + .499)), p75 = at((uint64_t)(int)(.75 * nq + .499));
		r->low = (int)(p25 - 2.0 * (p75 - p25) + .499);              // OUTLIER_BOUND
		if (r->low < 1) r->low = 1;
		r->high = (int)(p75 + 2.0 * (p75 - p25) + .499);
		uint64_t x = 0;
		r->avg = 0;
		for (int v = 1; v < W; ++v) if (v >= r->low && v <= r->high) { r->avg += (double)v * h[v]; x += h[v]; }   // integers: exact in any order
		r->avg /= x;
		r->std = 0;
		for (int v = 1; v < W; ++v) if (v >= r->low && v <= r->high) { const double t = ((double)v - r->avg) * ((double)v - r->avg); for (unsigned k = 0; k < h[v]; ++k) r->std += t; }
		r->std = sqrt(r->std / x);
		r->low = (int)(p25 - 3.0 * (p75 - p25) + .499);              // MAPPING_BOUND
		r->high = (int)(p75 + 3.0 * (p75 - p25) + .499);
		if (r->low > r->avg - 4.0 * r->std) r->low = (int)(r->avg - 4.0 * r->std + .499);      // MAX_STDDEV
		if (r->high < r->avg + 4.0 * r->std) r->high = (int)(r->avg + 4.0 * r->std + .499);
		if (r->low < 1) r->low = 1;
	}
	uint64_t mx = 0;
	for (int d = 0; d < 4; ++d) mx = mx > cnt[d] ? mx : cnt[d];
	for (int d = 0; d < 4; ++d) if (pes[d].failed == 0 && cnt[d] < (int)mx * 0.05) pes[d].failed = 1;   // MIN_DIR_RATIO
}

// The insert-size statistics as k_matesw and k_pair read them (PairLaunch::pes) and, per direction, .721 * log(2 * erfc(|ns| / sqrt 2)) for
// every admissible distance (bwamem_pair.c:243-244), by the host's libm, uploaded as PairLaunch::pair_tab / tab_off.  widest: the largest
// high - low of a live direction.  run_pe_rescue and bwahip_kat_pair both come through here.
static int pair_stats(bwahip_ctx *c, const bwahip_pestat_t pes[4], PairLaunch &pl, int64_t &widest)
{
	std::vector<double> tab;
	widest = 0;
	for (int d = 0; d < 4; ++d) {
		pl.pes[d].low = pes[d].low; pl.pes[d].high = pes[d].high; pl.pes[d].failed = pes[d].failed; pl.pes[d].pad = 0; pl.pes[d].avg = pes[d].avg; pl.pes[d].std = pes[d].std;
		pl.tab_off[d] = (int)tab.size();
		if (pes[d].failed || pes[d].high < pes[d].low) continue;
		if ((int64_t)pes[d].high - pes[d].low > (1 << 26)) return BWAHIP_EINVAL;
		widest = std::max<int64_t>(widest, (int64_t)pes[d].high - pes[d].low);
		for (int64_t dist = pes[d].low; dist <= pes[d].high; ++dist) {
			const double ns = (dist - pes[d].avg) / pes[d].std;
			tab.push_back(.721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)));
		}
	}
	tab.push_back(0.);
	const int rc = dev_upload(c->d_pair_tab, tab.data(), tab.size() * 8, c->stream);
	if (rc) return rc;
	pl.pair_tab = c->d_pair_tab.as<double>();
	return 0;
}

// The paired-end stages before mark-primary: insert-size statistics, mate rescue.  Leaves the per-read lists in d_pe_regs.
// Insert sizes, the lists of both ends, and mate rescue.  The rescue kernels (a handful of pairs, long dependent chains: the GPU is nearly idle
// under them) go to the second stream and are NOT waited for: run_final finalises all other pairs meanwhile and the rescued ones after ev_join.
static int run_pe_rescue(bwahip_ctx *c, const bwahip_opt_t *opt, const DevOpt &dopt, int64_t n_processed, const bwahip_pestat_t *pes0, PairLaunch &pl, int &n_resc_out)
{
	const int n = c->in->n;
	int rc;
	memset(&pl, 0, sizeof pl);
	pl.ix = c->ix; pl.opt = dopt; pl.n_reads = n; pl.seq = c->in->d_seq.as<uint8_t>(); pl.off = c->in->d_off.as<int64_t>(); pl.n_processed = n_processed;
	pl.logtab = c->d_logtab.as<double>();
	pl.incr_insert = c->knobs.incr_insert;
	pl.regs = c->d_regs.as<DevReg>(); pl.reg_base = c->d_reg_base.as<int64_t>(); pl.reg_n = c->d_reg_n.as<int>();
	unsigned long long *fm = c->d_fmisc.as<unsigned long long>();
	pl.err = (int*)(fm + 2); pl.resc_n = (int*)(fm + 4); pl.counters = fm + 5; pl.sw_n = (int*)(fm + 14); pl.queue = (unsigned int*)(fm + 16); pl.sw_n8 = (int*)(fm + 18); pl.paths = fm + 19;   // (PE_PATH_N = 12 slots: up to fm[30] of the 32)
	bwahip_pestat_t pes[4];
	if (pes0) memcpy(pes, pes0, sizeof pes);
	else {
		if (opt->max_ins < 1 || opt->max_ins > (1 << 24)) return BWAHIP_EINVAL;
		const size_t hb = (size_t)4 * (opt->max_ins + 1) * 4;
		if ((rc = c->d_hist.ensure(hb))) return rc;
		HIP_TRY(hipMemsetAsync(c->d_hist.p, 0, hb, c->stream));
		pl.hist = c->d_hist.as<unsigned>();
		if ((rc = launch_pestat(pl, c->stream))) return rc;
		std::vector<unsigned> h((size_t)4 * (opt->max_ins + 1));
		HIP_TRY(hipMemcpyAsync(h.data(), c->d_hist.p, hb, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		pestat_from_hist(opt, h, pes);
	}
	memcpy(c->last_pes, pes, sizeof pes);
	int64_t widest = 0;
	if ((rc = pair_stats(c, pes, pl, widest))) return rc;
	// list capacities after rescue
	if ((rc = c->d_nb.ensure((size_t)n * 4)) || (rc = c->d_pe_cap.ensure((size_t)n * 4)) || (rc = c->d_pe_base.ensure((size_t)(n + 1) * 8)) || (rc = c->d_pe_n.ensure((size_t)n * 4)) ||
	    (rc = c->d_resc.ensure((size_t)(n / 2 + 4) * 4)) || (rc = c->d_resc_flag.ensure((size_t)(n / 2 + 4))) || (rc = c->d_sw_cnt.ensure((size_t)n * 4)) || (rc = c->d_sw_base.ensure((size_t)(n + 1) * 8))) return rc;
	pl.sw_cnt = c->d_sw_cnt.as<int>(); pl.sw_base = c->d_sw_base.as<int64_t>();
	pl.nb = c->d_nb.as<int>(); pl.pe_cap = c->d_pe_cap.as<int>(); pl.pe_base = c->d_pe_base.as<int64_t>(); pl.pe_n = c->d_pe_n.as<int>(); pl.resc_list = c->d_resc.as<int>(); pl.resc_flag = c->d_resc_flag.as<uint8_t>();
	HIP_TRY(hipMemsetAsync(c->d_resc_flag.p, 0, (size_t)(n / 2 + 4), c->stream));
	if ((rc = launch_pe_prepare(pl, c->stream))) return rc;
	if ((rc = launch_scan(pl.pe_cap, c->d_pe_base.as<int64_t>(), n, c->d_scan, c->stream))) return rc;
	if ((rc = launch_scan(pl.sw_cnt, c->d_sw_base.as<int64_t>(), n, c->d_scan, c->stream))) return rc;
	int64_t cap = 0, n_slots = 0;
	HIP_TRY(hipMemcpyAsync(&cap, c->d_pe_base.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(&n_slots, c->d_sw_base.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	{
		const size_t S = (size_t)(n_slots ? n_slots : 1);
		if ((rc = c->d_sw_res.ensure(S * sizeof(SwRes))) || (rc = c->d_sw_tasks.ensure(S * 4)) || (rc = c->d_sw_info.ensure(S * 8))) return rc;
		HIP_TRY(hipMemsetAsync(c->d_sw_res.p, 0, S * sizeof(SwRes), c->stream));
		pl.sw_res = c->d_sw_res.as<SwRes>(); pl.sw_tasks = c->d_sw_tasks.as<int>(); pl.sw_info = c->d_sw_info.as<int2>(); pl.sw_cap = (int)S;
	}
	const size_t R = (size_t)(cap ? cap : 1);
	c->total_regs = cap;                                          // from here on the region slots are the paired-end ones
	if ((rc = c->d_pe_regs.ensure(R * sizeof(DevReg))) || (rc = c->d_pe_tmp.ensure(R * sizeof(DevReg))) || (rc = c->d_pe_keys.ensure(R * 16)) || (rc = c->d_pe_idx.ensure(R * 8))) return rc;
	pl.pe_regs = c->d_pe_regs.as<DevReg>(); pl.pe_tmp = c->d_pe_tmp.as<DevReg>(); pl.pe_keys = c->d_pe_keys.p; pl.pe_idx = c->d_pe_idx.as<int>();
	if ((rc = launch_pe_copy(pl, c->stream))) return rc;
	int n_resc = 0, n_sw_tasks = 0, n_sw_tasks8 = 0;
	HIP_TRY(hipMemcpyAsync(&n_sw_tasks8, pl.sw_n8, 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(&n_resc, pl.resc_n, 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(&n_sw_tasks, pl.sw_n, 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	n_resc_out = n_resc;
	c->last_pe_counters[3] = (unsigned long long)n_resc;
	c->last_sw_tasks = (unsigned long long)n_sw_tasks + (unsigned long long)n_sw_tasks8;
	c->last_sw_ahead[0] = (unsigned long long)n_sw_tasks; c->last_sw_ahead[1] = (unsigned long long)n_sw_tasks8;
	if (n_resc > 0 || n_sw_tasks > 0 || n_sw_tasks8 > 0) {
		HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
		HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
		if ((rc = launch_matesw_sw(pl, n_sw_tasks, n_sw_tasks8, c->in->max_len, c->stream2))) return rc;   // the alignments against the unrescued lists, all at once
		if (n_resc > 0) {
			if ((rc = c->d_resc_ord.ensure(((size_t)3 * n_resc + 8) * 4)) || (rc = launch_resc_order(pl, n_resc, c->d_resc_ord.as<int>(), c->stream2))) return rc;
			const int grid = std::min(n_resc, 2048);
			pl.slab_stride = (matesw_slab_bytes(widest + c->in->max_len) + 255) & ~(size_t)255;
			if ((rc = c->d_ms_slab.ensure(pl.slab_stride * (size_t)grid))) return rc;
			pl.slab = c->d_ms_slab.as<uint8_t>();
			HIP_TRY(hipMemsetAsync(pl.queue, 0, 16, c->stream2));
			if ((rc = launch_matesw(pl, grid, c->stream2))) return rc;
		}
		HIP_TRY(hipEventRecord(c->ev_join, c->stream2));
	}
	return 0;
}

// What k_mark works in and reads, for n reads over c->total_regs region slots: the marked regions and their spare copy, the 16 bytes of scratch
// per slot, the selection, the per-read counts; the launch record with the options, the read id base, the log table and the region lists
// (pe_lists: the ones mate rescue left in d_pe_*, otherwise k_extend's).  run_final and bwahip_kat_mark both come through here, so that the
// known-answer entry launches on the product's own layout; everything else of `f` is zero when this returns.
static int mark_prepare(bwahip_ctx *c, const bwahip_opt_t *opt, int n, int64_t n_processed, bool pe_lists, FinLaunch &f)
{
	int rc;
	const size_t R = (size_t)(c->total_regs ? c->total_regs : 1);
	if ((rc = c->d_fregs.ensure(R * sizeof(FinReg))) || (rc = c->d_fregs2.ensure(R * sizeof(FinReg))) || (rc = c->d_fscr.ensure(R * 16)) || (rc = c->d_need.ensure(R)) ||
	    (rc = c->d_xa_owner.ensure(R * 4)) || (rc = c->d_freg_n.ensure((size_t)n * 4)) || (rc = c->d_npri.ensure((size_t)n * 4)) || (rc = c->d_task_n.ensure((size_t)n * 4)) ||
	    (rc = c->d_rec_n.ensure((size_t)n * 4))) return rc;
	memset(&f, 0, sizeof f);
	f.ix = c->ix; f.opt = make_dev_opt(opt); f.n_reads = n;
	f.n_processed = n_processed; f.logtab = c->d_logtab.as<double>();
	f.regs = c->d_regs.as<DevReg>(); f.reg_base = c->d_reg_base.as<int64_t>(); f.reg_n = c->d_reg_n.as<int>();
	if (pe_lists) { f.regs = c->d_pe_regs.as<DevReg>(); f.reg_base = c->d_pe_base.as<int64_t>(); f.reg_n = c->d_pe_n.as<int>(); }
	f.fregs = c->d_fregs.as<FinReg>(); f.fregs2 = c->d_fregs2.as<FinReg>(); f.freg_n = c->d_freg_n.as<int>(); f.n_pri = c->d_npri.as<int>(); f.scr = c->d_fscr.as<int>();
	f.need = c->d_need.as<uint8_t>(); f.xa_owner = c->d_xa_owner.as<int>(); f.task_n = c->d_task_n.as<int>(); f.rec_n = c->d_rec_n.as<int>();
	return 0;
}

// k_pair's view of the lists k_mark marked (`f`, after mark_prepare): the regions it updates, the spare array its bitonic sort borrows, the
// scratch that holds v, the selection and the per-read answers; with dbg the per-pair record of mem_pair's results (zeroed here: a pair whose
// u is empty leaves it alone).  run_final and bwahip_kat_pair both come through here.
static int pair_wire(bwahip_ctx *c, const FinLaunch &f, int n, bool dbg, PairLaunch &pl)
{
	int rc;
	if ((rc = c->d_pe_read.ensure((size_t)n * sizeof(PeRead)))) return rc;
	pl.fregs = f.fregs; pl.fregs_w = f.fregs; pl.fregs_tmp = f.fregs2; pl.freg_n = f.freg_n; pl.n_pri = f.n_pri; pl.need = f.need; pl.xa_owner = f.xa_owner;
	pl.task_n = f.task_n; pl.rec_n = f.rec_n; pl.scr = f.scr; pl.pe_read = c->d_pe_read.as<PeRead>();
	if (dbg) {
		if ((rc = c->d_pair_dbg.ensure((size_t)(n / 2) * 12))) return rc;
		HIP_TRY(hipMemsetAsync(c->d_pair_dbg.p, 0, (size_t)(n / 2) * 12, c->stream));
		pl.pair_dbg = c->d_pair_dbg.as<int>();
	}
	return 0;
}

// K6 -> K9 over the batch run_pipeline left in HBM.  The text inputs (d_qual, d_names, ...) must be uploaded.
int run_final(bwahip_ctx *c, const bwahip_opt_t *opt, int64_t n_processed, const bwahip_pestat_t *pes0, bool timed, OutForm form, bool host_sam_off, bool pe_stage_stop)
{
	// the two output passes in the batch's format: SAM text (k_sam.hip) or BAM records (k_bam.hip)
	auto launch_out = [&](const FinLaunch &fl, bool write, int lo, int hi) {
		const bool pe_ = (opt->flag & BWAHIP_F_PE) != 0;
		return is_bam(form) ? (pe_ ? launch_bam_pe(fl, write, c->stream, lo, hi) : launch_bam(fl, write, c->stream, lo, hi)) : (pe_ ? launch_sam_pe(fl, write, c->stream, lo, hi) : launch_sam(fl, write, c->stream, lo, hi));
	};
	const int n = c->in->n;
	const bool pe = (opt->flag & BWAHIP_F_PE) != 0;
	BatchOut &o = *c->out;
	o.total = 0; o.n_rec = 0; o.n_blocks = 0; o.n_stored = 0; o.n_tmpl = 0; o.form = form; c->total_tasks = 0;
	const bool sorted = is_sorted(form);                          // the records leave in coordinate order: written to a scratch buffer, sorted into d_sam
	const bool bgzf = form == OutForm::Bgzf;                      // the records leave as BGZF members: written to the same scratch buffer, deflated into d_sam
	if (n == 0) return 0;
	if (pe && (n & 1)) return BWAHIP_EINVAL;
	int rc;
	HIP_TRY(hipMemsetAsync(c->d_fmisc.p, 0, 256, c->stream));
	if (timed) HIP_TRY(hipEventRecord(c->ev[20], c->stream));
	PairLaunch pl;
	const DevOpt dopt_pe = make_dev_opt(opt);
	int n_resc = 0;
	if (pe && (rc = run_pe_rescue(c, opt, dopt_pe, n_processed, pes0, pl, n_resc))) return rc;
	FinLaunch f;
	if ((rc = mark_prepare(c, opt, n, n_processed, pe, f))) return rc;
	const size_t R = (size_t)(c->total_regs ? c->total_regs : 1);
	if ((rc = c->d_aln_of_reg.ensure(R * 4)) || (rc = c->d_rec_list.ensure(R * 8)) || (rc = c->d_xa_list.ensure(R * 8)) ||
	    (rc = c->d_task_base.ensure((size_t)(n + 1) * 8)) || (rc = c->d_sam_len.ensure((size_t)n * 4)) || (rc = o.d_sam_off.ensure((size_t)(n + 1) * 8))) return rc;
	// rg id
	{
		std::string rg = c->rg_id;
		rg.resize(rg.size() + 64, 0);
		if ((rc = dev_upload(c->d_rg, rg.data(), rg.size(), c->stream))) return rc;
	}
	f.seq = c->in->d_seq.as<uint8_t>(); f.off = c->in->d_off.as<int64_t>();
	f.task_base = c->d_task_base.as<int64_t>(); f.aln_of_reg = c->d_aln_of_reg.as<int>();
	f.rec_list = c->d_rec_list.as<const DevAln*>(); f.xa_list = c->d_xa_list.as<const DevAln*>();
	unsigned long long *pool_head = c->d_fmisc.as<unsigned long long>();
	f.pool_head = pool_head; f.redo_n = (int*)(pool_head + 1); f.err = (int*)(pool_head + 2);
	f.qual = c->in->d_qual.as<uint8_t>(); f.qual_off = c->in->d_qual_off.as<int64_t>(); f.names = c->in->d_names.as<uint8_t>(); f.name_off = c->in->d_name_off.as<int64_t>();
	f.comments = c->in->comments(); f.comment_off = c->in->d_comment_off.as<int64_t>();
	f.ctg_names = c->d_ctg_names.as<uint8_t>(); f.ctg_name_off = c->d_ctg_name_off.as<int>(); f.ctg_anno = c->d_ctg_anno.as<uint8_t>(); f.ctg_anno_off = c->d_ctg_anno_off.as<int>();
	f.rg_id = c->d_rg.as<uint8_t>(); f.rg_len = (int)c->rg_id.size();
	f.sam_len = c->d_sam_len.as<int>(); f.sam_off = o.d_sam_off.as<int64_t>();
	if (timed) HIP_TRY(hipEventRecord(c->ev[15], c->stream));
	// paired end: first every pair mate rescue does not touch, while the rescue kernels run on the second stream; then, once those are done, their pairs
	if (pe) { f.resc_flag = pl.resc_flag; f.resc_pairs = pl.resc_list; f.subset = 1; }
	if ((rc = launch_mark_primary(f, !pe, 0, c->stream))) return rc;
	if (pe) {                                                     // mem_pair + the decisions of mem_sam_pe
		if ((rc = pair_wire(c, f, n, pe_stage_stop, pl))) return rc;
		pl.subset = 1;
		if ((rc = launch_pair(pl, 0, c->stream))) return rc;
		HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));      // the rescue kernels (an event not recorded in this batch is complete: no wait)
		if (n_resc > 0) {
			f.subset = 2; pl.subset = 2;
			if ((rc = launch_mark_primary(f, false, n_resc, c->stream))) return rc;
			if ((rc = launch_pair(pl, n_resc, c->stream))) return rc;
		}
		f.subset = 0; pl.subset = 0;
		static_assert(bwahip_ctx::PE_CNT_PATHS == 19 - 5, "PairLaunch::paths starts at d_fmisc[19], the counters at [5]");
		HIP_TRY(hipMemcpyAsync(c->last_pe_counters, pl.counters, bwahip_ctx::PE_CNT_N * 8, hipMemcpyDeviceToHost, c->stream));   // [0..3] as documented; [4..8]: ticks of 10 ns in the window fetch, the alignments and the list clean-up of k_matesw, its longest pair, alignments it ran itself; [14..]: paths
		f.pe_read = pl.pe_read;
		memcpy(f.pes, pl.pes, sizeof f.pes);
	}
	if (pe_stage_stop) {
		if (!pe) return BWAHIP_EINVAL;
		HIP_TRY(hipStreamSynchronize(c->stream));
		int err = 0;
		HIP_TRY(hipMemcpy(&err, c->d_fmisc.as<unsigned long long>() + 2, 4, hipMemcpyDeviceToHost));
		if (err) { fprintf(stderr, "[bwahip] paired-end kernels reported code %d\n", err); return BWAHIP_EINTERNAL; }
		return 0;
	}
	if ((rc = launch_scan(c->d_task_n.as<int>(), c->d_task_base.as<int64_t>(), n, c->d_scan, c->stream))) return rc;
	if (timed) HIP_TRY(hipEventRecord(c->ev[16], c->stream));
	int64_t T = 0;
	HIP_TRY(hipMemcpyAsync(&T, c->d_task_base.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->total_tasks = T;
	const size_t Tn = (size_t)(T ? T : 1);
	if ((rc = c->d_tasks.ensure(Tn * 8)) || (rc = c->d_alns.ensure(Tn * sizeof(DevAln))) || (rc = c->d_fredo.ensure((Tn + 4) * 4)) || (rc = c->d_task_lists.ensure(2 * Tn * 4))) return rc;
	f.tasks = c->d_tasks.as<int2>(); f.alns = c->d_alns.as<DevAln>(); f.redo_list = c->d_fredo.as<int>();
	f.fast_list = c->d_task_lists.as<int>(); f.dp_list = f.fast_list + Tn; f.list_n = (int*)(pool_head + 15);
	if ((rc = launch_task_fill(f, c->stream))) return rc;
	int n_list[2] = { 0, 0 };
	HIP_TRY(hipMemcpyAsync(n_list, f.list_n, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	size_t want_pool = std::max(c->pool_cap, Tn * 64 + Tn * 32 + (size_t)(16 << 20));   // 64-byte slot per task + a shared tail for long texts
	for (int attempt = 0;; ++attempt) {
		if ((rc = c->d_pool.ensure(want_pool))) return rc;
		c->pool_cap = want_pool;
		f.pool = c->d_pool.as<uint8_t>(); f.pool_cap = want_pool;
		HIP_TRY(hipMemsetAsync(c->d_fmisc.p, 0, 120, c->stream));   // pool head, redo count, error; the task-list lengths at +120 stay
		{ const unsigned long long head0 = (unsigned long long)Tn * 64; HIP_TRY(hipMemcpyAsync(c->d_fmisc.p, &head0, 8, hipMemcpyHostToDevice, c->stream)); }   // the shared tail starts behind the slots
		if (n_list[1] > 0) { if ((rc = c->d_zslab.ensure(cigar_zslab_bytes(c->in->max_len, n_list[1])))) return rc; f.zslab = c->d_zslab.as<unsigned>(); }
		if ((rc = launch_cigar(f, n_list[0], n_list[1], c->in->max_len, c->stream, c->stream2, c->ev_fork, c->ev_join))) return rc;
		int h[6] = { 0 };
		HIP_TRY(hipMemcpyAsync(h, c->d_fmisc.p, 24, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		int n_redo = h[2], err = h[4];
		if (err == 5 && attempt < 6) { want_pool *= 4; continue; }     // text pool exhausted: larger pool, run the stage again (GPU only)
		if (!err && n_redo > 0) {                                       // tasks beyond the LDS variant: global-slab variant
			const int grid = std::min(n_redo, 256);                   // one 5.7 MB slab per workgroup
			if ((rc = c->d_bigz.ensure((size_t)grid * cigar_big_slab_bytes()))) return rc;
			f.big_z = c->d_bigz.as<uint8_t>();
			if ((rc = launch_cigar_big(f, grid, c->stream))) return rc;
			HIP_TRY(hipMemcpyAsync(h, c->d_fmisc.p, 24, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
			err = h[4];
			if (err == 5 && attempt < 6) { want_pool *= 4; continue; }
		}
		if (err) {
			fprintf(stderr, "[bwahip] alignment kernel reported code %d (read %d of the batch)%s\n", err, h[5], err == 6 ? ": a region's reference span / band exceeds the compiled limits" : "");
			return err == 6 ? BWAHIP_ECAPACITY : BWAHIP_EINTERNAL;
		}
		break;
	}
	if (timed) HIP_TRY(hipEventRecord(c->ev[17], c->stream));
	if ((rc = launch_out(f, false, 0, -1))) return rc;
	if ((rc = launch_scan(c->d_sam_len.as<int>(), o.d_sam_off.as<int64_t>(), n, c->d_scan, c->stream))) return rc;
	if (timed) HIP_TRY(hipEventRecord(c->ev[18], c->stream));
	int64_t total = 0;
	HIP_TRY(hipMemcpyAsync(&total, o.d_sam_off.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	o.total = total; if (bgzf) o.n_blocks = bgzf_blocks(total);
	if ((rc = o.d_sam.ensure((size_t)total + (bgzf ? (size_t)bgzf_blocks(total) * 31 : 0) + 64))) return rc;   // bgzf: the bound bgzf_deflate asks for
	f.sam = o.d_sam.as<uint8_t>();
	if (sorted || bgzf) { if ((rc = c->bs.raw.ensure((size_t)total + 64))) return rc; f.sam = c->bs.raw.as<uint8_t>(); }
	if (host_sam_off) {                                         // bwahip_process_seqs: the offsets travel ahead of the write pass
		c->h_sam_off.resize((size_t)n + 1);
		HIP_TRY(hipMemcpyAsync(c->h_sam_off.data(), o.d_sam_off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
	}
	// the write pass in two halves (cut at an even read: mates stay together) with an event between them: a caller that downloads the text
	// (bwahip_process_seqs) starts on the first half while the second is being written
	c->sam_half_reads = (n / 2) & ~1;
	if ((rc = launch_out(f, true, 0, c->sam_half_reads))) return rc;
	HIP_TRY(hipEventRecord(c->ev_sam_half, c->stream));
	if ((rc = launch_out(f, true, c->sam_half_reads, n))) return rc;
	if (timed) HIP_TRY(hipEventRecord(c->ev[19], c->stream));
	if (sorted && (rc = bam_sort_batch(c, n, total, form == OutForm::BamSortedDup ? (pe ? 2 : 1) : 0))) return rc;
	if (bgzf) {                                                   // the deflate stage, queued behind the write pass
		for (auto &e : o.ev_bgzf) if (!e && (rc = e.make())) return rc;
		if ((rc = o.d_tot.ensure(16))) return rc;
		HIP_TRY(hipEventRecord(o.ev_bgzf[0], c->stream));
		if ((rc = bgzf_deflate(c, c->bs.raw.as<uint8_t>(), total, o.d_sam, o.d_tot.as<int64_t>(), c->stream))) return rc;
		HIP_TRY(hipEventRecord(o.ev_bgzf[1], c->stream));
	}
	if (timed) {
		HIP_TRY(hipStreamSynchronize(c->stream));
		if (sorted) for (int k = 0; k < 3; ++k) HIP_TRY(hipEventElapsedTime(&c->bs.ms[k], o.ev_sort[k], o.ev_sort[k + 1]));
		HIP_TRY(hipEventElapsedTime(&c->final_ms[0], c->ev[15], c->ev[16]));
		HIP_TRY(hipEventElapsedTime(&c->final_ms[1], c->ev[16], c->ev[17]));
		HIP_TRY(hipEventElapsedTime(&c->final_ms[2], c->ev[17], c->ev[18]));
		HIP_TRY(hipEventElapsedTime(&c->final_ms[3], c->ev[18], c->ev[19]));
		HIP_TRY(hipEventElapsedTime(&c->final_ms[4], c->ev[20], c->ev[15]));   // paired-end: insert sizes + mate rescue
	}
	return 0;
}

#define NT4_TABLE \
	4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4,  4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4, \
	4,4,4,4, 4,4,4,4, 4,4,4,4, 4,5,4,4,  4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4, \
	4,0,4,1, 4,4,4,2, 4,4,4,4, 4,4,4,4,  4,4,4,4, 3,4,4,4, 4,4,4,4, 4,4,4,4, \
	4,0,4,1, 4,4,4,2, 4,4,4,4, 4,4,4,4,  4,4,4,4, 3,4,4,4, 4,4,4,4, 4,4,4,4, \
	4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4,  4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4, \
	4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4,  4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4, \
	4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4,  4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4, \
	4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4,  4,4,4,4, 4,4,4,4, 4,4,4,4, 4,4,4,4
static const uint8_t k_nt4[256] = { NT4_TABLE };      // nst_nt4_table, bntseq.c:46
__constant__ uint8_t d_nt4[256] = { NT4_TABLE };

// bwamem.c:1067-1068 on the batch in HBM: seq[i] = seq[i] < 4 ? seq[i] : nst_nt4_table[seq[i]] (seq is char: bytes >= 128 compare
// below 4 and stay as they are, as in the reference), 16 bases per thread
__global__ __launch_bounds__(256) void k_nt4_conv(uint8_t *seq, int64_t n)
{
	const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
	if (i >= n) return;
	if (i + 16 <= n) {
		uint4 v = *reinterpret_cast<const uint4*>(seq + i);
		uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			uint32_t o = 0;
#pragma unroll
			for (int b = 0; b < 4; ++b) { const uint32_t c = w[k] >> (8 * b) & 0xff; o |= (uint32_t)(((int8_t)c < 4) ? c : d_nt4[c]) << (8 * b); }
			w[k] = o;
		}
		*reinterpret_cast<uint4*>(seq + i) = make_uint4(w[0], w[1], w[2], w[3]);
	} else for (int64_t k = i; k < n; ++k) { const uint8_t c = seq[k]; seq[k] = ((int8_t)c < 4) ? c : d_nt4[c]; }
}
int launch_nt4(uint8_t *seq, int64_t n, hipStream_t st)
{
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_nt4_conv, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, st, seq, n);
	return hipGetLastError() == hipSuccess ? 0 : BWAHIP_ENODEV;
}

// One batch of host reads on its way to HBM.  The base codes go first (converted in place exactly as bwamem.c:1067-1068 does)
// and the hot path starts on them at once; qualities, names and comments -- needed only when the SAM text is written -- are
// gathered and uploaded by a helper thread on the copy stream while the hot path runs.
static int stage_codes(bwahip_ctx *c, int nt, int n, bwahip_seq_t *seqs, BatchText &t)
{
	auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double t0 = now();
	t.off.resize(n + 1); t.qoff.resize(n); t.noff.resize(n + 1); t.coff.resize(n + 1);
	t.off[0] = t.noff[0] = t.coff[0] = 0;
	// offsets of bases / qualities / names / comments: per-chunk totals in parallel (two strlen per read), a serial scan over the
	// chunks, then the running sums inside every chunk in parallel
	const int C = n >= 4096 && nt > 1 ? nt : 1;
	struct Tot { int64_t seq = 0, qual = 0, name = 0, comm = 0; int bad = 0, any_comm = 0; char pad[24]; };
	std::vector<Tot> tot(C + 1);
	auto chunk = [&](int c) { return (int64_t)n * c / C; };
	auto for_chunks = [&](auto f) {
		if (C == 1) { f(0); return; }
		std::vector<std::thread> th;
		for (int c = 0; c < C; ++c) th.emplace_back(f, c);
		for (auto &x : th) x.join();
	};
	for_chunks([&](int c) {
		Tot x;
		for (int64_t i = chunk(c); i < chunk(c + 1); ++i) {
			if (seqs[i].l_seq < 0 || !seqs[i].name) { x.bad = 1; continue; }
			const int64_t ln = (int64_t)strlen(seqs[i].name) + 1, lc = seqs[i].comment ? (int64_t)strlen(seqs[i].comment) : 0;
			t.noff[i + 1] = ln; t.coff[i + 1] = lc ? lc + 1 : 0;
			x.seq += seqs[i].l_seq; x.qual += seqs[i].qual ? seqs[i].l_seq : 0; x.name += ln; x.comm += lc ? lc + 1 : 0; x.any_comm |= lc > 0;
		}
		tot[c + 1] = x;
	});
	for (int c = 1; c <= C; ++c) {
		if (tot[c].bad) return BWAHIP_EINVAL;
		t.any_comment |= tot[c].any_comm != 0;
		tot[c].seq += tot[c - 1].seq; tot[c].qual += tot[c - 1].qual; tot[c].name += tot[c - 1].name; tot[c].comm += tot[c - 1].comm;
	}
	t.qtot = tot[C].qual;
	for_chunks([&](int c) {
		int64_t so = tot[c].seq, qo = tot[c].qual, no = tot[c].name, co = tot[c].comm;
		for (int64_t i = chunk(c); i < chunk(c + 1); ++i) {
			so += seqs[i].l_seq; t.off[i + 1] = so;
			if (seqs[i].qual) { t.qoff[i] = qo; qo += seqs[i].l_seq; } else t.qoff[i] = -1;
			no += t.noff[i + 1]; t.noff[i + 1] = no;
			co += t.coff[i + 1]; t.coff[i + 1] = co;
		}
	});
	const double t1 = now();
	// one pinned staging buffer (kept by the context) holds codes | qualities | names | comments: the copies to HBM then run at
	// PCIe speed instead of through pageable memory
	t.sz_codes = ((size_t)t.off[n] + 64) & ~(size_t)63; t.sz_qual = ((size_t)t.qtot + 127) & ~(size_t)63; t.sz_names = ((size_t)t.noff[n] + 127) & ~(size_t)63;
	t.sz_comm = t.any_comment ? ((size_t)t.coff[n] + 127) & ~(size_t)63 : 0;
	int rc = c->in->h_stage.ensure(t.sz_codes + t.sz_qual + t.sz_names + t.sz_comm);
	if (rc) return rc;
	// device buffers of the text are sized here, on the calling thread, so that the helper only copies
	if ((rc = c->in->d_qual.ensure(t.sz_qual)) || (rc = c->in->d_qual_off.ensure((size_t)n * 8 + 16)) || (rc = c->in->d_names.ensure(t.sz_names)) ||
	    (rc = c->in->d_name_off.ensure((size_t)(n + 1) * 8)) || (rc = c->in->d_comment_off.ensure((size_t)(n + 1) * 8))) return rc;
	c->in->any_comment = t.any_comment;
	if (t.any_comment && (rc = c->in->d_comments.ensure(t.sz_comm))) return rc;
	// the bases travel as the caller wrote them (ASCII or codes) and are turned into codes in HBM (k_nt4: the same table look-up as
	// bwamem.c:1067-1068); the caller's own arrays are converted in place by the helper thread while the hot path runs
	const double t2 = now();
	uint8_t *codes = (uint8_t*)c->in->h_stage.p;
	par_for_chunks(n, nt, [&](int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) memcpy(codes + t.off[i], seqs[i].seq, (size_t)seqs[i].l_seq); });
	const double t3 = now();
	if ((rc = bwahip_batch_upload(c, n, codes, t.off.data()))) return rc;
	if (c->knobs.e2e_log) fprintf(stderr, "[bwahip] stage_codes: offsets %.1f ms, buffers %.1f ms, gather %.1f ms, upload %.1f ms\n", (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (now() - t3) * 1e3);
	return launch_nt4(c->in->d_seq.as<uint8_t>(), c->in->total_bases, c->stream);
}

// helper thread: the text of the batch into the pinned buffer and on to HBM (copy stream); returns when the copies are done
static int stage_text(bwahip_ctx *c, int nt, int n, bwahip_seq_t *seqs, const BatchText &t)
{
	HIP_TRY(hipSetDevice(c->device));
	uint8_t *qual = (uint8_t*)c->in->h_stage.p + t.sz_codes, *names = qual + t.sz_qual, *comments = names + t.sz_names;
	memset(qual + (size_t)t.qtot, 0, t.sz_qual - (size_t)t.qtot); memset(names + (size_t)t.noff[n], 0, t.sz_names - (size_t)t.noff[n]);
	if (t.any_comment) memset(comments + (size_t)t.coff[n], 0, t.sz_comm - (size_t)t.coff[n]);
	par_for_chunks(n, nt, [&](int64_t b, int64_t e) {
		for (int64_t i = b; i < e; ++i) {
			char *s = seqs[i].seq;                                  // bwamem.c:1067-1068, in place (the reference's contract)
			for (int k = 0; k < seqs[i].l_seq; ++k) s[k] = s[k] < 4 ? s[k] : (char)k_nt4[(uint8_t)s[k]];
			if (t.qoff[i] >= 0) memcpy(&qual[t.qoff[i]], seqs[i].qual, seqs[i].l_seq);
			memcpy(&names[t.noff[i]], seqs[i].name, t.noff[i + 1] - t.noff[i]);
			if (t.any_comment && t.coff[i + 1] > t.coff[i]) memcpy(&comments[t.coff[i]], seqs[i].comment, t.coff[i + 1] - t.coff[i]);
		}
	});
	hipStream_t st = c->stream_copy;
	HIP_TRY(hipMemcpyAsync(c->in->d_qual.p, qual, t.sz_qual, hipMemcpyHostToDevice, st));
	if (n) HIP_TRY(hipMemcpyAsync(c->in->d_qual_off.p, t.qoff.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(c->in->d_names.p, names, t.sz_names, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(c->in->d_name_off.p, t.noff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(c->in->d_comment_off.p, t.coff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
	if (t.any_comment) HIP_TRY(hipMemcpyAsync(c->in->d_comments.p, comments, t.sz_comm, hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

// What a bwahip_process_seqs* entry wants back: the batch in `form`; text != nullptr: in one piece (in the context's pinned buffer) instead
// of being cut into per-read strings, with the pointers the form fills beside it
struct SeqsOut {
	OutForm form = OutForm::Sam;
	const char **text = nullptr; int64_t *len = nullptr; const int64_t **off = nullptr;   // off: the reads' offsets (optional; SAM text, BAM records)
	const uint64_t **keys = nullptr; const int64_t **rec_off = nullptr; int64_t *n_rec = nullptr;   // BamSorted
	int64_t *raw_len = nullptr, *n_blocks = nullptr;                                        // Bgzf
	const uint32_t **tmpl = nullptr; const bwahip_dup_desc_t **desc = nullptr; int64_t *n_tmpl = nullptr;   // BamSortedDup
};

// The end of the one-piece forms that do not leave in read order: `bytes` of d_sam into the pinned buffer whose turn it is (valid until the
// next-but-one call), beside what `more` queues on the context's stream for the buffers of the same turn; both streams awaited, no per-read strings
template <class More>
static int download_piece(bwahip_ctx *ctx, int64_t bytes, int n, bwahip_seq_t *seqs, int nt, const SeqsOut &out, More more)
{
	PinnedOut &pin = ctx->pin[ctx->turn ^= 1];
	HostBuf &hb = pin.h_sam;
	int rc;
	if ((rc = hb.ensure((size_t)bytes + 1)) || (rc = more(pin))) return rc;
	if (bytes) HIP_TRY(hipMemcpyAsync(hb.p, ctx->out->d_sam.p, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream_copy));
	par_for_chunks(n, nt, [&](int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) seqs[i].sam = nullptr; });
	*out.text = (const char*)hb.p; *out.len = bytes;
	return 0;
}

static int process_seqs_impl(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0, const SeqsOut &out)
{
	static const int64_t no_records[1] = { 0 };
	const bool sorted = is_sorted(out.form), bz = out.form == OutForm::Bgzf, dup = out.form == OutForm::BamSortedDup;
	if (sorted) { *out.keys = nullptr; *out.rec_off = no_records; *out.n_rec = 0; }
	if (dup) { *out.tmpl = nullptr; *out.desc = nullptr; *out.n_tmpl = 0; }
	if (!ctx || !opt || n < 0 || (n && !seqs)) return BWAHIP_EINVAL;
	const bool pe = (opt->flag & BWAHIP_F_PE) != 0;
	if (pe && (n & 1)) return BWAHIP_EINVAL;
	if (out.text) { *out.text = ""; *out.len = 0; if (out.off) *out.off = nullptr; }
	if (!ctx->knobs.gpu_final || (pe && !ctx->knobs.gpu_pair)) {
		if (out.text) return BWAHIP_EINVAL;                       // the one-piece output exists on the GPU path only
		host_final_fn hf = load_host_final();
		return hf ? hf(ctx, opt, n_processed, n, seqs, pes0) : BWAHIP_EINVAL;
	}
	if (pe) for (int i = 0; i < n; i += 2) if (strcmp(seqs[i].name, seqs[i + 1].name) != 0) { fprintf(stderr, "[bwahip] paired reads have different names\n"); return BWAHIP_EINVAL; }   // err_fatal in the reference (bwamem_pair.c:386)
	if (n == 0) return 0;
	if (is_bam(out.form)) { const int rc_bam = bam_check_reads(n, seqs); if (rc_bam) return rc_bam; }   // what BAM cannot hold is refused before any launch
	HIP_TRY(hipSetDevice(ctx->device));
	const bool verbose = ctx->knobs.verbose != 0;
	auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double t0 = now();
	const int nt = opt->n_threads > 1 ? opt->n_threads : 1;
	BatchText &bt = ctx->batch_text;                             // kept by the context: no fresh page faults per batch
	bt.qtot = 0; bt.any_comment = false;
	int rc = stage_codes(ctx, nt, n, seqs, bt);
	if (rc) return rc;
	const double t1 = now();
	// the text travels while the hot path runs (half of the host threads: the other half of the machine belongs to the caller's reader)
	int rc_text = 0;
	std::thread text_thread([&] { rc_text = stage_text(ctx, nt > 2 ? nt / 2 : 1, n, seqs, bt); });
	rc = run_pipeline(ctx, opt, false, false);
	text_thread.join();
	if (rc || (rc = rc_text)) return rc;
	const double t2 = now();
	if ((rc = run_final(ctx, opt, n_processed, pes0, false, out.form, true))) return rc;
	if (bz) {                                                     // the members in one piece: their total was left in HBM by the deflate stage
		int64_t tot[2] = { 0, 0 };
		HIP_TRY(hipMemcpyAsync(tot, ctx->out->d_tot.p, 16, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		if ((rc = download_piece(ctx, tot[0], n, seqs, nt, out, [](PinnedOut&) { return 0; }))) return rc;
		*out.raw_len = ctx->out->total; *out.n_blocks = ctx->out->n_blocks;
		return 0;
	}
	if (sorted) {                                                 // records, keys and offsets in one piece each
		const int64_t nr = ctx->out->n_rec;
		rc = download_piece(ctx, ctx->out->total, n, seqs, nt, out, [&](PinnedOut &pin) -> int {
			int r;
			if ((r = pin.h_keys.ensure((size_t)(nr ? nr : 1) * 8)) || (r = pin.h_rec_off.ensure((size_t)(nr + 1) * 8))) return r;
			if (nr) HIP_TRY(hipMemcpyAsync(pin.h_keys.p, ctx->out->d_keys.p, (size_t)nr * 8, hipMemcpyDeviceToHost, ctx->stream));
			HIP_TRY(hipMemcpyAsync(pin.h_rec_off.p, ctx->out->d_rec_off.p, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
			if (dup) {
				const int64_t nt_ = ctx->out->n_tmpl;
				if ((r = pin.h_tmpl.ensure((size_t)(nr ? nr : 1) * 4)) || (r = pin.h_desc.ensure((size_t)(nt_ ? nt_ : 1) * sizeof(bwahip_dup_desc_t)))) return r;
				if (nr) HIP_TRY(hipMemcpyAsync(pin.h_tmpl.p, ctx->out->d_tmpl.p, (size_t)nr * 4, hipMemcpyDeviceToHost, ctx->stream));
				if (nt_) HIP_TRY(hipMemcpyAsync(pin.h_desc.p, ctx->out->d_desc.p, (size_t)nt_ * sizeof(bwahip_dup_desc_t), hipMemcpyDeviceToHost, ctx->stream));
			}
			return 0;
		});
		if (rc) return rc;
		if (dup) { *out.tmpl = (const uint32_t*)ctx->pin[ctx->turn].h_tmpl.p; *out.desc = (const bwahip_dup_desc_t*)ctx->pin[ctx->turn].h_desc.p; *out.n_tmpl = ctx->out->n_tmpl; }
		*out.keys = (const uint64_t*)ctx->pin[ctx->turn].h_keys.p; *out.rec_off = (const int64_t*)ctx->pin[ctx->turn].h_rec_off.p; *out.n_rec = nr;
		return 0;
	}
	// SAM text back through the pinned buffer.  run_final wrote it in two halves and sent the offsets ahead: once the first half is written
	// (ev_sam_half) its download starts on the copy stream, beside the kernel that writes the second half.  Per-read strings: in slices of reads --
	// while slice k+1 travels, the host threads cut slice k into one malloc()ed string per read, which is what the reference's contract wants
	// (bwamem.c:1054).  (The context's streams are non-blocking: a plain hipMemcpy would not wait for the SAM kernels.)
	std::vector<int64_t> &soff = ctx->h_sam_off;
	HostBuf &hs = ctx->pin[out.text ? (ctx->turn ^= 1) : 0].h_sam;   // one-piece callers: the text stays valid until the next-but-one call
	if ((rc = hs.ensure((size_t)ctx->out->total + 1))) return rc;
	char *text = (char*)hs.p;
	HIP_TRY(hipEventSynchronize(ctx->ev_sam_half));               // first half written; the offsets arrived before that
	const int half = ctx->sam_half_reads;
	constexpr int SLICES = 8;
	int64_t sl_beg[SLICES + 1];
	for (int k = 0; k <= SLICES / 2; ++k) sl_beg[k] = (int64_t)half * k / (SLICES / 2);
	for (int k = 0; k <= SLICES / 2; ++k) sl_beg[SLICES / 2 + k] = half + (int64_t)(n - half) * k / (SLICES / 2);
	auto copy_slice = [&](int k, hipStream_t st) -> int {
		const int64_t b = soff[sl_beg[k]], e = soff[sl_beg[k + 1]];
		if (e > b) HIP_TRY(hipMemcpyAsync(text + b, (const char*)ctx->out->d_sam.p + b, (size_t)(e - b), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipEventRecord(ctx->ev_slice[k], st));
		return 0;
	};
	for (int k = 0; k < SLICES / 2; ++k) if ((rc = copy_slice(k, ctx->stream_copy))) return rc;
	for (int k = SLICES / 2; k < SLICES; ++k) if ((rc = copy_slice(k, ctx->stream))) return rc;
	const int n_sl = SLICES;
	if (out.text) {                                               // one piece: no per-read strings
		HIP_TRY(hipStreamSynchronize(ctx->stream_copy));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		const double t4 = now();
		text[ctx->out->total] = 0;
		*out.text = text; *out.len = ctx->out->total; if (out.off) *out.off = soff.data();
		par_for_chunks(n, nt, [&](int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) seqs[i].sam = nullptr; });
		if (verbose || ctx->knobs.e2e_log)
			fprintf(stderr, "[bwahip] process_seqs_text %d reads: codes gather+upload %.1f ms, hot path (text upload beside it) %.1f ms, finalisation+SAM on GPU and download %.1f ms (%lld bytes), rest %.1f ms\n",
			        n, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t2) * 1e3, (long long)ctx->out->total, (now() - t4) * 1e3);
		return 0;
	}
	const double t3 = now();
	std::atomic<int> oom(0), hip_bad(0);
	auto cut = [&](int tid, int nthr) {
		(void)hipSetDevice(ctx->device);
		for (int k = 0; k < n_sl; ++k) {
			if (hipEventSynchronize(ctx->ev_slice[k]) != hipSuccess) { hip_bad = 1; return; }
			const int64_t cnt = sl_beg[k + 1] - sl_beg[k], per = (cnt + nthr - 1) / nthr;
			const int64_t b = sl_beg[k] + tid * per, e = b + per < sl_beg[k + 1] ? b + per : sl_beg[k + 1];
			for (int64_t i = b; i < e; ++i) {
				const size_t len = (size_t)(soff[i + 1] - soff[i]);
				char *p = (char*)malloc(len + 1);
				if (!p) { oom = 1; seqs[i].sam = nullptr; continue; }
				memcpy(p, text + soff[i], len); p[len] = 0;
				seqs[i].sam = p;
			}
		}
	};
	if (nt == 1) cut(0, 1);
	else { std::vector<std::thread> th; for (int t = 0; t < nt; ++t) th.emplace_back(cut, t, nt); for (auto &x : th) x.join(); }
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if (verbose || ctx->knobs.e2e_log)
		fprintf(stderr, "[bwahip] process_seqs %d reads: codes gather+upload %.1f ms, hot path (text upload beside it) %.1f ms, finalisation+SAM on GPU %.1f ms (%lld bytes), download + per-read strings %.1f ms\n",
		        n, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (long long)ctx->out->total, (now() - t3) * 1e3);
	if (hip_bad) return BWAHIP_ENODEV;
	return oom ? BWAHIP_ENOMEM : 0;
}

extern "C" int bwahip_process_seqs(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0)
{
	return process_seqs_impl(ctx, opt, n_processed, n, seqs, pes0, SeqsOut());
}

// The same work with the batch's SAM handed over in one piece -- for a caller whose output step is one fwrite (fastmap.c prints
// seqs[i].sam read by read): no malloc per read, no second copy.  *sam: NUL-terminated text of the whole batch in read order, *off
// (optional): n + 1 offsets, read i's records are sam[off[i] .. off[i+1]).  Both live in the context and stay valid until its next call.
extern "C" int bwahip_process_seqs_text(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0,
                                        const char **sam, int64_t *sam_len, const int64_t **off)
{
	if (!sam || !sam_len) return BWAHIP_EINVAL;
	return process_seqs_impl(ctx, opt, n_processed, n, seqs, pes0, { OutForm::Sam, sam, sam_len, off });
}

// The same work with the batch as BAM records (k_bam.hip): *bam = the records of all reads in read order, concatenated, without header
// and uncompressed (bwahip_bam_header / bwahip_bgzf_write make a file of them); the buffers and their lifetime as for the text.
extern "C" int bwahip_process_seqs_bam(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0,
                                       const uint8_t **bam, int64_t *bam_len, const int64_t **off)
{
	if (!bam || !bam_len) return BWAHIP_EINVAL;
	return process_seqs_impl(ctx, opt, n_processed, n, seqs, pes0, { OutForm::Bam, (const char**)bam, bam_len, off });
}

// The same records in coordinate order (k_bamsort.hip; the key and the order are in include/bwahip.h), with what a merge of several
// batches needs: the sorted keys and the records' offsets.  Buffers and lifetimes as above.
extern "C" int bwahip_process_seqs_bam_sorted(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0,
                                              const uint8_t **bam, int64_t *bam_len, const uint64_t **keys, const int64_t **rec_off, int64_t *n_rec)
{
	if (!bam || !bam_len || !keys || !rec_off || !n_rec) return BWAHIP_EINVAL;
	return process_seqs_impl(ctx, opt, n_processed, n, seqs, pes0, { OutForm::BamSorted, (const char**)bam, bam_len, nullptr, keys, rec_off, n_rec });
}

// bwahip_process_seqs_bam_sorted with what duplicate marking in a device merger needs (k_markdup.hip): per record the index of its template,
// per template its descriptor
extern "C" int bwahip_process_seqs_bam_sorted_dup(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0,
                                                  const uint8_t **bam, int64_t *bam_len, const uint64_t **keys, const int64_t **rec_off, int64_t *n_rec,
                                                  const uint32_t **tmpl, const bwahip_dup_desc_t **desc, int64_t *n_tmpl)
{
	if (!bam || !bam_len || !keys || !rec_off || !n_rec || !tmpl || !desc || !n_tmpl) return BWAHIP_EINVAL;
	SeqsOut so = { OutForm::BamSortedDup, (const char**)bam, bam_len, nullptr, keys, rec_off, n_rec };
	so.tmpl = tmpl; so.desc = desc; so.n_tmpl = n_tmpl;
	return process_seqs_impl(ctx, opt, n_processed, n, seqs, pes0, so);
}

// bwahip_process_seqs_bam with the records leaving the GPU as BGZF members (k_bgzf.hip): *bgzf = the members of the batch's records, cut
// every 65 280 bytes, concatenated -- no file header, no end-of-file block; *raw_len = the bytes of the records, *n_blocks = members.
extern "C" int bwahip_process_seqs_bgzf(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0,
                                        const uint8_t **bgzf, int64_t *bgzf_len, int64_t *raw_len, int64_t *n_blocks)
{
	if (!bgzf || !bgzf_len || !raw_len || !n_blocks) return BWAHIP_EINVAL;
	*raw_len = 0; *n_blocks = 0;
	return process_seqs_impl(ctx, opt, n_processed, n, seqs, pes0, { OutForm::Bgzf, (const char**)bgzf, bgzf_len, nullptr, nullptr, nullptr, nullptr, raw_len, n_blocks });
}

// Insert-size statistics (mem_pestat_t x 4: FF, FR, RF, RR) and mate-rescue counters ([0] Smith-Waterman alignments run on
// the GPU, [1] regions they added, [2] most alignments of one pair, [3] pairs that needed any) of the last paired-end batch
// finalised on the GPU.
extern "C" int bwahip_last_pe_stats(bwahip_ctx *ctx, bwahip_pestat_t *pes4, uint64_t *counters2)
{
	if (!ctx) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if (pes4) memcpy(pes4, ctx->last_pes, sizeof ctx->last_pes);
	if (counters2) for (int i = 0; i < 4; ++i) counters2[i] = ctx->last_pe_counters[i];
	if (getenv("BWAHIP_PE_LOG")) {
		const unsigned long long *c = ctx->last_pe_counters;
		fprintf(stderr, "[bwahip] mate rescue: %llu alignments run ahead by k_matesw_sw; mem_matesw used %llu (%llu more inside k_matesw), %llu regions added, %llu pairs; k_matesw summed over its wavefronts: window fetch %.1f ms, alignments %.1f ms, list clean-up %.1f ms; longest pair %.2f ms\n",
		        ctx->last_sw_tasks, c[0], c[8], c[1], c[3], c[4] / 1e5, c[5] / 1e5, c[6] / 1e5, c[7] / 1e5);
	}
	return 0;
}

// Which paths the paired-end kernels of the last batch took: out[0..n) of
//   [0] alignments run ahead of the sequential pass by the byte kernel (k_matesw_sw), [1] by the word kernel (k_matesw_sw8),
//   [2] alignments run inside k_matesw with the reference window in LDS, [3] with the window in the global slab,
//   [4] rescued regions placed by incr_insert, [5] calls of the general sort_dedup_nopatch,
//   [6] pairs taken by the BIG instantiations of k_matesw, [7] pairs copied by k_pe_copy_big,
//   [8..11] alignments attempted per orientation FF, FR, RF, RR, [12] windows rejected because their middle lies in another contig than the
//   anchor, [13] pairs with one end rescued by a <16> and the other by an <8> instantiation of k_matesw.
extern "C" int bwahip_last_pe_paths(bwahip_ctx *ctx, uint64_t *out, int n)
{
	if (!ctx || !out || n < 0) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	for (int i = 0; i < n; ++i) out[i] = i < 2 ? ctx->last_sw_ahead[i] : i < 2 + PE_PATH_N ? ctx->last_pe_counters[bwahip_ctx::PE_CNT_PATHS + i - 2] : 0;
	return 0;
}

// Stage dump of the paired-end path (the counterpart of bwahip_run_stages): upload, run_pipeline, then run_final's paired-end part up to and
// including both k_pair passes.  Records as bwahip_run_stages writes them: BWAHIP_STAGE_PESTAT once in front, then per read the header
// (tag 100) and the stages asked for.
extern "C" int bwahip_run_pe_stages(bwahip_ctx *c, const bwahip_opt_t *opt_in, int64_t n_processed, int n, const uint8_t *seq, const int64_t *off,
                                    const bwahip_pestat_t *pes0, int stage_mask, int64_t **out, int64_t *out_len)
{
	if (!c || !opt_in || !out || !out_len || n < 0 || (n & 1)) return BWAHIP_EINVAL;
	bwahip_opt_t opt = *opt_in;
	opt.flag |= BWAHIP_F_PE;
	int rc = bwahip_batch_upload(c, n, seq, off);
	if (rc) return rc;
	std::vector<int64_t> o, v;
	if (n) {
		if ((rc = run_pipeline(c, &opt, false, false))) return rc;
		if ((rc = run_final(c, &opt, n_processed, pes0, false, OutForm::Sam, false, true))) return rc;
	} else memset(c->last_pes, 0, sizeof c->last_pes);
	for (int d = 0; d < 4; ++d) {
		const bwahip_pestat_t &p = c->last_pes[d];
		int64_t a, s;
		memcpy(&a, &p.avg, 8); memcpy(&s, &p.std, 8);
		v.push_back(p.low); v.push_back(p.high); v.push_back(p.failed); v.push_back(a); v.push_back(s);
	}
	if (stage_mask & (1 << BWAHIP_STAGE_PESTAT)) stage_rec(o, BWAHIP_STAGE_PESTAT, v);
	if (n) {
		const size_t R1 = (size_t)c->total_regs;
		std::vector<int> n0(n), n1(n), dbg((size_t)(n / 2) * 3);
		std::vector<int64_t> b0(n + 1), b1(n + 1);
		std::vector<PeRead> pr(n);
		HIP_TRY(hipMemcpy(n0.data(), c->d_reg_n.p, (size_t)n * 4, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(b0.data(), c->d_reg_base.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(n1.data(), c->d_pe_n.p, (size_t)n * 4, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(b1.data(), c->d_pe_base.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(pr.data(), c->d_pe_read.p, (size_t)n * sizeof(PeRead), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(dbg.data(), c->d_pair_dbg.p, dbg.size() * 4, hipMemcpyDeviceToHost));
		std::vector<DevReg> r0((size_t)b0[n] + 1), r1(R1 + 1);
		if (b0[n]) HIP_TRY(hipMemcpy(r0.data(), c->d_regs.p, (size_t)b0[n] * sizeof(DevReg), hipMemcpyDeviceToHost));
		if (R1) HIP_TRY(hipMemcpy(r1.data(), c->d_pe_regs.p, R1 * sizeof(DevReg), hipMemcpyDeviceToHost));
		for (int i = 0; i < n; ++i) {
			v = { (int64_t)i, off[i + 1] - off[i] };
			stage_rec(o, 100, v);
			if (stage_mask & (1 << BWAHIP_STAGE_REGS)) { v.clear(); stage_put_regs(v, n0[i], &r0[b0[i]]); stage_rec(o, BWAHIP_STAGE_REGS, v); }
			if (stage_mask & (1 << BWAHIP_STAGE_REGS_PE)) { v.clear(); stage_put_regs(v, n1[i], &r1[b1[i]]); stage_rec(o, BWAHIP_STAGE_REGS_PE, v); }
			if (stage_mask & (1 << BWAHIP_STAGE_PAIR)) {
				const PeRead &q = pr[i];
				const int *g = &dbg[(size_t)(i >> 1) * 3];
				v = { q.mode, q.h_reg, q.alt_reg, q.mapq, q.extra_flag, g[0], g[1], g[2] };
				stage_rec(o, BWAHIP_STAGE_PAIR, v);
			}
		}
	}
	*out_len = (int64_t)o.size();
	*out = (int64_t*)malloc(o.size() * 8 + 8);
	if (!*out) return BWAHIP_ENOMEM;
	memcpy(*out, o.data(), o.size() * 8);
	return 0;
}

// The part bwahip_kat_mark and bwahip_kat_pair share: caller region lists checked, turned into DevReg and uploaded with exactly n slots per
// read -- into k_extend's list buffers (pe_lists false) or into the paired-end list buffers mate rescue leaves (true) --, the marking buffers
// and the launch record made by mark_prepare, and k_mark launched as run_final launches it: once, or with `pairs` twice (every pair but the
// listed ones, then the listed ones; the pair list and its flags stay in d_resc / d_resc_flag for launch_pair).
struct KatLists {
	std::vector<DevReg> regs; std::vector<int> regn; std::vector<uint8_t> flag; std::vector<int> list;
	int64_t total = 0;
};
static int kat_lists_check(const bwahip_ctx *c, int n, const int64_t *reg_off, const int64_t *reg_words, const int32_t *pairs, int n_pairs, KatLists &L)
{
	if (!reg_off || reg_off[0] != 0) return BWAHIP_EINVAL;
	for (int i = 0; i < n; ++i) if (reg_off[i + 1] < reg_off[i] || reg_off[i + 1] - reg_off[i] > (1 << 24)) return BWAHIP_EINVAL;
	const int64_t total = L.total = reg_off[n];
	if (total > (1 << 26) || (total && !reg_words) || (n_pairs && !pairs)) return BWAHIP_EINVAL;
	L.regs.assign((size_t)total + 1, DevReg());
	L.regn.resize(n);
	for (int i = 0; i < n; ++i) L.regn[i] = (int)(reg_off[i + 1] - reg_off[i]);
	for (int64_t k = 0; k < total; ++k) {
		const int64_t *w = reg_words + 19 * k;
		if (w[3] < w[2] || w[1] < w[0] || w[4] < 0 || w[4] >= c->ix.n_seqs) return BWAHIP_EINVAL;
		DevReg r; memset(&r, 0, sizeof r);
		r.rb = w[0]; r.re = w[1]; r.qb = (int)w[2]; r.qe = (int)w[3]; r.rid = (int)w[4]; r.score = (int)w[5]; r.truesc = (int)w[6]; r.sub = (int)w[7]; r.csub = (int)w[9];
		r.sub_n = (int)w[10]; r.w = (int)w[11]; r.seedcov = (int)w[12]; r.seedlen0 = (int)w[15]; r.n_comp = (int)w[16]; r.is_alt = (int)w[17];
		const uint32_t u = (uint32_t)w[18]; memcpy(&r.frac_rep, &u, 4);
		L.regs[(size_t)k] = r;
	}
	L.flag.assign((size_t)(n / 2 + 4), 0);
	L.list.assign(pairs ? (size_t)n_pairs + 1 : 1, 0);
	for (int k = 0; pairs && k < n_pairs; ++k) {
		if (pairs[k] < 0 || pairs[k] >= n / 2 || L.flag[pairs[k]]) return BWAHIP_EINVAL;    // (a pair named twice would be marked by two workgroups at once)
		L.flag[pairs[k]] = 1; L.list[k] = pairs[k];
	}
	return 0;
}
// queues on c->stream; sel0: the byte the selection's buffers start as (0xff where the launches must write them)
static int kat_upload_mark(bwahip_ctx *c, const bwahip_opt_t *opt, int n, int64_t n_processed, const int64_t *reg_off, const KatLists &L, bool pe_lists, bool plan, int sel0,
                           bool listed, int n_pairs, FinLaunch &f)
{
	int rc;
	const size_t R = (size_t)(L.total ? L.total : 1);
	c->total_regs = L.total;
	DevBuf &d_r = pe_lists ? c->d_pe_regs : c->d_regs, &d_b = pe_lists ? c->d_pe_base : c->d_reg_base, &d_n = pe_lists ? c->d_pe_n : c->d_reg_n;
	if ((rc = dev_upload(d_r, L.regs.data(), L.regs.size() * sizeof(DevReg), c->stream)) || (rc = dev_upload(d_b, reg_off, (size_t)(n + 1) * 8, c->stream)) ||
	    (rc = dev_upload(d_n, L.regn.data(), (size_t)n * 4, c->stream)) || (rc = mark_prepare(c, opt, n, n_processed, pe_lists, f))) return rc;
	// what k_mark<false> leaves alone comes back as zero; what a launch must write starts as 0xff, so that nothing a call before this one
	// left in the context's buffers can pass for an answer
	if (hipMemsetAsync(c->d_fregs.p, 0xff, R * sizeof(FinReg), c->stream) != hipSuccess || hipMemsetAsync(c->d_freg_n.p, 0xff, (size_t)n * 4, c->stream) != hipSuccess ||
	    hipMemsetAsync(c->d_npri.p, 0xff, (size_t)n * 4, c->stream) != hipSuccess ||
	    hipMemsetAsync(c->d_need.p, sel0, R, c->stream) != hipSuccess || hipMemsetAsync(c->d_xa_owner.p, sel0, R * 4, c->stream) != hipSuccess ||
	    hipMemsetAsync(c->d_task_n.p, sel0, (size_t)n * 4, c->stream) != hipSuccess || hipMemsetAsync(c->d_rec_n.p, sel0, (size_t)n * 4, c->stream) != hipSuccess) return BWAHIP_ENODEV;
	if (listed) {                                                // as run_final does for a paired-end batch: all pairs but the listed ones, then the listed ones
		if ((rc = dev_upload(c->d_resc, L.list.data(), L.list.size() * 4, c->stream)) || (rc = dev_upload(c->d_resc_flag, L.flag.data(), L.flag.size(), c->stream))) return rc;
		f.resc_flag = c->d_resc_flag.as<uint8_t>(); f.resc_pairs = c->d_resc.as<int>(); f.subset = 1;
		if ((rc = launch_mark_primary(f, plan, 0, c->stream))) return rc;
		if (n_pairs > 0) {
			f.subset = 2;
			if ((rc = launch_mark_primary(f, plan, n_pairs, c->stream))) return rc;
		}
		f.subset = 0;
	} else if ((rc = launch_mark_primary(f, plan, 0, c->stream))) return rc;
	return 0;
}
// hash -> index in the input list of read `id` (k_mark gives region k of the input the hash of id + k: a bijection)
static inline uint64_t kat_hash_64(uint64_t key)                    // utils.h:97
{
	key += ~(key << 32); key ^= (key >> 22); key += ~(key << 13); key ^= (key >> 8);
	key += (key << 3); key ^= (key >> 15); key += ~(key << 27); key ^= (key >> 31);
	return key;
}

// Primary marking, -5, the selection and mapQ (k_mark, fin::select_records, fin::approx_mapq_se) on caller region lists; see bwahip.h.  The
// buffers and the launch record are run_final's (mark_prepare), the launches are launch_mark_primary as run_final calls it -- one launch, or
// with `pairs` the two of the paired-end path -- and only the region lists come from the caller.
extern "C" int bwahip_kat_mark(bwahip_ctx *c, const bwahip_opt_t *opt, int64_t n_processed, int n_reads, const int64_t *reg_off, const int64_t *reg_words,
                               int plan, const int32_t *pairs, int n_pairs, int64_t **out, int64_t *out_len)
{
	if (!c || !opt || n_reads < 0 || !out || !out_len || (plan != 0 && plan != 1) || n_pairs < 0 || n_processed < 0) return BWAHIP_EINVAL;
	*out = nullptr; *out_len = 0;
	if (n_reads == 0) return 0;
	const int n = n_reads;
	if (((opt->flag & BWAHIP_F_PE) || pairs) && (n & 1)) return BWAHIP_EINVAL;
	KatLists L;
	int rc;
	if ((rc = kat_lists_check(c, n, reg_off, reg_words, pairs, n_pairs, L))) return rc;
	const int64_t total = L.total;
	const std::vector<int> &regn = L.regn;
	HIP_TRY(hipSetDevice(c->device));
	const size_t R = (size_t)(total ? total : 1);
	std::vector<FinReg> h_f(R);
	std::vector<uint8_t> h_need(R);
	std::vector<int> h_own(R), h_mq(2 * R), h_fn(n), h_np(n), h_tn(n), h_rn(n);
	DevBuf d_mq;
	FinLaunch f;
	auto queue = [&]() -> int {                                  // the uploads, the launches, the copies back: the stream is awaited whatever this returns
		if ((rc = d_mq.ensure(R * 8)) || (rc = kat_upload_mark(c, opt, n, n_processed, reg_off, L, false, plan != 0, plan ? 0xff : 0, pairs != nullptr, n_pairs, f))) return rc;
		if ((rc = launch_kat_mapq(f, total, d_mq.as<int>(), c->stream))) return rc;
		if ((total && (hipMemcpyAsync(h_f.data(), c->d_fregs.p, (size_t)total * sizeof(FinReg), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		               hipMemcpyAsync(h_need.data(), c->d_need.p, (size_t)total, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		               hipMemcpyAsync(h_own.data(), c->d_xa_owner.p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		               hipMemcpyAsync(h_mq.data(), d_mq.p, (size_t)total * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess)) ||
		    hipMemcpyAsync(h_fn.data(), c->d_freg_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(h_np.data(), c->d_npri.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(h_tn.data(), c->d_task_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(h_rn.data(), c->d_rec_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return BWAHIP_ENODEV;
		return 0;
	};
	rc = queue();
	if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = BWAHIP_ENODEV;
	if (rc) return rc;
	auto hash_64 = kat_hash_64;
	std::vector<int64_t> o, v;
	std::vector<std::pair<uint64_t, int>> by_hash;
	for (int i = 0; i < n; ++i) {
		const int m = regn[i];
		if (h_fn[i] != m) return BWAHIP_EINTERNAL;
		const uint64_t id = (opt->flag & BWAHIP_F_PE) ? ((((uint64_t)n_processed >> 1) + (uint64_t)(i >> 1)) << 1 | (uint64_t)(i & 1)) : (uint64_t)n_processed + (uint64_t)i;
		by_hash.clear();
		for (int k = 0; k < m; ++k) by_hash.emplace_back(hash_64(id + (uint64_t)k), k);
		std::sort(by_hash.begin(), by_hash.end());
		v = { (int64_t)i, (int64_t)m };
		stage_rec(o, 100, v);
		v = { (int64_t)m, (int64_t)h_np[i], (int64_t)h_tn[i], (int64_t)h_rn[i] };
		for (int k = 0; k < m; ++k) {
			const size_t s = (size_t)reg_off[i] + k;
			const FinReg &p = h_f[s];
			uint32_t u; memcpy(&u, &p.frac_rep, 4);
			const auto it = std::lower_bound(by_hash.begin(), by_hash.end(), std::make_pair(p.hash, 0));
			const int64_t w[BWAHIP_KAT_MARK_WORDS] = { p.rb, p.re, p.qb, p.qe, p.rid, p.score, p.truesc, p.sub, p.alt_sc, p.csub, p.sub_n, p.w, p.seedcov, p.secondary, p.secondary_all,
			                                           p.seedlen0, p.n_comp, p.is_alt, (int64_t)u, (int64_t)p.hash, it != by_hash.end() && it->first == p.hash ? it->second : -1,
			                                           h_need[s], h_own[s], h_mq[2 * s], h_mq[2 * s + 1] };
			v.insert(v.end(), w, w + BWAHIP_KAT_MARK_WORDS);
		}
		stage_rec(o, BWAHIP_KAT_MARK_TAG, v);
	}
	*out = (int64_t*)malloc(o.size() * 8 + 8);
	if (!*out) return BWAHIP_ENOMEM;
	memcpy(*out, o.data(), o.size() * 8);
	*out_len = (int64_t)o.size();
	return 0;
}

// mem_pair and the decisions of mem_sam_pe (k_pair) on caller region lists; see bwahip.h.  The lists go into the paired-end list buffers,
// are marked as the paired-end path marks them (kat_upload_mark) and paired by launch_pair with the same subsets; the statistics, the penalty
// table (pair_stats) and the wiring of the launch record (pair_wire) are run_final's.
extern "C" int bwahip_kat_pair(bwahip_ctx *c, const bwahip_opt_t *opt0, int64_t n_processed, int n_reads, const int64_t *reg_off, const int64_t *reg_words,
                               const bwahip_pestat_t *pes, const int32_t *pairs, int n_pairs, int64_t **out, int64_t *out_len)
{
	if (!c || !opt0 || n_reads < 0 || !out || !out_len || n_pairs < 0 || n_processed < 0 || !pes) return BWAHIP_EINVAL;
	*out = nullptr; *out_len = 0;
	if (n_reads == 0) return 0;
	const int n = n_reads;
	if (n & 1) return BWAHIP_EINVAL;
	bwahip_opt_t opt = *opt0;
	opt.flag |= BWAHIP_F_PE;
	for (int d = 0; d < 4; ++d) if (!pes[d].failed && pes[d].high >= pes[d].low && (int64_t)pes[d].high - pes[d].low > (1 << 26)) return BWAHIP_EINVAL;
	KatLists L;
	int rc;
	if ((rc = kat_lists_check(c, n, reg_off, reg_words, pairs, n_pairs, L))) return rc;
	const int64_t total = L.total;
	HIP_TRY(hipSetDevice(c->device));
	const size_t R = (size_t)(total ? total : 1);
	std::vector<FinReg> h_f(R);
	std::vector<uint8_t> h_need(R);
	std::vector<int> h_own(R), h_fn(n), h_np(n), h_tn(n), h_rn(n), h_dbg((size_t)(n / 2) * 3);
	std::vector<PeRead> h_pr(n);
	FinLaunch f;
	PairLaunch pl;
	int err = 0;
	auto queue = [&]() -> int {                                  // the uploads, the launches, the copies back: the stream is awaited whatever this returns
		if (hipMemsetAsync(c->d_fmisc.p, 0, 256, c->stream) != hipSuccess) return BWAHIP_ENODEV;
		if ((rc = kat_upload_mark(c, &opt, n, n_processed, reg_off, L, true, false, 0xff, pairs != nullptr, n_pairs, f))) return rc;
		memset(&pl, 0, sizeof pl);
		pl.ix = c->ix; pl.opt = make_dev_opt(&opt); pl.n_reads = n; pl.n_processed = n_processed; pl.logtab = c->d_logtab.as<double>();
		pl.pe_base = c->d_pe_base.as<int64_t>(); pl.pe_regs = c->d_pe_regs.as<DevReg>(); pl.pe_n = c->d_pe_n.as<int>();
		pl.err = (int*)(c->d_fmisc.as<unsigned long long>() + 2);
		int64_t widest;
		if ((rc = pair_stats(c, pes, pl, widest)) || (rc = pair_wire(c, f, n, true, pl))) return rc;
		if (hipMemsetAsync(c->d_pe_read.p, 0xff, (size_t)n * sizeof(PeRead), c->stream) != hipSuccess) return BWAHIP_ENODEV;
		if (pairs) {
			pl.resc_flag = c->d_resc_flag.as<uint8_t>(); pl.resc_list = c->d_resc.as<int>(); pl.subset = 1;
			if ((rc = launch_pair(pl, 0, c->stream))) return rc;
			if (n_pairs > 0) {
				pl.subset = 2;
				if ((rc = launch_pair(pl, n_pairs, c->stream))) return rc;
			}
			pl.subset = 0;
		} else if ((rc = launch_pair(pl, 0, c->stream))) return rc;
		if ((total && (hipMemcpyAsync(h_f.data(), c->d_fregs.p, (size_t)total * sizeof(FinReg), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		               hipMemcpyAsync(h_need.data(), c->d_need.p, (size_t)total, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		               hipMemcpyAsync(h_own.data(), c->d_xa_owner.p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)) ||
		    hipMemcpyAsync(h_fn.data(), c->d_freg_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(h_np.data(), c->d_npri.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(h_tn.data(), c->d_task_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(h_rn.data(), c->d_rec_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(h_pr.data(), c->d_pe_read.p, (size_t)n * sizeof(PeRead), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(h_dbg.data(), c->d_pair_dbg.p, h_dbg.size() * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipMemcpyAsync(&err, pl.err, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return BWAHIP_ENODEV;
		return 0;
	};
	rc = queue();
	if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = BWAHIP_ENODEV;
	if (rc) return rc;
	if (err) { fprintf(stderr, "[bwahip] paired-end kernels reported code %d\n", err); return BWAHIP_EINTERNAL; }
	std::vector<int64_t> o, v;
	std::vector<std::pair<uint64_t, int>> by_hash;
	for (int i = 0; i < n; ++i) {
		const int m = L.regn[i];
		if (h_fn[i] != m) return BWAHIP_EINTERNAL;
		const uint64_t id = (((uint64_t)n_processed >> 1) + (uint64_t)(i >> 1)) << 1 | (uint64_t)(i & 1);
		by_hash.clear();
		for (int k = 0; k < m; ++k) by_hash.emplace_back(kat_hash_64(id + (uint64_t)k), k);
		std::sort(by_hash.begin(), by_hash.end());
		v = { (int64_t)i, (int64_t)m };
		stage_rec(o, 100, v);
		const PeRead &q = h_pr[i];
		const int *g = &h_dbg[(size_t)(i >> 1) * 3];
		v = { q.mode, q.h_reg, q.alt_reg, q.mapq, q.extra_flag, g[0], g[1], g[2], (int64_t)m, (int64_t)h_np[i], (int64_t)h_tn[i], (int64_t)h_rn[i] };
		for (int k = 0; k < m; ++k) {
			const size_t s = (size_t)reg_off[i] + k;
			const FinReg &p = h_f[s];
			uint32_t u; memcpy(&u, &p.frac_rep, 4);
			const auto it = std::lower_bound(by_hash.begin(), by_hash.end(), std::make_pair(p.hash, 0));
			const int64_t w[BWAHIP_KAT_PAIR_WORDS] = { p.rb, p.re, p.qb, p.qe, p.rid, p.score, p.truesc, p.sub, p.alt_sc, p.csub, p.sub_n, p.w, p.seedcov, p.secondary, p.secondary_all,
			                                           p.seedlen0, p.n_comp, p.is_alt, (int64_t)u, it != by_hash.end() && it->first == p.hash ? it->second : -1, h_need[s], h_own[s] };
			v.insert(v.end(), w, w + BWAHIP_KAT_PAIR_WORDS);
		}
		stage_rec(o, BWAHIP_KAT_PAIR_TAG, v);
	}
	*out = (int64_t*)malloc(o.size() * 8 + 8);
	if (!*out) return BWAHIP_ENOMEM;
	memcpy(*out, o.data(), o.size() * 8);
	*out_len = (int64_t)o.size();
	return 0;
}

// ------------------------------------------------------------------ the stream driver's stages (stream_pipe.h)
#include "stream_pipe.h"
#include <condition_variable>
#include <functional>
#include <mutex>

namespace {

double pipe_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the staging threads of one context: run(f) calls f(0 .. n-1), f(0) on the calling thread, and returns when all are back
struct StagePool {
	std::vector<std::thread> th;
	std::mutex mu; std::condition_variable cv, cv_done;
	const std::function<void(int)> *job = nullptr;
	long gen = 0; int left = 0; bool quit = false;
	int size() const { return (int)th.size() + 1; }
	void start(int n)
	{
		for (int t = 1; t < n; ++t) th.emplace_back([this, t] {
			long seen = 0;
			for (;;) {
				const std::function<void(int)> *f;
				{ std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return quit || gen != seen; }); if (quit) return; seen = gen; f = job; }
				(*f)(t);
				{ std::lock_guard<std::mutex> lk(mu); if (--left == 0) cv_done.notify_all(); }
			}
		});
	}
	void run(const std::function<void(int)> &f)
	{
		if (th.empty()) { f(0); return; }
		{ std::lock_guard<std::mutex> lk(mu); job = &f; left = (int)th.size(); ++gen; }
		cv.notify_all();
		f(0);
		std::unique_lock<std::mutex> lk(mu);
		cv_done.wait(lk, [&] { return left == 0; });
	}
	void stop()
	{
		{ std::lock_guard<std::mutex> lk(mu); quit = true; }
		cv.notify_all();
		for (auto &t : th) t.join();
		th.clear(); quit = false; gen = 0;
	}
};

// the GPU time of the sort stage that filled the set (record table, radix sort, gather)
double sort_stage_ms(const BatchOut &o) { float ms = 0; if (o.n_rec && o.ev_sort[0] && hipEventElapsedTime(&ms, o.ev_sort[0], o.ev_sort[3]) != hipSuccess) ms = 0; return ms; }

} // namespace

struct StreamPipe {
	BatchIn in[PIPE_SETS];
	BatchOut out[PIPE_SETS];
	PinnedOut pin[PIPE_SETS];
	StagePool pool;
};

long pipe_realloc_count() { return g_bwahip_reallocs.load(); }

int pipe_open(bwahip_ctx *c, int n_threads)
{
	if (!c) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (!c->pipe) {
		std::unique_ptr<StreamPipe> p(new StreamPipe);              // the context's only once all of it exists
		int rc;
		for (auto &s : p->in) if ((rc = s.ev.make(hipEventDisableTiming))) return rc;
		for (auto &s : p->pin) if ((rc = s.ev_written.make(hipEventDisableTiming)) || (rc = s.ev_copied.make(hipEventDisableTiming))) return rc;
		c->pipe = p.release();
	}
	c->pipe->pool.start(n_threads > 1 ? n_threads : 1);
	return 0;
}

void pipe_close(bwahip_ctx *c)
{
	if (!c || !c->pipe) return;
	(void)hipSetDevice(c->device);
	for (const Stream *s : { &c->stream_copy, &c->stream2, &c->stream3, &c->stream }) if (*s) (void)hipStreamSynchronize(*s);
	c->pipe->pool.stop();
}

void pipe_destroy(bwahip_ctx *c)
{
	delete c->pipe;
	c->pipe = nullptr;
}

// What stage_codes + stage_text do for bwahip_process_seqs, in two passes of the context's staging threads and without writing to the
// reader's records: pass 1 the per-chunk totals (two strlen per read), the longest read and the checks; pass 2 the offsets and the gather
// of bases, qualities, names and comments, all into one pinned buffer.  The bases travel as ASCII and become codes in HBM (k_nt4_conv).
int pipe_stage_in(bwahip_ctx *c, int in, const bwahip_opt_t *opt, int n, const bwahip_seq_t *seqs, OutForm form, double *t_copy_begin)
{
	if (!c || !c->pipe || in < 0 || in >= PIPE_SETS || !opt || n <= 0 || !seqs) return BWAHIP_EINVAL;
	const bool pe = (opt->flag & BWAHIP_F_PE) != 0;
	if (pe && (n & 1)) return BWAHIP_EINVAL;
	if (!c->knobs.gpu_final || (pe && !c->knobs.gpu_pair)) return BWAHIP_EINVAL;   // the one-piece output exists on the GPU path only
	if (is_bam(form)) { const int rc_bam = bam_check_reads(n, seqs); if (rc_bam) return rc_bam; }
	HIP_TRY(hipSetDevice(c->device));
	BatchIn &s = c->pipe->in[in];
	StagePool &pool = c->pipe->pool;
	const int C = n >= 4096 ? pool.size() : 1;
	struct Tot { int64_t seq = 0, qual = 0, name = 0, comm = 0; int bad = 0, any_comm = 0, max_len = 0, long_read = -1, name_diff = 0; char pad[12]; };
	std::vector<Tot> tot(C + 1);
	auto chunk = [&](int k) { return ((int64_t)n * k / C) & ~(int64_t)1; };   // even: mates stay in one chunk
	auto chunk_end = [&](int k) { return k + 1 == C ? (int64_t)n : chunk(k + 1); };
	pool.run([&](int k) {
		if (k >= C) return;
		Tot x;
		for (int64_t i = chunk(k); i < chunk_end(k); ++i) {
			if (seqs[i].l_seq < 0 || !seqs[i].name || !seqs[i].seq) { x.bad = 1; continue; }
			const int64_t ln = (int64_t)strlen(seqs[i].name) + 1, lc = seqs[i].comment ? (int64_t)strlen(seqs[i].comment) : 0;
			if (seqs[i].l_seq > BWAHIP_MAX_READ_LEN && x.long_read < 0) x.long_read = (int)i;
			if (seqs[i].l_seq > x.max_len) x.max_len = seqs[i].l_seq;
			if (pe && (i & 1) && seqs[i - 1].name && strcmp(seqs[i - 1].name, seqs[i].name) != 0) x.name_diff = 1;
			x.seq += seqs[i].l_seq; x.qual += seqs[i].qual ? seqs[i].l_seq : 0; x.name += ln; x.comm += lc ? lc + 1 : 0; x.any_comm |= lc > 0;
		}
		tot[k + 1] = x;
	});
	s.any_comment = false; s.max_len = 0;
	for (int k = 1; k <= C; ++k) {
		if (tot[k].bad) return BWAHIP_EINVAL;
		if (tot[k].name_diff) { fprintf(stderr, "[bwahip] paired reads have different names\n"); return BWAHIP_EINVAL; }   // err_fatal in the reference (bwamem_pair.c:386)
		if (tot[k].long_read >= 0) { fprintf(stderr, "[bwahip] read %d is %d bases long (limit %d)\n", tot[k].long_read, seqs[tot[k].long_read].l_seq, BWAHIP_MAX_READ_LEN); return BWAHIP_ECAPACITY; }
		s.any_comment |= tot[k].any_comm != 0;
		if (tot[k].max_len > s.max_len) s.max_len = tot[k].max_len;
		tot[k].seq += tot[k - 1].seq; tot[k].qual += tot[k - 1].qual; tot[k].name += tot[k - 1].name; tot[k].comm += tot[k - 1].comm;
	}
	const int64_t n_codes = tot[C].seq, n_qual = tot[C].qual, n_names = tot[C].name, n_comm = tot[C].comm;
	const size_t sz_off = (((size_t)n + 1) * 8 + 63) & ~(size_t)63;
	const size_t sz_codes = ((size_t)n_codes + 64) & ~(size_t)63, sz_qual = ((size_t)n_qual + 127) & ~(size_t)63, sz_names = ((size_t)n_names + 127) & ~(size_t)63;
	const size_t sz_comm = s.any_comment ? ((size_t)n_comm + 127) & ~(size_t)63 : 0;
	// the set is this stage's alone: its buffers grow here, before anything is queued on them
	int rc;
	if ((rc = s.h_stage.ensure(4 * sz_off + sz_codes + sz_qual + sz_names + sz_comm))) return rc;
	if ((rc = s.d_seq.ensure(sz_codes)) || (rc = s.d_off.ensure(sz_off)) || (rc = s.d_qual.ensure(sz_qual)) || (rc = s.d_qual_off.ensure(sz_off + 16)) || (rc = s.d_names.ensure(sz_names)) ||
	    (rc = s.d_name_off.ensure(sz_off)) || (rc = s.d_comment_off.ensure(sz_off)) || (s.any_comment && (rc = s.d_comments.ensure(sz_comm)))) return rc;
	int64_t *off = (int64_t*)s.h_stage.p, *qoff = off + sz_off / 8, *noff = qoff + sz_off / 8, *coff = noff + sz_off / 8;
	uint8_t *codes = (uint8_t*)(coff + sz_off / 8), *qual = codes + sz_codes, *names = qual + sz_qual, *comments = names + sz_names;
	off[0] = noff[0] = coff[0] = 0;
	pool.run([&](int k) {
		if (k >= C) return;
		int64_t so = tot[k].seq, qo = tot[k].qual, no = tot[k].name, co = tot[k].comm;
		for (int64_t i = chunk(k); i < chunk_end(k); ++i) {
			const int l = seqs[i].l_seq;
			memcpy(codes + so, seqs[i].seq, (size_t)l);
			so += l; off[i + 1] = so;
			if (seqs[i].qual) { memcpy(qual + qo, seqs[i].qual, (size_t)l); qoff[i] = qo; qo += l; } else qoff[i] = -1;
			const int64_t ln = (int64_t)strlen(seqs[i].name) + 1, lc = seqs[i].comment ? (int64_t)strlen(seqs[i].comment) : 0;
			memcpy(names + no, seqs[i].name, (size_t)ln);
			no += ln; noff[i + 1] = no;
			if (lc) { memcpy(comments + co, seqs[i].comment, (size_t)lc + 1); co += lc + 1; }
			coff[i + 1] = co;
		}
	});
	memset(codes + n_codes, 0, sz_codes - (size_t)n_codes); memset(qual + n_qual, 0, sz_qual - (size_t)n_qual); memset(names + n_names, 0, sz_names - (size_t)n_names);
	if (s.any_comment) memset(comments + n_comm, 0, sz_comm - (size_t)n_comm);
	s.n = n; s.total_bases = n_codes;
	if (t_copy_begin) *t_copy_begin = pipe_now();
	hipStream_t st = c->stream_copy;
	HIP_TRY(hipMemcpyAsync(s.d_seq.p, codes, (size_t)n_codes ? (size_t)n_codes : 1, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(s.d_off.p, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(s.d_qual.p, qual, sz_qual, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(s.d_qual_off.p, qoff, (size_t)n * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(s.d_names.p, names, sz_names, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(s.d_name_off.p, noff, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(s.d_comment_off.p, coff, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
	if (s.any_comment) HIP_TRY(hipMemcpyAsync(s.d_comments.p, comments, sz_comm, hipMemcpyHostToDevice, st));
	HIP_TRY(hipEventRecord(s.ev, st));
	HIP_TRY(hipEventSynchronize(s.ev));
	return 0;
}

int pipe_compute(bwahip_ctx *c, int in, int out, const bwahip_opt_t *opt, int64_t n_processed, const bwahip_pestat_t *pes0, OutForm form, double *t_hot_end)
{
	if (!c || !c->pipe || in < 0 || in >= PIPE_SETS || out < 0 || out >= PIPE_SETS || !opt) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	// run_pipeline and run_final work on what the context points at: the two sets for this batch, its own again whatever happens
	struct OnSets {
		bwahip_ctx *c;
		OnSets(bwahip_ctx *c, BatchIn *in, BatchOut *out) : c(c) { c->in = in; c->out = out; }
		~OnSets() { c->in = &c->own_in; c->out = &c->own_out; }
	} on_sets(c, &c->pipe->in[in], &c->pipe->out[out]);
	int rc;
	HIP_TRY(hipStreamWaitEvent(c->stream, c->in->ev, 0));
	if ((rc = launch_nt4(c->in->d_seq.as<uint8_t>(), c->in->total_bases, c->stream))) return rc;
	if ((rc = run_pipeline(c, opt, false, false))) return rc;
	if (t_hot_end) *t_hot_end = pipe_now();
	if ((rc = run_final(c, opt, n_processed, pes0, false, form))) return rc;
	HIP_TRY(hipEventRecord(c->pipe->pin[out].ev_written, c->stream));
	return 0;
}

int pipe_stage_out(bwahip_ctx *c, int out, const char **text, int64_t *len, double *t_kernels_end)
{
	if (!c || !c->pipe || out < 0 || out >= PIPE_SETS || !text || !len) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	BatchOut &o = c->pipe->out[out];
	PinnedOut &pin = c->pipe->pin[out];
	// waiting on the host, not in the copy stream: the next batch's upload is queued there and must not stand behind this batch's kernels
	HIP_TRY(hipEventSynchronize(pin.ev_written));
	if (t_kernels_end) *t_kernels_end = pipe_now();
	int64_t total = o.total;
	if (o.form == OutForm::Bgzf) {                                              // what travels is the members: their total was left in HBM by the deflate stage
		int64_t tot[2] = { 0, 0 };
		HIP_TRY(hipMemcpyAsync(tot, o.d_tot.p, 16, hipMemcpyDeviceToHost, c->stream_copy));
		HIP_TRY(hipEventRecord(pin.ev_copied, c->stream_copy));
		HIP_TRY(hipEventSynchronize(pin.ev_copied));
		total = tot[0]; o.n_stored = tot[1];
	}
	int rc = pin.h_sam.ensure((size_t)total + 1);
	if (rc) return rc;
	char *p = (char*)pin.h_sam.p;
	// in slices, each awaited before the next is queued: an upload the stager queues meanwhile waits for one slice at the most
	constexpr int64_t SLICE = 64 << 20;
	for (int64_t b = 0; b < total; b += SLICE) {
		HIP_TRY(hipMemcpyAsync(p + b, (const char*)o.d_sam.p + b, (size_t)std::min(SLICE, total - b), hipMemcpyDeviceToHost, c->stream_copy));
		HIP_TRY(hipEventRecord(pin.ev_copied, c->stream_copy));
		HIP_TRY(hipEventSynchronize(pin.ev_copied));
	}
	p[total] = 0;
	*text = p; *len = total;
	return 0;
}

// After pipe_stage_out of a batch computed as OutForm::BamSorted: the keys and offsets of the set's records in its pinned buffers (valid as long
// as the text), and the time the sort stage took on the GPU.
int pipe_stage_out_sorted(bwahip_ctx *c, int out, const uint64_t **keys, const int64_t **rec_off, int64_t *n_rec, double *sort_ms)
{
	if (!c || !c->pipe || out < 0 || out >= PIPE_SETS || !keys || !rec_off || !n_rec) return BWAHIP_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	const BatchOut &o = c->pipe->out[out];
	PinnedOut &pin = c->pipe->pin[out];
	if (!is_sorted(o.form)) return BWAHIP_EINVAL;
	int rc;
	if ((rc = pin.h_keys.ensure((size_t)(o.n_rec ? o.n_rec : 1) * 8)) || (rc = pin.h_rec_off.ensure((size_t)(o.n_rec + 1) * 8))) return rc;
	if (o.n_rec) HIP_TRY(hipMemcpyAsync(pin.h_keys.p, o.d_keys.p, (size_t)o.n_rec * 8, hipMemcpyDeviceToHost, c->stream_copy));
	if (o.n_rec) HIP_TRY(hipMemcpyAsync(pin.h_rec_off.p, o.d_rec_off.p, (size_t)(o.n_rec + 1) * 8, hipMemcpyDeviceToHost, c->stream_copy));
	else *(int64_t*)pin.h_rec_off.p = 0;
	HIP_TRY(hipEventRecord(pin.ev_copied, c->stream_copy));
	HIP_TRY(hipEventSynchronize(pin.ev_copied));
	if (sort_ms) *sort_ms = sort_stage_ms(o);
	*keys = (const uint64_t*)pin.h_keys.p; *rec_off = (const int64_t*)pin.h_rec_off.p; *n_rec = o.n_rec;
	return 0;
}

// Instead of pipe_stage_out + pipe_stage_out_sorted when the run stays in HBM: the set's records, keys and offsets into device buffers of
// the run's own (k_bammerge.hip), on the copy stream.
int pipe_stage_out_devrun(bwahip_ctx *c, int out, DevRun **run, int64_t *raw_len, int64_t *n_rec, double *sort_ms, double *t_kernels_end)
{
	if (!c || !c->pipe || out < 0 || out >= PIPE_SETS || !run || !raw_len || !n_rec) return BWAHIP_EINVAL;
	*run = nullptr;
	HIP_TRY(hipSetDevice(c->device));
	const BatchOut &o = c->pipe->out[out];
	HIP_TRY(hipEventSynchronize(c->pipe->pin[out].ev_written));
	if (t_kernels_end) *t_kernels_end = pipe_now();
	if (!is_sorted(o.form)) return BWAHIP_EINVAL;
	if (sort_ms) *sort_ms = sort_stage_ms(o);
	*raw_len = o.total; *n_rec = o.n_rec;
	int rc = bam_devrun_make(c, o.d_sam.as<uint8_t>(), o.total, o.d_keys.as<uint64_t>(), o.d_rec_off.as<int64_t>(), o.n_rec, c->stream_copy, run);
	if (!rc && o.form == OutForm::BamSortedDup && (rc = bam_devrun_add_dup(*run, o.d_tmpl.as<uint32_t>(), o.d_desc.as<bwahip_dup_desc_t>(), o.n_tmpl, c->stream_copy))) { bam_devrun_free(*run); *run = nullptr; }
	return rc == BWAHIP_ENOMEM ? 0 : rc;
}

// After pipe_stage_out of a batch computed as OutForm::Bgzf: the bytes of the records the members hold, the members, those that are stored,
// and the GPU time of the deflate stage.
int pipe_stage_out_bgzf(bwahip_ctx *c, int out, int64_t *raw_len, int64_t *n_blocks, int64_t *n_stored, double *deflate_ms)
{
	if (!c || !c->pipe || out < 0 || out >= PIPE_SETS || !raw_len || !n_blocks || !n_stored) return BWAHIP_EINVAL;
	const BatchOut &o = c->pipe->out[out];
	if (o.form != OutForm::Bgzf) return BWAHIP_EINVAL;
	*raw_len = o.total; *n_blocks = o.n_blocks; *n_stored = o.n_stored;
	if (deflate_ms) { float ms = 0; if (o.ev_bgzf[0] && hipEventElapsedTime(&ms, o.ev_bgzf[0], o.ev_bgzf[1]) != hipSuccess) ms = 0; *deflate_ms = ms; }
	return 0;
}
