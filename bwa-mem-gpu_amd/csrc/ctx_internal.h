// Context of libbwahip (one GPU, one index resident in HBM, the batch buffers) -- shared by the host translation units
// runtime.hip (hot path sequencing, C ABI) and final_rt.hip (finalisation / SAM sequencing).
#pragma once
#include "bwahip_internal.h"
#include "own.h"
#include "upload_once.h"
#include <atomic>
#include <memory>
#include <string>
#include <utility>

// hipFree / hipMalloc / hipHostMalloc synchronise the whole device: counted, so that the stream driver can report how many a pass paid
// (BWAHIP_STREAM_LOG; a steady pass of equal batches pays none)
inline std::atomic<long> g_bwahip_reallocs{0};
// what the library owns in this process (bwahip_live_resources): device buffers, their bytes, pinned buffers, their bytes, events, streams
inline std::atomic<int64_t> g_bwahip_live[6];

// ------------------------------------------------------------------ owners of HIP resources (own.h: the buffer type itself)
struct DevMem {
	static constexpr size_t slack = 256;
	static constexpr const char *what = "hipMalloc";
	static void *alloc(size_t bytes)
	{
		void *p = nullptr;
		if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		++g_bwahip_live[0]; g_bwahip_live[1] += (int64_t)bytes;
		return p;
	}
	static void free(void *p, size_t bytes) { (void)hipFree(p); --g_bwahip_live[0]; g_bwahip_live[1] -= (int64_t)bytes; }
	static void count_sync() { ++g_bwahip_reallocs; }
};
struct PinnedMem {
	static constexpr size_t slack = 4096;
	static constexpr const char *what = "hipHostMalloc";
	static void *alloc(size_t bytes)
	{
		void *p = nullptr;
		if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		++g_bwahip_live[2]; g_bwahip_live[3] += (int64_t)bytes;
		return p;
	}
	static void free(void *p, size_t bytes) { (void)hipHostFree(p); --g_bwahip_live[2]; g_bwahip_live[3] -= (int64_t)bytes; }
	static void count_sync() { ++g_bwahip_reallocs; }
};
using DevBuf = Buf<DevMem>;              // device memory; adopt(): caller-owned (bwahip_batch_attach, bwahip_init_device)
using HostBuf = Buf<PinnedMem>;          // pinned host staging buffer

// An event / a stream the library made: move-only, destroyed with its owner, passed wherever HIP takes the handle
struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
	Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e = o.e; o.e = nullptr; } return *this; }
	~Event() { reset(); }
	int make(unsigned flags = hipEventDefault)
	{
		reset();
		if (hipEventCreateWithFlags(&e, flags) != hipSuccess) { (void)hipGetLastError(); e = nullptr; return BWAHIP_ENODEV; }
		++g_bwahip_live[4];
		return 0;
	}
	void reset() { if (e) { (void)hipEventDestroy(e); --g_bwahip_live[4]; e = nullptr; } }
	operator hipEvent_t() const { return e; }
};
struct Stream {
	hipStream_t s = nullptr;
	Stream() = default;
	Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
	Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); s = o.s; o.s = nullptr; } return *this; }
	~Stream() { reset(); }
	int make(unsigned flags = hipStreamNonBlocking)
	{
		reset();
		if (hipStreamCreateWithFlags(&s, flags) != hipSuccess) { (void)hipGetLastError(); s = nullptr; return BWAHIP_ENODEV; }
		++g_bwahip_live[5];
		return 0;
	}
	void reset() { if (s) { (void)hipStreamDestroy(s); --g_bwahip_live[5]; s = nullptr; } }
	operator hipStream_t() const { return s; }
};

// Tuning knobs (hand-off thresholds of the heavy-read kernels).  Read from the environment ONCE, when the context is
// created; bwahip_ctx_tune changes them afterwards (tests force every hand-off kernel onto ordinary reads that way).
struct Knobs {
	int intv_cap = 96;          // BWAHIP_INTV_CAP: initial per-read interval capacity (grown on overflow)
	int smem_lanes = 1;         // BWAHIP_SMEM_LANES: lanes per read in k_smem (1, 2, 4, 8)
	int sa_intv = 1;            // BWAHIP_SA_INTV: interval of the SA table in HBM (1: every row, 8 bytes each; the index files' own interval or more: the files' table as it is); a table that would take over a quarter of the free HBM is built at the next interval that fits
	int kmer_k = 14;            // BWAHIP_KMER_K: the interval table holds the bi-intervals of all strings of up to kmer_k bases (16 bytes each, 4^k of them per length: 14 -> 5.7 GB, 15 -> 23 GB, 16 -> 92 GB; 0 or 1: no table); never longer than log4 of the text, nor than a quarter of the free HBM
	int smem_skip = -1;         // BWAHIP_SMEM_SKIP: depth J of k_smem's table jump -- a bwt_smem1a call starts at the table entry of its first J bases and materialises the J - 1 shorter ends by look-ups (same intervals).  -1: the largest J <= the table's depth with 4^J <= text length / 16 (3.1 Gbp: 14); 0: off; n >= 2: that depth.  Always clamped to the table's depth and, per batch, to min_seed_len
	int heavy_mult = -1;        // BWAHIP_HEAVY_MULT: hand a read to k_smem_heavy after heavy_mult x len extends (0: never; -1: 10 for reads up to 200 bases, 30 above -- a 250 bp read at 5 % error needs 2 500 extends on average, and the hand-off is for the outliers)
	int chain_mid_max = 1536, chain_big_max = 3200, chain_glb_grid = 2048;   // BWAHIP_CHAIN_MID_MAX / _BIG_MAX / _GLB_GRID: seeds up to which a read's B-tree lives in 77 KB / 150 KB of LDS (beyond: in global memory), and the workgroups of that last kernel
	int chain_big_min = 512;    // BWAHIP_CHAIN_BIG_MIN: seeds above which a wavefront-per-read chaining kernel takes the read (< 0: off)
	int rank_sort_min = 2;      // BWAHIP_RANK_SORT_MIN: dedup lists at least this long are sorted by the whole wavefront (shorter: the one-lane restatement of ks_introsort)
	int spec_min_chains = 16;   // BWAHIP_SPEC_MIN_CHAINS: chains from which k_extend_spec extends ahead of time (0: off)
	int ext_lds_window = 1 << 30;   // BWAHIP_EXT_LDS_WINDOW: reference windows above this go to k_extend_big (tests; default = the compiled LDS window)
	int ext_early_stop = 1;     // BWAHIP_EXT_EARLY_STOP: ksw_extend2 ends once no later row can change its results (0: every row to the end, as the reference -- same results, more rows)
	int ext_diag = 1;           // BWAHIP_EXT_DIAG: ksw_extend2 answers a flank of ACGT bases with at most K mismatches (1 at the default scores) from its main diagonal, without a DP row (0: every call runs its rows -- same results)
	int sorted_piece_blocks = 1024;   // BWAHIP_SORTED_PIECE_BLOCKS: BGZF blocks a device merger (k_bammerge.hip) gathers and deflates at a time (1 .. 4096; the bytes do not depend on it)
	int gpu_final = 1;          // BWAHIP_GPU_FINAL: 0 = finalisation of single-end batches on host threads (host_final.cpp) instead of the GPU kernels
	int gpu_pair = 1;           // BWAHIP_GPU_PAIR: 0 = paired-end batches finalised on host threads (mate rescue, pairing, SAM)
	int incr_insert = 1;        // mate rescue places a region into a clean list without sorting it again (k_pair.hip: incr_insert); 0 = every orientation ends in the full sort-and-dedup, as the reference -- same lists, more work (BWAHIP_INCR_INSERT)
	int verbose = 0;            // BWAHIP_VERBOSE
	int e2e_log = 0;            // BWAHIP_E2E_LOG: one line of phase timings per bwahip_process_seqs call
	const char *dump_ext = nullptr;   // BWAHIP_DUMP_EXT (diagnostic)
	void from_env()
	{
		auto geti = [](const char *k, int &v) { if (const char *e = getenv(k)) v = atoi(e); };
		geti("BWAHIP_INTV_CAP", intv_cap); geti("BWAHIP_SMEM_LANES", smem_lanes); geti("BWAHIP_HEAVY_MULT", heavy_mult); geti("BWAHIP_SMEM_SKIP", smem_skip); geti("BWAHIP_SA_INTV", sa_intv); geti("BWAHIP_KMER_K", kmer_k);
		geti("BWAHIP_CHAIN_BIG_MIN", chain_big_min); geti("BWAHIP_CHAIN_MID_MAX", chain_mid_max); geti("BWAHIP_CHAIN_BIG_MAX", chain_big_max); geti("BWAHIP_CHAIN_GLB_GRID", chain_glb_grid); geti("BWAHIP_RANK_SORT_MIN", rank_sort_min); geti("BWAHIP_SPEC_MIN_CHAINS", spec_min_chains); geti("BWAHIP_EXT_LDS_WINDOW", ext_lds_window); geti("BWAHIP_EXT_EARLY_STOP", ext_early_stop); geti("BWAHIP_EXT_DIAG", ext_diag); geti("BWAHIP_GPU_FINAL", gpu_final); geti("BWAHIP_GPU_PAIR", gpu_pair);
		verbose = getenv("BWAHIP_VERBOSE") != nullptr;
		e2e_log = getenv("BWAHIP_E2E_LOG") != nullptr;
		dump_ext = getenv("BWAHIP_DUMP_EXT");
		if (intv_cap < 2) intv_cap = 2;
		ext_early_stop = ext_early_stop != 0; ext_diag = ext_diag != 0;
		geti("BWAHIP_INCR_INSERT", incr_insert); incr_insert = incr_insert != 0;
		geti("BWAHIP_SORTED_PIECE_BLOCKS", sorted_piece_blocks);
		if (sorted_piece_blocks < 1 || sorted_piece_blocks > 4096) sorted_piece_blocks = 1024;
	}
};

// offsets of one host batch on its way to HBM (bwahip_process_seqs)
struct BatchText {
	std::vector<int64_t> off, qoff, noff, coff;
	int64_t qtot = 0;
	bool any_comment = false;
	size_t sz_codes = 0, sz_qual = 0, sz_names = 0, sz_comm = 0;
};

// Working set of the coordinate sort of a batch's BAM records (k_bamsort.hip), one per context.  Per record: two key and two ordinal
// buffers (the radix passes go back and forth), offset, length and sorted length; per read: record count and base; per pass: the
// (digit, workgroup) histogram and its scan; `raw`: the batch's records in input order (the sorted ones go to d_sam).
struct BamSort {
	DevBuf raw, rec_cnt, rec_base, keys[2], idx[2], off, len, len_sorted, hist, hist_base, bits;
	DevBuf tmpl;                         // OutForm::BamSortedDup: per record in input order the index of its template (k_markdup.hip)
	float ms[3] = { 0, 0, 0 };           // record table, radix sort, gather of the last timed run
	int n_passes = 0;                    // radix passes the last sort ran
};

// Working set of the deflate stage (k_bgzf.hip), one per context: a 64 KiB slot per BGZF block for the member as it is formed, the
// members' lengths and their scan, per workgroup of the grid one word per input position (match candidate, then length and distance),
// the count of blocks that left stored.
struct Bgzf {
	DevBuf slots, mlen, moff, md, cnt;
};

// The form a batch's output leaves run_final in (d_sam): SAM text; BAM records in read order (k_bam.hip); the records in coordinate order with their
// keys and offsets (k_bamsort.hip: written to bs.raw, sorted into d_sam); the records as BGZF members (k_bgzf.hip: written to bs.raw, deflated into d_sam)
// BamSortedDup: BamSorted, and what duplicate marking in a device merger needs (k_markdup.hip): per record its template's index, per template its descriptor
enum class OutForm { Sam, Bam, BamSorted, Bgzf, BamSortedDup };
inline bool is_bam(OutForm f) { return f != OutForm::Sam; }
inline bool is_sorted(OutForm f) { return f == OutForm::BamSorted || f == OutForm::BamSortedDup; }

// What a batch arrives in: bases (codes 0..4 once k_nt4_conv has run), qualities, names, comments and their offsets in HBM, the pinned buffer they
// travel through, and the event behind the last copy to HBM (stream path).  One type for the context's own batch and for the stream driver's sets.
struct BatchIn {
	DevBuf d_seq, d_off, d_qual, d_qual_off, d_names, d_name_off, d_comments, d_comment_off;
	HostBuf h_stage;
	Event ev;                            // the copies to HBM are done
	int n = 0, max_len = 0; int64_t total_bases = 0; bool any_comment = false;
	// a batch without comments: a null pointer tells the kernels (d_comments itself is kept from batch to batch)
	const uint8_t *comments() const { return any_comment ? d_comments.as<uint8_t>() : nullptr; }
};

// What run_final leaves behind: the batch in `form` in d_sam (`total` bytes of text or records; OutForm::Bgzf: of the records the members hold)
// with the reads' offsets; BamSorted: n_rec keys and n_rec + 1 offsets of the records, the events at the begin of the record table, of the
// radix sort, of the gather, and at the end; Bgzf: d_tot = [0] the members' bytes, [1] members that left stored (int64 each, in HBM), n_blocks
// members, the events around the deflate stage; n_stored: d_tot[1] once it has been read back.  BamSortedDup: beside the keys n_rec template
// indices in d_tmpl, and n_tmpl descriptors in d_desc (with the descriptor kernel's error word behind them).
struct BatchOut {
	DevBuf d_sam, d_sam_off, d_keys, d_rec_off, d_tot, d_tmpl, d_desc;
	Event ev_sort[4], ev_bgzf[2];
	int64_t total = 0, n_rec = 0, n_blocks = 0, n_stored = 0, n_tmpl = 0;
	OutForm form = OutForm::Sam;
};

// The pinned buffers a BatchOut comes back into -- one per set of the stream driver, two taken in turn for the context's own set (the one-piece
// entries of bwahip_process_seqs*) -- and the events of the way back (stream path): the write pass has ended / the bytes are in h_sam
struct PinnedOut {
	HostBuf h_sam, h_keys, h_rec_off, h_tmpl, h_desc;
	Event ev_written, ev_copied;
};

struct StreamPipe;                       // final_rt.hip: the second sets of batch buffers the stream driver's three stages work on

struct bwahip_ctx {
	StreamPipe *pipe = nullptr;          // made by the first bwahip_stream_run on this context, kept (buffers do not shrink), freed with the context
	BatchText batch_text;
	BamSort bs;
	Bgzf bz;
	// The batch of the direct entry points (bwahip_batch_upload / _attach*, bwahip_process_seqs*, the stage dumps) and what run_final makes of it.
	// Everything that computes goes through `in` / `out`: they point here, except while pipe_compute has them on two of the stream driver's sets.
	BatchIn own_in;
	BatchOut own_out;
	BatchIn *in = &own_in;
	BatchOut *out = &own_out;
	PinnedOut pin[2];                    // one-piece output of bwahip_process_seqs_text / _bam / _bam_sorted / _bgzf: taken in turn (plain bwahip_process_seqs: pin[0])
	int turn = 0;
	std::vector<int64_t> h_sam_off;      // offsets of the reads' SAM text in h_sam (bwahip_process_seqs / _text)
	bool external_index = false;
	bool index_resident = false;         // d_bwt / d_sa / d_pac were filled before ctx_setup (bwahip_init_rccl)
	Knobs knobs;
	std::string rg_id;                   // read-group id appended as RG:Z: to every record (bwa_rg_id, bwa.c:44); empty = none
	DevBuf d_logtab;                     // log(i), i < BWAHIP_LOGTAB_N, from the host's libm (bwamem.c:607, 974-981)         // index arrays live in caller-owned HBM (bwahip_init_device)
	int device = 0;
	Stream stream_copy;                  // uploads that run beside the kernels (bwahip_process_seqs: names / qualities during the hot path)
	Event ev_sam_half; int sam_half_reads = 0;   // run_final: recorded when the SAM text of reads [0, sam_half_reads) is written
	Event ev_slice[8];                   // bwahip_process_seqs: one per slice of the SAM download
	Stream stream, stream2, stream3;   // stream2/3: kernels that run beside the main one (k_chain_big)
	Event ev_fork, ev_join, ev_join3;
	HostIndex host = {};                 // host copy: contig table + packed reference (always owned); FM-index arrays only when loaded from files
	DevIndex ix;
	DevBuf d_bwt, d_sa, d_pac, d_anns;
	DevBuf d_bwtp;                       // bit-plane copy of a caller-owned BWT (bwahip_init_device); otherwise d_bwt itself is re-laid in place
	bool bwt_is_planes = false;          // d_bwt already holds the bit-plane layout (bwahip_ctx_clone_on: copied from a context's array)
	DevBuf d_kmer;                       // the interval table of the BWT search (launch_kmer_table); clones read their source's
	const bwahip_ctx *share_from = nullptr;   // bwahip_ctx_clone: the context whose index arrays this one reads
	DevBuf d_sa_dense;                   // the SA table the kernels read when it is denser than the files' (launch_sa_densify); owned by the context that built it
	// working set of the batch
	DevBuf d_seq4, d_smem_heavy, d_raw, d_raw_n;
	DevBuf d_intv, d_intv_n, d_seed_cnt, d_lrep, d_seed_base, d_seeds, d_scratch;
	DevBuf d_misc;                       // CNT_SLOTS rows of CNT_N counters (u64), then queue (4 x u32), err (i32)
	// K3/K4 working set (sized from the seed count of the batch)
	DevBuf d_cw, d_nxt, d_ord, d_wts, d_kept, d_first, d_keep, d_nodes, d_stack;
	DevBuf d_chains, d_chain_seeds, d_chain_n, d_kept_seeds, d_reg_base, d_regs, d_tmp_regs, d_reg_n, d_srt;
	DevBuf d_dbg_chains, d_dbg_seeds, d_dbg_chain_n, d_dbg_regs, d_dbg_reg_n, d_flt, d_heavy, d_perm, d_spec_regs, d_spec_items, d_scan, d_chain_big, d_redo, d_big_t, d_dedup, d_cperm;
	// finalisation on the GPU (final_rt.hip)
	DevBuf d_ctg_names, d_ctg_name_off, d_ctg_anno, d_ctg_anno_off, d_rg;      // contig names / annotations (SAM RNAME, XR), read-group id
	DevBuf d_fregs, d_fregs2, d_fscr, d_need, d_xa_owner, d_freg_n, d_npri, d_task_n, d_rec_n, d_task_base, d_tasks, d_aln_of_reg, d_alns;
	DevBuf d_hist, d_pair_tab, d_nb, d_pe_cap, d_pe_base, d_pe_regs, d_pe_n, d_pe_tmp, d_pe_keys, d_pe_idx, d_resc, d_ms_slab, d_pe_read, d_sw_cnt, d_sw_base, d_sw_res, d_sw_tasks, d_sw_info;   // paired-end stages
	bwahip_pestat_t last_pes[4];         // insert-size statistics of the last paired-end batch
	unsigned long long last_sw_tasks = 0;   // alignments k_matesw_sw ran ahead of the list logic (BWAHIP_PE_LOG)
	unsigned long long last_sw_ahead[2] = { 0, 0 };   // alignments run ahead by the byte / the word kernel (bwahip_last_pe_paths)
	DevBuf d_pair_dbg;                   // stage dump: PairLaunch::pair_dbg
	static constexpr int PE_CNT_PATHS = 14, PE_CNT_N = PE_CNT_PATHS + PE_PATH_N;   // d_fmisc[5 .. 5 + PE_CNT_N) in one copy: the 9 counters, 5 words of other use, PairLaunch::paths
	unsigned long long last_pe_counters[PE_CNT_N] = { 0 };   // [0..3] mate-rescue alignments run / regions added / most per pair / pairs rescued
	DevBuf d_task_lists;                 // k_cigar's two work lists (no-DP tasks, DP tasks)
	DevBuf d_resc_flag;                  // one byte per pair: mate rescue works on it (finalised by the second k_mark / k_pair launch)
	DevBuf d_zslab;                      // k_cigar's backtrack slabs
	DevBuf d_resc_ord;                   // scratch of the rescue list's ordering
	DevBuf d_pool, d_fmisc, d_fredo, d_bigz, d_rec_list, d_xa_list, d_sam_len;
	int64_t total_tasks = 0;
	size_t pool_cap = 0;
	float dup_desc_ms = 0;               // k_dup_desc in the last bwahip_kat_dup_desc
	float final_ms[8] = { 0 };           // k_mark, k_cigar, k_sam(size), k_sam(write) of the last run
	int intv_cap = 96;                   // current capacity (starts at knobs.intv_cap, grows on overflow)
	int64_t total_seeds = 0, total_regs = 0;
	Event ev[24];
	float last_ms[24];
};


extern "C" int ctx_setup(bwahip_ctx *c, const bwahip_bwt_t *bwt, const bwahip_bns_t *bns, const uint8_t *pac);   // streams, tables, DevIndex
int launch_scan(const int *in, int64_t *out, int n, DevBuf &tmp, hipStream_t st);   // exclusive scan int32 -> int64, n+1 outputs
int launch_nt4(uint8_t *seq, int64_t n, hipStream_t st);   // runtime.hip: ASCII / codes -> codes 0..4 in place (nst_nt4_table)
int dev_upload(DevBuf &b, const void *src, size_t bytes, hipStream_t st);
int run_pipeline(bwahip_ctx *c, const bwahip_opt_t *opt, bool timed, bool dump);      // the hot path over the uploaded batch
// one region list as a stage record's words (bwahip_run_stages, bwahip_run_pe_stages): the count, then 19 words per region
inline void stage_put_regs(std::vector<int64_t> &v, int cnt, const DevReg *rg)
{
	auto f2i = [](float f) { uint32_t u; memcpy(&u, &f, 4); return (int64_t)u; };
	v.push_back(cnt);
	for (int k = 0; k < cnt; ++k) {
		const DevReg &p = rg[k];
		v.push_back(p.rb); v.push_back(p.re); v.push_back(p.qb); v.push_back(p.qe); v.push_back(p.rid);
		v.push_back(p.score); v.push_back(p.truesc); v.push_back(p.sub); v.push_back(0); v.push_back(p.csub);
		v.push_back(p.sub_n); v.push_back(p.w); v.push_back(p.seedcov); v.push_back(0);
		v.push_back(0); v.push_back(p.seedlen0); v.push_back(p.n_comp); v.push_back(p.is_alt);
		v.push_back(f2i(p.frac_rep));
	}
}
inline void stage_rec(std::vector<int64_t> &o, int64_t tag, const std::vector<int64_t> &v)
{
	o.push_back(tag); o.push_back((int64_t)v.size());
	o.insert(o.end(), v.begin(), v.end());
}
// pe_stage_stop: paired end only, for bwahip_run_pe_stages -- return once both k_pair passes are done (the stream is idle then), with mem_pair's
// results per pair in d_pair_dbg; nothing of the output stages runs
int run_final(bwahip_ctx *c, const bwahip_opt_t *opt, int64_t n_processed, const bwahip_pestat_t *pes0, bool timed, OutForm form, bool host_sam_off = false, bool pe_stage_stop = false);   // regions in HBM -> the batch in `form` in HBM (SE, or PE when opt->flag has MEM_F_PE); host_sam_off: the offsets travel to h_sam_off ahead of the write pass (bwahip_process_seqs)
// k_bamsort.hip: the records of c->bs.raw (per-read offsets c->out->d_sam_off, n_reads + 1) in coordinate order into c->out->d_sam, their keys
// into c->out->d_keys, their offsets into c->out->d_rec_off; sets c->out->n_rec.  Queued on c->stream (with two small read-backs awaited in between).
// dup_tmpl: 0, or the reads of a template (1, 2): then also the templates' descriptors into c->out->d_desc and the records' templates into c->out->d_tmpl
int bam_sort_batch(bwahip_ctx *c, int n_reads, int64_t total, int dup_tmpl = 0);
// the stable LSD radix sort of bam_sort_batch alone, over c->bs.keys[0] / idx[0] (n items): the result is in keys[*which] / idx[*which]
int bam_sort_radix(bwahip_ctx *c, int n, int key_bits, int *which);
int bam_sort_iota(unsigned *idx, int n, hipStream_t st);
int bam_sort_tile();
// k_bgzf.hip: `len` bytes at d_in (HBM) as BGZF members, cut every 65 280 bytes, concatenated into out (grown here to the bound
// len + 31 per block: a member is never longer than its stored form); tot[0] = the bytes of the members, tot[1] = members that are
// stored (both int64, in HBM: nothing is awaited).  Queued on st; len == 0 launches nothing but sets tot.
int bgzf_deflate(bwahip_ctx *c, const uint8_t *d_in, int64_t len, DevBuf &out, int64_t *tot_dev, hipStream_t st);
inline int64_t bgzf_blocks(int64_t len) { return (len + 65279) / 65280; }
// k_bammerge.hip: one sorted run in device buffers of its own (records, keys, n_rec + 1 offsets), as a device merger holds it.
// bam_devrun_make allocates them on c's device and copies from device pointers on st (one device-to-device copy each; awaited, so the
// source is free on return); a failed allocation: BWAHIP_ENOMEM and nothing is held.  bam_devmerger_adopt registers the run under
// run_no and owns it from then on (refused: the caller still owns it).  bam_devrun_download copies a run to host buffers of at least
// len, n_rec and n_rec + 1 items.
// With duplicate marking (has_dup): n_rec template indices and n_tmpl descriptors as well.
struct DevRun {
	int64_t n_rec = 0, len = 0; DevBuf d_rec, d_keys, d_off; int device = 0;   // allocated to size: no slack
	bool has_dup = false; int64_t n_tmpl = 0; DevBuf d_tmpl, d_desc;
	bool spilled = false; std::vector<int64_t> h_off;               // a spilled run (k_bamspill.hip): d_rec stays empty, the bytes are in the merger's store; the offsets on the host as well
	uint8_t *rec() const { return d_rec.as<uint8_t>(); }
	uint64_t *keys() const { return d_keys.as<uint64_t>(); }
	int64_t *off() const { return d_off.as<int64_t>(); }
	uint32_t *tmpl() const { return d_tmpl.as<uint32_t>(); }
	bwahip_dup_desc_t *desc() const { return d_desc.as<bwahip_dup_desc_t>(); }
};
int  bam_devrun_make(bwahip_ctx *c, const uint8_t *d_rec, int64_t len, const uint64_t *d_keys, const int64_t *d_rec_off, int64_t n_rec, hipStream_t st, DevRun **out);
int  bam_devrun_download(const DevRun *r, uint8_t *rec, uint64_t *keys, int64_t *rec_off, hipStream_t st);
void bam_devrun_free(DevRun *r);
// the run's template indices and descriptors, copied from device pointers on st as bam_devrun_make copies the records (BWAHIP_ENOMEM: the run is as before)
int  bam_devrun_add_dup(DevRun *r, const uint32_t *d_tmpl, const bwahip_dup_desc_t *d_desc, int64_t n_tmpl, hipStream_t st);
int  bam_devmerger_adopt(bwahip_bam_devmerger *m, int64_t run_no, DevRun *r);
// adopt, with the run held spilled (the merger is armed): its record bytes go device -> store on st and leave HBM, its offsets are kept on
// the host as well; *longest (may be null): its longest record.  Refused: the caller still owns the run, whole
int  bam_devmerger_window_pieces(const bwahip_bam_devmerger *m);   // of an armed merger: what set_spill resolved (0: not armed)
int  bam_devmerger_adopt_spilled(bwahip_bam_devmerger *m, int64_t run_no, DevRun *r, hipStream_t st, int64_t *longest);
// the device-to-device form of bwahip_bam_devmerger_add: make + adopt
int  bam_devmerger_add_dev(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *d_rec, int64_t len, const uint64_t *d_keys, const int64_t *d_rec_off, int64_t n_rec, hipStream_t st);
// the merger's runs in run-number order, handed to the caller (who frees them); the merger is empty afterwards.  A merger that holds a
// spilled run is refused (BWAHIP_EINVAL) and keeps its runs: their record bytes are in its store
int  bam_devmerger_take_runs(bwahip_bam_devmerger *m, std::vector<std::pair<int64_t, DevRun*>> *out);
// What one finish of a device merger runs beside the members, and where the stages' outputs go: resolved once, by the three
// bwahip_bam_devmerger_finish* entry points or by a sink of the stream driver.  The record stages (below) are the merger's armed state
// (bwahip_bam_devmerger_set_qc, _set_pileup, _set_recal), the windowed path follows from its runs: the finish fills it in.
struct FinishPlan {
	bool index = false; int bai_fd = -1; int64_t base = 0; int32_t n_ref = 0; bwahip_bai_stats_t *bs = nullptr;   // the .bai of what is written (base: the first member's offset in the file)
	bool mark = false; bwahip_markdup_stats_t *ms = nullptr;       // duplicates marked before anything is gathered (ms may be null)
	bool spill = false;                                            // filled in by the finish
};
int  bam_devmerger_finish(bwahip_bam_devmerger *m, int fd, bwahip_devmerge_stats_t *st, FinishPlan plan);
// k_bai.hip: the index stage of a device merger's finish.  bai_stage_members: room for the lengths of n_blocks members (the caller fills
// them, on c->stream); bai_stage_run: the index of the n records addr[idx[i]] (sorted order; out_off: their n + 1 offsets in the stream of
// `total` bytes) as the bytes of a .bai file -- queued on c->stream and awaited; the context's sort buffers (bs.keys / bs.idx) are reused
struct BaiStage;
BaiStage *bai_stage_new();
void bai_stage_free(BaiStage *s);
int  bai_stage_members(BaiStage *s, int64_t n_blocks, int **mlen);
int  bai_stage_run(BaiStage *s, bwahip_ctx *c, int n, const uint8_t *const *addr, const unsigned *idx, const int64_t *out_off, int64_t total, int64_t n_blocks, int64_t base,
                   int32_t n_ref, std::vector<uint8_t> *bytes, bwahip_bai_stats_t *bs, bool parsed = false);
// the parse alone, for a merger with spilled runs: bai_stage_parse_begin once (buffers, cleared tables), bai_stage_parse over the sorted
// ordinals [lo, hi) while their records -- and that of ordinal lo - 1 -- can be read; bai_stage_run(parsed = true) does the rest
int  bai_stage_parse_begin(BaiStage *s, bwahip_ctx *c, int n, int64_t n_blocks, int32_t n_ref);
int  bai_stage_parse(BaiStage *s, bwahip_ctx *c, int lo, int hi, const uint8_t *const *addr, const unsigned *idx, const int64_t *out_off, int32_t n_ref);
// k_markdup.hip.  Per batch, from bam_sort_batch: dup_batch_desc after the record table (descriptors, templates in input order), dup_batch_tmpl
// after the radix sort (templates in sorted order; awaits the descriptor kernel's error word).  The decision stage of a device merger's
// marked finish: desc = the descriptors of all runs in run order; markdup_decide leaves one byte per template in dup (queued on c->stream, the
// context's sort buffers are used); markdup_count and markdup_mark_run add to cnt ([0..5] templates and duplicates per kind, [6] records
// marked, [7] the marking pass's error word), which markdup_counters_reset zeroes.
struct MarkdupStage {
	Tally hbm;
	DevBuf desc{hbm}, head{hbm}, seg{hbm}, best{hbm}, pair_here{hbm}, dup{hbm}, cnt{hbm};
	Event ev[3];                         // begin, decision done, end
};
int dup_batch_desc(bwahip_ctx *c, int n_reads, bool paired, int64_t n_rec);
int dup_batch_tmpl(bwahip_ctx *c, int n_rec, const unsigned *idx);
int markdup_decide(MarkdupStage *s, bwahip_ctx *c, int64_t n_tmpl);
int markdup_counters_reset(MarkdupStage *s, bwahip_ctx *c);
int markdup_count(MarkdupStage *s, bwahip_ctx *c, int64_t n_tmpl);
// marked_to: where the records marked are counted (null: cnt[6]; a spilled run's record staged a second time counts elsewhere)
int markdup_mark_run(MarkdupStage *s, bwahip_ctx *c, uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, const uint32_t *tmpl, int64_t first_tmpl, int64_t n_tmpl,
                     unsigned long long *marked_to = nullptr);
// k_bamspill.hip: the window cuts of a merger with spilled runs (cut: n_windows rows of n_runs + 1 cells) and a window's source addresses
int spill_window_cuts(hipStream_t st, int n, int n_runs, const int64_t *first, const uint8_t *spilled, const unsigned *idx, const int *piece_first, int window_pieces, int n_windows, int *cut);
int spill_window_addr(hipStream_t st, int rec_lo, int n_rec, int n_runs, const int64_t *first, const int64_t *const *run_off, const uint8_t *spilled, const int64_t *base,
                      const unsigned *idx, const uint8_t **addr);
// A stage of a device merger's finish that reads every record once, run by run, on c->stream, changes none, and leaves a file of its own.  It
// holds what it was configured with (resolved options, checked contig lengths, where its reference comes from, the caller's stats struct) and
// its buffers, which later finishes use again.  hbm_need: the HBM it will allocate for that many records, as configured -- the public
// bwahip_*_hbm_need of its own resolved configuration, so whoever budgets for the stage (the stream driver's sinks, through
// bam_devmerger_record_stages_need) asks the stage that allocates.  begin: the layout, the tables cleared; records: one run, or one staged
// slice of one -- record i = rec[off[i] .. off[i + 1]) within the run's `len` bytes, ord0: the ordinal of its first record among all runs';
// done: the rest of the work, the one download (awaited), the file's bytes into `bytes` and the stats -- BWAHIP_EINVAL when a record was
// refused; write: the bytes to fd (fd < 0: nowhere).  n_records == 0 launches nothing.  takes_windows: a spilled run's slices may pass
// window by window, each gone when the next arrives -- not so for a stage whose done reads the runs again.
// A new stage: implement this, hbm_need included; give the merger a setter (k_bammerge.hip); give the stream driver's request its fields
// (SortedDevReq, stream.cpp).
struct RecordStage {
	bool armed = false; int fd = -1;
	std::vector<uint8_t> bytes;
	virtual ~RecordStage() = default;
	virtual int64_t hbm_need(int64_t n_records) const = 0;
	virtual int begin(bwahip_ctx *c, int64_t n_records) = 0;
	virtual int records(bwahip_ctx *c, const uint8_t *rec, const int64_t *off, int64_t n_rec, int64_t len, int64_t ord0) = 0;
	virtual int done(bwahip_ctx *c) = 0;
	virtual int write() = 0;
	virtual bool takes_windows() const = 0;
};
// the sum of hbm_need over the merger's armed record stages
int64_t bam_devmerger_record_stages_need(bwahip_bam_devmerger *m, int64_t n_records);
// The reference of a stage that reads one (the pileup, the recalibration table): the contigs' lengths and the table `lengths | first base
// (n_ref + 1)` on the host and in HBM, and the packed reference -- the caller's, copied by set() and uploaded once per set(), or (pac null)
// the context's, read where it lies.  The buffers count in the stage's tally.  A call in flight: begin(c), which says where the packed
// reference will come from (BWAHIP_EINVAL: bases, and no packed reference anywhere), then, when there are records, upload(q): the table and,
// if it is due, the caller's reference, in that order on q.  d_pac is good from then on.
struct DevUpload { static int upload(DevBuf &b, const void *src, size_t bytes, hipStream_t q) { return dev_upload(b, src, bytes, q); } };
using DevOnce = UploadOnce<DevBuf, DevUpload>;
struct StageRef {
	std::vector<int64_t> len, h_tab;
	int32_t n_ref = 0; int64_t sum = 0, pac_bytes = 0;
	DevBuf tab; DevOnce own;
	const uint8_t *d_pac = nullptr;
	explicit StageRef(Tally &t) : tab(t), own(t) {}
	const int64_t *d_len() const { return tab.as<int64_t>(); }
	const int64_t *d_off() const { return tab.as<int64_t>() + n_ref; }
	void set(int32_t n, const int64_t *ref_len, const uint8_t *pac)
	{
		n_ref = n; len.assign(ref_len, ref_len + n);
		h_tab.assign(2 * (size_t)n + 1, 0);
		for (int32_t r = 0; r < n; ++r) { h_tab[(size_t)r] = ref_len[r]; h_tab[(size_t)n + r + 1] = h_tab[(size_t)n + r] + ref_len[r]; }
		sum = h_tab[2 * (size_t)n]; pac_bytes = (sum + 3) / 4;
		own.set(pac, (size_t)pac_bytes);
	}
	int begin(const bwahip_ctx *c) { d_pac = own.held ? nullptr : c->d_pac.as<uint8_t>(); return sum && !d_pac && !own.held ? BWAHIP_EINVAL : 0; }
	int upload(hipStream_t q)
	{
		int rc = dev_upload(tab, h_tab.data(), h_tab.size() * 8, q);
		if (!rc && !(rc = own.begin(q)) && own.held) d_pac = own.d.as<uint8_t>();
		return rc;
	}
};
// k_qc.hip: the QC summary.  k_pileup.hip: the pileup -- pac: the packed reference of these contigs (StageRef: null is the context's).
// k_recal.hip: the recalibration table -- pac as for the pileup, mask: the known sites over these contigs' bases, copied and uploaded
// likewise (null: none).  *_set: resolved options and checked lengths; the stats struct may be null
RecordStage *qc_stage_new();
void qc_stage_set(RecordStage *s, const bwahip_qc_opt_t &opt, int32_t n_ref, const int64_t *ref_len, int fd, bwahip_qc_stats_t *qs);
RecordStage *pu_stage_new();
void pu_stage_set(RecordStage *s, const bwahip_pileup_opt_t &opt, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, int fd, bwahip_pileup_stats_t *ps);
RecordStage *recal_stage_new();
void recal_stage_set(RecordStage *s, const bwahip_recal_opt_t &opt, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const uint8_t *mask, int fd, bwahip_recal_stats_t *st);
// k_bammerge.hip: exactly a configured stage on the caller's records, uploaded as one run (bwahip_kat_qc, bwahip_kat_pileup, bwahip_kat_recal); the file's bytes to out
int  record_stage_kat(RecordStage *s, bwahip_ctx *c, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, uint8_t *out, int64_t out_cap, int64_t *out_len);
int bam_check_reads(int n, const bwahip_seq_t *seqs);   // bam_host.cpp: BWAHIP_EINVAL (with a message naming the read) for a name or a comment BAM cannot hold
void pipe_destroy(bwahip_ctx *c);                                                     // final_rt.hip: the stream driver's buffer sets
int final_setup(bwahip_ctx *c);                                                       // contig name tables for the SAM kernels
