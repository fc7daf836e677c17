/* bwahip.h -- C ABI of the MI355X-native BWA-MEM hot path.
 *
 * This is the drop-in boundary: a thin `extern "C"` launcher that replaces the
 * reference's CUDA seam (cuda/bwamem_GPU.cuh:13 mem_align_GPU,
 * cuda/streams.cuh:21-63 newProcess/newTransfer/..., cuda/bwt_CUDA.cuh,
 * cuda/ksw_CUDA.cuh) behind the unchanged host surface
 *     mem_process_seqs()   bwamem.h:69 / bwamem.c:1215
 *     mem_align1_core()    bwamem.c:1061   (= the per-read work of worker1, bwamem.c:1183)
 * Plain pointers and sizes only; no C++/torch types.  Every struct below is a
 * layout mirror of the reference's own struct (cited), so a reference
 * translation unit can pass its objects straight through.
 * All functions return 0 on success and a negative BWAHIP_E* code on failure;
 * nothing here ever falls back to a CPU implementation of the hot path.
 */
#ifndef BWAHIP_H
#define BWAHIP_H

#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- layout mirrors of reference types --------------------------------- */

typedef struct {                 /* bwt_t, bwt.h:48-60 */
	uint64_t primary;
	uint64_t L2[5];
	uint64_t seq_len;
	uint64_t bwt_size;           /* number of uint32 words in `bwt` */
	uint32_t *bwt;               /* Occ-interleaved BWT: per 128 bases 4 x u64 counts + 8 x u32 (bwtindex.c:150) */
	uint32_t cnt_table[256];
	int sa_intv;
	uint64_t n_sa;
	uint64_t *sa;
} bwahip_bwt_t;

typedef struct {                 /* bntann1_t, bntseq.h:41-48 */
	int64_t offset;
	int32_t len;
	int32_t n_ambs;
	uint32_t gi;
	int32_t is_alt;
	char *name, *anno;
} bwahip_ann_t;

typedef struct {                 /* bntamb1_t, bntseq.h:50-54 */
	int64_t offset;
	int32_t len;
	char amb;
} bwahip_amb_t;

typedef struct {                 /* bntseq_t, bntseq.h:56-64 */
	int64_t l_pac;
	int32_t n_seqs;
	uint32_t seed;
	bwahip_ann_t *anns;
	int32_t n_holes;
	bwahip_amb_t *ambs;
	FILE *fp_pac;
} bwahip_bns_t;

typedef struct {                 /* bseq1_t, bwa.h:58-63 (fork layout: l_name/l_comment/l_qual appended) */
	int l_seq, id;
	char *name, *comment, *seq, *qual, *sam;
	int8_t l_name, l_comment;
	int16_t l_qual;
} bwahip_seq_t;

typedef struct {                 /* mem_opt_t, bwa.h:86-118 (168 bytes, mat at offset 136) */
	uint64_t max_mem_intv;
	int a, b;
	int o_del, e_del;
	int o_ins, e_ins;
	int pen_unpaired;
	int pen_clip5, pen_clip3;
	int w;
	int zdrop;
	int T;
	int flag;
	int min_seed_len;
	int min_chain_weight;
	int max_chain_extend;
	float split_factor;
	int split_width;
	int max_occ;
	int max_chain_gap;
	int n_threads;
	int chunk_size;
	float mask_level;
	float drop_ratio;
	float XA_drop_ratio;
	float mask_level_redun;
	float mapQ_coef_len;
	int mapQ_coef_fac;
	int max_ins;
	int max_matesw;
	int max_XA_hits, max_XA_hits_alt;
	int8_t mat[25];
} bwahip_opt_t;

#define BWAHIP_F_PE        0x2      /* MEM_F_* of bwa.h:70-81 */
#define BWAHIP_F_NOPAIRING 0x4
#define BWAHIP_F_ALL       0x8
#define BWAHIP_F_NO_MULTI  0x10
#define BWAHIP_F_NO_RESCUE 0x20
#define BWAHIP_F_REF_HDR   0x100
#define BWAHIP_F_SOFTCLIP  0x200
#define BWAHIP_F_SMARTPE   0x400
#define BWAHIP_F_PRIMARY5  0x800
#define BWAHIP_F_KEEP_SUPP_MAPQ 0x1000
#define BWAHIP_F_XB        0x2000

typedef struct {                 /* mem_alnreg_t, bwa.h:145-163 (88 bytes) */
	int64_t rb, re;
	uint64_t hash;
	float frac_rep;
	int qb, qe;
	int rid;
	int score;
	int truesc;
	int sub;
	int alt_sc;
	int csub;
	int sub_n;
	int w;
	int seedcov;
	int secondary;
	int secondary_all;
	int seedlen0;
	int n_comp:30, is_alt:2;
} bwahip_alnreg_t;

typedef struct { int n, m; bwahip_alnreg_t *a; } bwahip_alnreg_v;   /* mem_alnreg_v, bwa.h:165 */

typedef struct {                 /* mem_pestat_t, bwa.h:167-171 */
	int low, high;
	int failed;
	double avg, std;
} bwahip_pestat_t;

typedef struct { uint64_t x[3], info; } bwahip_intv_t;              /* bwtintv_t, bwt.h:62-64 */

/* ---- error codes -------------------------------------------------------- */
#define BWAHIP_OK          0
#define BWAHIP_EINVAL     -1   /* bad argument */
#define BWAHIP_ENODEV     -2   /* no usable HIP device / HIP runtime error (message on stderr) */
#define BWAHIP_ENOMEM     -3   /* device or host allocation failed */
#define BWAHIP_EIO        -4   /* index files unreadable / inconsistent */
#define BWAHIP_ECAPACITY  -5   /* a read exceeds the compiled limits (length > BWAHIP_MAX_READ_LEN) */
#define BWAHIP_EINTERNAL  -6   /* a kernel reported an inconsistency (never expected) */

/* Longest read the kernels accept (LDS sizing of the per-read kernels).  mem_flt_chained_seeds (bwamem.c:605) runs on the GPU
 * (k_seed_sw): with the default -W 0 it is active only from ~730 bp, but a caller's -W (opt->min_chain_weight) switches it on
 * for every read of at least 22*W bases. */
#define BWAHIP_MAX_READ_LEN 700

typedef struct bwahip_ctx bwahip_ctx;

/* ---- reading FASTA/FASTQ (plain, gzip or bgzip) into batches: bseq_read (bwa.c:191) / kseq_read (kseq.h:176) -------------
 * A parallel pipeline per input file reads ahead of the caller (csrc/fastq_reader.cpp): plain files are mmap()ed and parsed in
 * chunks by n_threads workers, gzip streams are inflated on their own thread with the parse workers behind it, BGZF (bgzip)
 * members are inflated by the workers in parallel; anything that is not plain four-line FASTQ goes through an exact, sequential
 * restatement of kseq_read.  path2 != NULL: the mates' file, batches come interleaved (read i of file 1, read i of file 2);
 * "-" = stdin.  n_threads <= 0: BWAHIP_READER_THREADS or half of the host's cores (at most 8). */
typedef struct bwahip_fastq bwahip_fastq;
typedef struct bwahip_fastq_batch bwahip_fastq_batch;
int  bwahip_fastq_open(const char *path1, const char *path2, bwahip_fastq **out);
int  bwahip_fastq_open_mt(const char *path1, const char *path2, int n_threads, bwahip_fastq **out);
/* Next batch: reads until it holds at least chunk_bases bases and an even number of reads (bwa.c:216; `bwa mem -K`).  *n = 0 at
 * the end of the input.  name/comment/seq/qual of (*seqs)[i] point into the reader's memory and stay valid until the next call
 * or bwahip_fastq_close -- unlike bseq_read's they are NOT the caller's to free; seqs[i].sam (set by bwahip_process_seqs) is.
 * keep_comments = 0 drops FASTQ comments (stock behaviour without -C).  Names lose a trailing "/[0-9]" (bwa.c:73).
 * A damaged input (corrupt or truncated gzip data) returns BWAHIP_EIO -- the reference's err_gzread (utils.c:142) is fatal --
 * never a silently shortened batch. */
int  bwahip_fastq_next(bwahip_fastq *r, int64_t chunk_bases, int keep_comments, bwahip_seq_t **seqs, int *n);
/* The same batch as an owned object: it stays valid (with its strings) until bwahip_fastq_batch_release, independently of
 * later batches and of the reader, so that several batches can be in flight on several contexts.  *batch = NULL and *n = 0 at
 * the end of the input.  seqs may be NULL (bwahip_fastq_batch_seqs returns the array later). */
int  bwahip_fastq_next_batch(bwahip_fastq *r, int64_t chunk_bases, int keep_comments, bwahip_fastq_batch **batch, bwahip_seq_t **seqs, int *n);
bwahip_seq_t *bwahip_fastq_batch_seqs(bwahip_fastq_batch *b, int *n);
void bwahip_fastq_batch_release(bwahip_fastq_batch *b);
void bwahip_fastq_close(bwahip_fastq *r);

/* ---- lifetime ------------------------------------------------------------
 * bwahip_init replaces newProcess()/transferIndex() (cuda/streams.cu:8,164): it copies the three
 * index arrays (bwt, sa, pac) and the contig table into HBM of HIP device `device` and builds the
 * launch workspaces.  The context keeps its own host copy of the contig table (names included) and of the
 * packed reference; the caller's arrays are not referenced after it returns. */
int  bwahip_init(const bwahip_bwt_t *bwt, const bwahip_bns_t *bns, const uint8_t *pac, int device, bwahip_ctx **out);
/* Same, but bwt_dev->bwt, bwt_dev->sa and pac_dev already point into HBM of `device` (e.g. filled by an RCCL
 * broadcast from the rank that loaded the index); the device arrays stay owned by the caller and must outlive the
 * ctx.  bns is a host struct; the packed reference is read back once (l_pac/4+1 bytes) for host-side finalisation. */
int  bwahip_init_device(const bwahip_bwt_t *bwt_dev, const bwahip_bns_t *bns, const uint8_t *pac_dev, int device, bwahip_ctx **out);
/* One process per GPU on one node: rank 0 reads the index files, every rank receives the three index arrays and the contig
 * table over RCCL (xGMI) into its own HBM and gets a context on them -- what transferIndex() (cuda/streams.cu:8) does for
 * one GPU.  id128: a 128-byte ncclUniqueId made by bwahip_rccl_unique_id() on one rank and handed to the others by the
 * caller's own means (MPI, a file, torch.distributed ...).  prefix is read on rank 0 only.  Collective: every rank calls it. */
int  bwahip_rccl_unique_id(void *id128);
int  bwahip_init_rccl(const char *prefix, int rank, int world, const void *id128, int device, bwahip_ctx **out);
/* A further context on the same GPU sharing src's index arrays in HBM (no device copy; src must outlive it).  Contexts are
 * independent otherwise (own streams and batch buffers): two of them, each driven by its own host thread and taking batches in
 * turn, overlap one batch's latency-bound kernels with the other's throughput-bound ones. */
int  bwahip_ctx_clone(bwahip_ctx *src, bwahip_ctx **out);
/* A context on another GPU of the node: the three index arrays are copied device to device (hipMemcpyPeer: over xGMI where the
 * GPUs are linked, no second pass over the files or the host copy) into HBM the new context owns; it is independent of src
 * afterwards.  device == src's device: the same as bwahip_ctx_clone. */
int  bwahip_ctx_clone_on(bwahip_ctx *src, int device, bwahip_ctx **out);
int  bwahip_device_count(void);              /* HIP devices visible to the process (0 when there is none) */
/* Convenience: read a stock `bwa index` file set <prefix>.{bwt,sa,pac,ann,amb[,alt]} (bwa.c:402 bwa_idx_load) and init. */
int  bwahip_init_from_files(const char *prefix, int device, bwahip_ctx **out);
void bwahip_destroy(bwahip_ctx *ctx);
/* Host copies of the loaded index (valid until destroy); lets a caller that used
 * bwahip_init_from_files get at contig names etc. without loading the index twice. */
const bwahip_bns_t *bwahip_bns(const bwahip_ctx *ctx);
const bwahip_bwt_t *bwahip_bwt(const bwahip_ctx *ctx);
const uint8_t      *bwahip_pac(const bwahip_ctx *ctx);
/* Read-group id printed as RG:Z:<id> on every record (the reference's global bwa_rg_id, bwa.c:44, set by -R); NULL or
 * "" = none. */
int bwahip_ctx_set_rg_id(bwahip_ctx *ctx, const char *id);
const char *bwahip_ctx_rg_id(const bwahip_ctx *ctx);
void bwahip_opt_init(bwahip_opt_t *opt);     /* mem_opt_init defaults, bwamem.c:74 */
void bwahip_opt_fill_scmat(bwahip_opt_t *opt);   /* bwa_fill_scmat(opt->a, opt->b, opt->mat), bwa.c:249: call after changing a or b */

/* ---- the hot path ---------------------------------------------------------
 * bwahip_align_batch == kt_for(worker1) of mem_process_seqs (bwamem.c:1232): for every read i it
 * produces exactly the mem_alnreg_v that mem_align1_core (bwamem.c:1061) returns, computed on the
 * GPU.  seqs[i].seq is converted in place to 0..4 codes as the reference does (bwamem.c:1067).
 * regs_out[i].a is malloc()ed for the caller (free() it), regs_out[i].n == regs_out[i].m. */
int bwahip_align_batch(bwahip_ctx *ctx, const bwahip_opt_t *opt, int n, bwahip_seq_t *seqs, bwahip_alnreg_v *regs_out);

/* bwahip_process_seqs == mem_process_seqs (bwamem.h:69): hot path on the GPU, then the per-read
 * finalisation (mark primary, mapQ, CIGAR/NM/MD, SAM text; PE: insert-size stats, mate rescue,
 * pairing) with opt->n_threads host threads.  seqs[i].sam is malloc()ed, NUL terminated. */
int bwahip_process_seqs(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0);
/* The same work with the batch's SAM in one piece, for a caller whose output step is a single fwrite: *sam = NUL-terminated text
 * of the whole batch in read order (*sam_len bytes), *off (may be NULL) = n + 1 offsets with read i's records at sam[off[i]..off[i+1]).
 * Both point into the context; seqs[i].sam is left NULL (no malloc per read).  *off stays valid until the next call on the context,
 * *sam until the next-but-one (the context alternates between two pinned buffers, so that a writer thread can still be busy with
 * batch k while batch k + 1 is processed). */
int  bwahip_process_seqs_text(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs,
                              const bwahip_pestat_t *pes0, const char **sam, int64_t *sam_len, const int64_t **off);

/* The same work with the batch as BAM records (SAM specification 4.2) encoded on the GPU: *bam = the records of all reads in read
 * order, concatenated -- no header, no compression (bwahip_bam_header and bwahip_bgzf_write make a file of them); *off: n + 1
 * offsets, read i's records are bam[off[i]..off[i+1]).  Buffers and lifetimes as for bwahip_process_seqs_text.  A record says what
 * the SAM line says: the same flags, positions, CIGAR (BAM's operation codes), tags in the same order; NM / AS / XS as the smallest
 * integer type that holds the value, pa as the single nearest to the printed "%.3f", the others as Z.  What a record cannot hold
 * is refused with BWAHIP_EINVAL (and a message naming the read) before anything is launched: a read name of 255 bytes or more,
 * and a comment (-C) whose tab-separated fields are not all XX:Z:<printable>, XX:A:<char> or XX:i:<integer in [-2^31, 2^32)>. */
int  bwahip_process_seqs_bam(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs,
                             const bwahip_pestat_t *pes0, const uint8_t **bam, int64_t *bam_len, const int64_t **off);

/* bwahip_process_seqs_bam with the records leaving the GPU compressed: *bgzf = BGZF members (SAM specification 4.1) of the batch's
 * records, deflated and checksummed on the GPU (csrc/k_bgzf.hip), concatenated in order -- the records are cut every 65 280 bytes
 * exactly as bwahip_bgzf_write cuts them, regardless of record boundaries; no file header, no end-of-file block.  *raw_len = the
 * bytes of the records, *n_blocks = the number of members.  Buffers, lifetimes and refusals as for bwahip_process_seqs_bam.  The
 * same input gives the same bytes on every run and every context. */
int  bwahip_process_seqs_bgzf(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs,
                              const bwahip_pestat_t *pes0, const uint8_t **bgzf, int64_t *bgzf_len, int64_t *raw_len, int64_t *n_blocks);

/* ---- BAM file pieces that need no device -----------------------------------------------------------------------------------
 * bwahip_bam_header: magic, l_text + text, n_ref, names and lengths in a malloc()ed buffer (free() it).  The text is what
 * bwa_print_sam_hdr (bwa.c:520) writes for bns and hdr_line: one @SQ line per contig (AH:* for ALT contigs) unless hdr_line
 * (may be NULL) brings @SQ lines of its own, then hdr_line and a newline.  A @PG line is the caller's to put into hdr_line.
 * bwahip_bgzf_write: data as BGZF blocks (at most 65 280 input bytes each) on fd (< 0: produced and dropped), deflated by
 * n_threads workers and written in order -- the bytes do not depend on n_threads.  level 0: stored, 1..9: zlib's levels.
 * bwahip_bgzf_eof: the 28-byte end-of-file block.  A BAM file = bgzf(header) bgzf(records)... eof. */
int  bwahip_bam_header(const bwahip_bns_t *bns, const char *hdr_line, uint8_t **out, int64_t *len);
int  bwahip_bgzf_write(int fd, const void *data, int64_t len, int level, int n_threads);
int  bwahip_bgzf_eof(int fd);

/* ---- the batch driver: FASTQ files in -> SAM text out -------------------------------------------------------------------
 * What superBatchMain(ktp_aux_t*) (cuda/superbatch_process.h:35, superbatch_process.cpp:133: read || process, double buffered,
 * one GPU) and process()/kt_pipeline (fastmap.c:46,307: bseq_read -> mem_process_seqs -> fputs) are in the reference, for any
 * number of contexts: one reader (bwahip_fastq_*), one host thread per context taking whole batches with their true
 * n_processed, one writer emitting the SAM text in input order to out_fd (< 0: the text is produced and dropped).  ctxs: n_ctx
 * contexts -- on different devices (bwahip_ctx_clone_on), or several on one device (bwahip_ctx_clone; two per device overlap one
 * batch's serial tails with the other's kernels).  fq2 != NULL: paired-end (MEM_F_PE is set).  opt->n_threads is the host-thread
 * budget of the run for batch staging (divided among the contexts).  Fill the first four fields of *st (0 = defaults); the rest
 * is written on return.  The SAM header is the caller's (bwa_print_sam_hdr, bwa.c:520).  Returns the first error of any stage. */
typedef struct {
	int64_t chunk_bases;      /* in: bases per batch, bwa mem -K (actual_chunk_size, fastmap.c:304); <= 0: opt->chunk_size * opt->n_threads */
	int64_t max_reads;        /* in: > 0: stop at the first batch boundary at or after this many reads */
	int keep_comments;        /* in: -C */
	int reader_threads;       /* in: parse threads of the reader; <= 0: default */
	int64_t n_reads, n_batches, sam_bytes;   /* out */
	double seconds;           /* out: the call (opening the files) -> last SAM byte written */
	double reader_wait_s;     /* out: summed over the contexts: time their stage-in threads spent waiting for the reader */
	double gpu_busy_s;        /* out: summed over the contexts: time in the compute stage (hot path and finalisation queued and their
	                           * size read-backs awaited; staging and the copies run beside it and are not counted) */
	double write_s;           /* out: time the writer spent in write() */
} bwahip_stream_t;
int bwahip_stream_run(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                      const char *fq1, const char *fq2, int out_fd, bwahip_stream_t *st);

/* bwahip_stream_run with a BAM file as the output: the header (bwahip_bam_header of the contexts' index and hdr_line) first, every
 * batch's records (bwahip_process_seqs_bam) through the BGZF writer in input order, the end-of-file block last; out_fd < 0:
 * produced, deflated and dropped.  st as above, with sam_bytes = the uncompressed bytes of the records (header excluded) and
 * write_s = deflate + write().  Of opt->n_threads, half deflate and the other half stage the batches. */
int bwahip_stream_run_bam(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                          const char *fq1, const char *fq2, int out_fd, const char *hdr_line, int level, bwahip_stream_t *st);

/* bwahip_stream_run_bam with the BGZF blocks of the records made on the GPU: the same three-stage pipeline per context with the
 * deflate stage queued behind the BAM write pass, so what comes back from a context is a batch's finished members (about a quarter
 * of the bytes) and the writer only write()s them in input order.  The header goes through bwahip_bgzf_write at level 1, the
 * end-of-file block last.  There are no deflate workers: all of opt->n_threads stage the batches.  st as for bwahip_stream_run_bam
 * (sam_bytes = the uncompressed bytes of the records); *bs is written on return: raw_bytes (= st->sam_bytes), bgzf_bytes = the
 * members' bytes (the file without header member and EOF block), members, members that left stored, and the GPU time of the deflate
 * stage summed over the batches.  The file's bytes do not depend on the number of contexts or on thread counts.  Coordinate-sorted
 * output is not offered here: its blocks are cut by the host merge (bwahip_stream_run_bam_sorted). */
typedef struct { int64_t raw_bytes, bgzf_bytes, n_blocks, n_stored; double deflate_ms; } bwahip_bgzf_stats_t;
int bwahip_stream_run_bam_dev(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                              const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_bgzf_stats_t *bs);

/* ---- coordinate-sorted BAM ---------------------------------------------------------------------------------------------------------
 * The order is `samtools sort`'s coordinate order with its ties made explicit:
 *   1. refID as an unsigned number: -1 (no reference) after every contig;
 *   2. pos, -1 first within a refID (only records without a reference have it);
 *   3. strand: forward before reverse (flag 0x10);
 *   4. input order: batch (run) number, then the record's ordinal within the batch's unsorted records -- the sort is stable.
 * An unmapped read with a mapped mate carries the mate's refID and pos (bwamem.c:842-845) and so sorts next to it.  Rules 1-3 are one
 * uint64_t whose unsigned order is that order -- part of the ABI, because callers merge on it:
 *     bit 0                        reverse strand
 *     bits 1 .. P                  pos + 1                         P = bit length of (longest contig of the index + 1)
 *     bits P + 1 .. P + R          refID, -1 mapped to n_seqs      R = bit length of n_seqs
 * and no bit above.  n_seqs and contig lengths are int32 (bntseq.h), so P <= 32, R <= 31 and the key fits 64 bits for any index.
 * bwahip_bam_sort_key is the host restatement (no device; a refID outside [0, n_seqs) counts as -1), bwahip_bam_sort_key_bits = 1 + P + R.
 *
 * bwahip_process_seqs_bam_sorted: bwahip_process_seqs_bam with the batch's records in that order, sorted on the GPU (csrc/k_bamsort.hip: a
 * record table, a stable radix sort of (key, ordinal) over the key bits that differ, one gather of the record bytes).  *keys: the n_rec
 * sorted keys; *rec_off: n_rec + 1 offsets, record i is bam[rec_off[i] .. rec_off[i+1]).  Buffers and lifetimes as for
 * bwahip_process_seqs_bam (*bam and *keys until the next-but-one call on the context, *rec_off likewise). */
int  bwahip_process_seqs_bam_sorted(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0,
                                    const uint8_t **bam, int64_t *bam_len, const uint64_t **keys, const int64_t **rec_off, int64_t *n_rec);
uint64_t bwahip_bam_sort_key(const bwahip_bns_t *bns, int32_t refID, int32_t pos, int reverse);
int  bwahip_bam_sort_key_bits(const bwahip_bns_t *bns);
/* the same for any index with n_seqs contigs whose longest has `longest` bases: the key depends on the contig table through these alone */
uint64_t bwahip_bam_sort_key_for(int32_t n_seqs, int32_t longest, int32_t refID, int32_t pos, int reverse);
int  bwahip_bam_sort_key_bits_for(int32_t n_seqs, int32_t longest);
/* bwahip_bam_header with "@HD\tVN:1.6\tSO:coordinate" as the first line of the text; a hdr_line that brings an @HD line of its own:
 * BWAHIP_EINVAL. */
int  bwahip_bam_header_sorted(const bwahip_bns_t *bns, const char *hdr_line, uint8_t **out, int64_t *len);

/* Device-free merger of sorted runs (one run = one batch of bwahip_process_seqs_bam_sorted, handed over with its keys and offsets; no
 * record is ever parsed).  open: runs stay in host memory while their total is within mem_budget bytes; from the first run that would
 * exceed it, every run goes to a file of its own under tmp_dir (NULL: $TMPDIR or /tmp; mem_budget <= 0: every run) -- raw records, keys
 * and offsets, uncompressed, private.  tmp_dir must be a directory files can be made in: BWAHIP_EIO otherwise.  add: thread-safe, copies
 * what it is given (the caller's buffers are free on return); a run_no given twice: BWAHIP_EINVAL; a failed or short write: BWAHIP_EIO.
 * finish: k-way merge by (key, run_no, position in the run) into BGZF blocks on fd (< 0: produced and dropped) -- no header, no EOF
 * block; spilled runs are read through bounded windows and the output is deflated in pieces, so the whole is never in memory; the bytes
 * are those of one bwahip_bgzf_write over all records in order, whatever the budget and however the records were cut into runs.
 * A spilled run's file is open only while one of its windows
 * is filled, so the number of runs is not bounded by the limit on open descriptors.
 * close: frees everything and removes the files (also those of runs whose add failed half way). */
typedef struct bwahip_bam_merger bwahip_bam_merger;
int  bwahip_bam_merger_open(const char *tmp_dir, int64_t mem_budget, bwahip_bam_merger **m);
int  bwahip_bam_merger_add(bwahip_bam_merger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys, const int64_t *rec_off, int64_t n_rec);
int  bwahip_bam_merger_finish(bwahip_bam_merger *m, int fd, int level, int n_threads);
int  bwahip_bam_merger_stats(bwahip_bam_merger *m, int64_t *n_records, int64_t *n_runs, int64_t *spilled_bytes, double *merge_s);   /* any pointer may be NULL */
void bwahip_bam_merger_close(bwahip_bam_merger *m);

/* bwahip_stream_run_bam with a coordinate-sorted file as the output.  The pipeline per context is the same (stager, compute, drainer);
 * every batch leaves its context sorted and is handed to a merger with its batch number as the run number; after the last batch the
 * header (bwahip_bam_header_sorted), the merge and the EOF block are written.  The bytes do not depend on the number of contexts, on
 * which context took a batch, on mem_budget or on thread counts.  st as for bwahip_stream_run_bam (seconds: to the last byte written;
 * write_s includes the merge).  so: fill tmp_dir and mem_budget (see bwahip_bam_merger_open); the rest is written on return: records and
 * runs merged, bytes that went through tmp_dir, sort_ms = GPU time of the sort stage summed over the batches, merge_s = the merge
 * (deflate and write included).  On failure of any stage every thread ends and the temporary files are gone. */
typedef struct {
	const char *tmp_dir; int64_t mem_budget;                                    /* in */
	int64_t n_records, n_runs, spilled_bytes; double sort_ms, merge_s;         /* out */
} bwahip_sort_t;
int bwahip_stream_run_bam_sorted(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0, const char *fq1, const char *fq2,
                                 int out_fd, const char *hdr_line, int level, bwahip_stream_t *st, bwahip_sort_t *so);

/* Merger of sorted runs that stay in HBM (csrc/k_bammerge.hip): the same contract as bwahip_bam_merger_* -- no record is parsed, a run is
 * bytes + sorted keys + n_rec + 1 offsets, the order is (key, run_no, position in the run) over all 64 bits of the key -- with the merge,
 * the gather and the deflate on the context's device.  open: piece_blocks = BGZF blocks gathered and deflated at a time (1 .. 4096;
 * <= 0: the context's "sorted_piece_blocks", bwahip_ctx_tune).  add: host pointers, uploaded into device buffers of the run's own (the
 * caller's are free on return); thread-safe; a run_no given twice, offsets that do not start at 0, end at len and never decrease:
 * BWAHIP_EINVAL; more than 2^31 - 1 records in total (or one record of 2^31 bytes or more): BWAHIP_ECAPACITY; a failed allocation:
 * BWAHIP_ENOMEM -- after any refused add the merger holds what it held before and stays usable.  finish: one stable radix sort of all keys
 * in (run_no, position) order, then pieces of piece_blocks x 65 280 bytes of the sorted byte stream are gathered from the runs and
 * deflated (k_bgzf.hip) while the members of the piece before travel to the host and are written to fd (< 0: produced and dropped) -- no
 * header, no EOF block.  The members are those of one deflate stage over all records in order (bwahip_kat_bgzf of the sorted
 * concatenation), whatever piece_blocks, however the records were cut into runs and in whichever order the runs were added.  *st (may be
 * NULL): records, runs, bytes of the records, of the members, members, members that left stored, HBM held at the end of finish (runs
 * and working set), GPU time of the sort, the gathers and the deflate stages, and the seconds finish took.  finish runs on the
 * context's streams: no other call on the context meanwhile.  close (before the context is destroyed) frees everything. */
typedef struct bwahip_bam_devmerger bwahip_bam_devmerger;
typedef struct { int64_t n_records, n_runs, raw_bytes, bgzf_bytes, n_blocks, n_stored, hbm_bytes; double sort_ms, gather_ms, deflate_ms, finish_s; } bwahip_devmerge_stats_t;
int  bwahip_bam_devmerger_open(bwahip_ctx *ctx, int piece_blocks, bwahip_bam_devmerger **m);
int  bwahip_bam_devmerger_add(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys, const int64_t *rec_off, int64_t n_rec);
int  bwahip_bam_devmerger_finish(bwahip_bam_devmerger *m, int fd, bwahip_devmerge_stats_t *st);
void bwahip_bam_devmerger_close(bwahip_bam_devmerger *m);
/* HBM a device merger takes for runs of raw_bytes bytes and n_records records in all, finish included (no device is touched): the
 * runs (raw_bytes + 16 per record + 8 per run), and as working set, counted with the eighth of slack its buffers grow with: the sort's
 * and the source table's 48 bytes per record, two piece inputs, two piece outputs and the deflate stage's slots (4 x 65 280 + 2 x 31 +
 * 65 536 + 12 bytes per block of a piece, a piece no longer than the records), and 64 MiB for the deflate stage's per-workgroup words.
 * An argument < 0 or piece_blocks outside 1 .. 4096: -1. */
int64_t bwahip_bam_devmerge_hbm_need(int64_t raw_bytes, int64_t n_records, int64_t n_runs, int piece_blocks);

/* bwahip_stream_run_bam_sorted with the runs kept in HBM and merged, gathered and deflated there after the last batch
 * (bwahip_bam_devmerger_* on ctxs[0]): nothing of a batch travels to the host before the end, and what travels then is BGZF members.
 * All contexts must be on one device (BWAHIP_EINVAL otherwise, before anything starts).  The header goes through bwahip_bgzf_write at
 * level 1; the records' members are bwahip_kat_bgzf of the sorted records.  sd in: hbm_budget = bytes of HBM the runs and the finish may
 * take (bwahip_bam_devmerge_hbm_need of the runs so far, taken in input order; 0: half of the device's free memory when the run
 * starts), piece_blocks as for bwahip_bam_devmerger_open; tmp_dir, mem_budget and level belong to the host merger and are used only after
 * a fall-back: when run k would exceed hbm_budget (or its device buffers cannot be allocated), the runs held so far are downloaded into a
 * host merger in run order, every later run is downloaded as bwahip_stream_run_bam_sorted does, and the file is exactly that entry
 * point's at `level` (fell_back = 1, fell_back_at_run = k, dev all zero; a tmp_dir that cannot be used: BWAHIP_EIO then, not before).
 * sd out: n_records, n_runs, spilled_bytes, sort_ms (the batches' sorts), merge_s (the finish, device or host) as bwahip_sort_t. */
typedef struct {
	const char *tmp_dir; int64_t mem_budget; int level;                         /* in: the host merger after a fall-back */
	int64_t hbm_budget; int piece_blocks;                                       /* in */
	int fell_back; int64_t fell_back_at_run;                                    /* out */
	int64_t n_records, n_runs, spilled_bytes; double sort_ms, merge_s;         /* out */
	bwahip_devmerge_stats_t dev;                                                /* out */
} bwahip_sort_dev_t;
int bwahip_stream_run_bam_sorted_dev(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0, const char *fq1, const char *fq2,
                                     int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd);

/* ---- the BAI index beside a coordinate-sorted file (SAM specification 5.2; csrc/bai_host.cpp, csrc/k_bai.hip) ----
 * The canonical form every path here writes, byte for byte.  Virtual offsets: the record stream is cut every 65 280 bytes into members
 * 0 .. B - 1 at file offsets c[b]; V(u) = c[u / 65280] << 16 | u % 65280, and V(total) = c[B] << 16, where the end-of-file block goes;
 * record i spans [V(u_i), V(u_i+1)).  Per record, read from its bytes: rlen = the lengths of its M D N = X operations, e = pos + rlen
 * when rlen > 0 and 0x4 is clear, else pos + 1; bin = reg2bin(pos, e), never the record's own field.  refID < 0: counted in n_no_coor
 * only.  A chunk is a maximal run of consecutive records of one (refID, bin); within a bin chunks are in file order and a chunk that
 * begins in the member in which its predecessor ends is joined to it; bins ascending, then pseudo-bin 37450 (first begin / last end,
 * records with 0x4 clear / set); a reference without records: n_bin = 0, n_intv = 0.  Linear index: n_intv = 1 + the largest
 * (e - 1) >> 14, a window holds the smallest begin over the records that overlap it, an empty one the value of the next to its right.
 * Sparse bins are not moved into their parents, and there is no CSI form.  Any reader that follows the specification can use the index;
 * that its bytes are those of another writer is not claimed.
 * Refused, before a byte of the index is written, with the code of the first offending record in file order: BWAHIP_EINVAL for a record
 * shorter than 36 bytes, whose block_size + 4 is not its length, whose name and CIGAR (36 + l_read_name + 4 x n_cigar_op) exceed it, with
 * refID >= n_ref or refID >= 0 and pos < 0, or that comes before its predecessor (refID as unsigned, then pos); BWAHIP_ECAPACITY for
 * e > 2^29.  No byte outside a record is read to find that out.
 *
 * Device-free builder.  open: n_ref references, the file offset of the first member of the records.  add_records: whole records in file
 * order, record i is rec[rec_off[i] .. rec_off[i+1]); add_members: the lengths of the next members in file order (1 .. 65 536 each).
 * The two may be called in any interleaving; what is held is proportional to the chunks, the windows and the records whose members
 * are not known yet, not to the records.  finish: members that are not exactly those of the records' bytes: BWAHIP_EINVAL; the index on
 * bai_fd (< 0: built and dropped).  After a refusal every later call returns the same code. */
typedef struct bwahip_bai_builder bwahip_bai_builder;
int  bwahip_bai_builder_open(int32_t n_ref, int64_t first_member_offset, bwahip_bai_builder **b);
int  bwahip_bai_builder_add_records(bwahip_bai_builder *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec);
int  bwahip_bai_builder_add_members(bwahip_bai_builder *b, const int32_t *member_len, int64_t n);
int  bwahip_bai_builder_finish(bwahip_bai_builder *b, int bai_fd);
void bwahip_bai_builder_close(bwahip_bai_builder *b);
/* BWAHIP_ECAPACITY for a contig table with a contig longer than 2^29 bases: BAI cannot index it (no device is touched) */
int  bwahip_bai_check_contigs(const bwahip_bns_t *bns);
/* bwahip_bgzf_write that also returns the length of every member it wrote, in file order (the same bytes on fd).  member_len has room
 * for cap lengths: fewer than the (len + 65 279) / 65 280 members: BWAHIP_ECAPACITY, nothing is written. */
int  bwahip_bgzf_write_lens(int fd, const void *data, int64_t len, int level, int n_threads, int32_t *member_len, int64_t cap, int64_t *n_members);
/* bwahip_bam_merger_finish with the index: the builder is fed every record as it is emitted and the lengths of the members as each
 * piece leaves the writer; the bytes on fd are bwahip_bam_merger_finish's.  The caller opens, finishes and closes the builder. */
int  bwahip_bam_merger_finish_bai(bwahip_bam_merger *m, int fd, int level, int n_threads, bwahip_bai_builder *builder);

/* The index stage on the device (csrc/k_bai.hip).  bwahip_bam_devmerger_finish_bai: bwahip_bam_devmerger_finish (the same members on
 * fd) and, after the last piece, the index of the sorted records on bai_fd (< 0: built and dropped): the records are parsed where the
 * runs lie, the members' lengths were kept as each piece was deflated; what travels to the host is the compact tables.  n_ref and
 * first_member_offset as for the builder.  A refusal (above) comes after the members were written and before any byte of the index.
 * *bs (may be NULL): chunks and linear-index windows written, records without a reference, bytes of the index, HBM the stage held
 * beside the merger's, GPU time of the stage.
 * bwahip_kat_bai: exactly that stage on the caller's records (host pointers; record i = rec[rec_off[i] .. rec_off[i+1]), in file
 * order) and the caller's member lengths, no deflate; the index into out (out_cap too small: BWAHIP_ECAPACITY, *out_len says what it
 * takes); n_members other than the (bytes + 65 279) / 65 280 of the records: BWAHIP_EINVAL.
 * bwahip_bam_devmerge_bai_hbm_need: the HBM the stage takes beside bwahip_bam_devmerge_hbm_need, with the eighth of slack its buffers
 * grow with: 29 bytes per record and, for at most as many chunks, 52 each; 12 per member; 56 per reference (first and last record,
 * window and 0x4 counts, the linear index's offset, 32 of metadata); 16 per window of the linear index (no device is touched; an
 * argument < 0: -1). */
typedef struct { int64_t n_chunks, n_windows, n_no_coor, bai_bytes, hbm_bytes; double index_ms; } bwahip_bai_stats_t;
int  bwahip_bam_devmerger_finish_bai(bwahip_bam_devmerger *m, int fd, int bai_fd, int64_t first_member_offset, int32_t n_ref, bwahip_devmerge_stats_t *st, bwahip_bai_stats_t *bs);
int  bwahip_kat_bai(bwahip_ctx *ctx, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, const int32_t *member_len, int64_t n_members, int64_t first_member_offset,
                    int32_t n_ref, uint8_t *out, int64_t out_cap, int64_t *out_len);
int64_t bwahip_bam_devmerge_bai_hbm_need(int64_t n_records, int64_t n_blocks, int64_t n_ref, int64_t n_windows);

/* bwahip_stream_run_bam_sorted and bwahip_stream_run_bam_sorted_dev with the index of the file on bai_fd (< 0: built and dropped); the
 * BAM file is the one the entry point without index writes.  An index whose longest contig exceeds 2^29 bases: BWAHIP_ECAPACITY before
 * anything starts.  The header goes through bwahip_bgzf_write_lens, so its members give the offset of the first member of the records.
 * Host-merged: a builder listens to the merge (bwahip_bam_merger_finish_bai).  Device-merged: hbm_budget counts
 * bwahip_bam_devmerge_hbm_need and bwahip_bam_devmerge_bai_hbm_need (windows: those of the contig table) together, the finish is
 * bwahip_bam_devmerger_finish_bai; after a fall-back the index comes from the host path.  On any failure the return code says so and
 * what may have reached bai_fd is not an index. */
int bwahip_stream_run_bam_sorted_bai(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0, const char *fq1, const char *fq2,
                                     int out_fd, const char *hdr_line, int level, bwahip_stream_t *st, bwahip_sort_t *so, int bai_fd);
int bwahip_stream_run_bam_sorted_dev_bai(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0, const char *fq1, const char *fq2,
                                         int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, int bai_fd);

/* ---- Duplicate marking of device-merged, coordinate-sorted BAM (csrc/k_markdup.hip), before the deflate ----
 * One canonical rule, recomputable from the records of the file alone.  Byte identity with samtools markdup or Picard is not claimed:
 * one library (read groups are ignored), no optical duplicates, no UMIs.
 *   Template        the records of one read (single end) or of one pair (reads 2i and 2i + 1 of a batch under BWAHIP_F_PE).
 *   Primary record  a read's record with flag & 0x900 == 0 (the first one, if there are several; a read without one counts as
 *                   unmapped); it is mapped when 0x4 is clear.
 *   u5              the unclipped 5' position of a mapped primary record, with rlen = the lengths of its M D N = X operations:
 *                   forward strand pos - (lengths of the leading S/H operations); reverse strand (0x10) pos + max(rlen, 1) - 1 +
 *                   (lengths of the trailing S/H operations); taken as int32.
 *   End word        (uint64)refID << 33 | (uint64)(u5 + 2^31) << 1 | reverse  -- bwahip_dup_end_word, on the host, no device.
 *   Score           of a record: the sum of its quality bytes that are >= 15, 0 when the first quality byte is 0xff (no qualities);
 *                   of a template: the sum over its mapped primary records, as uint32.
 *   Kind            2 (pair): both primaries mapped; 1 (fragment): exactly one (a single-end read, or a pair with one end unmapped);
 *                   0: none.
 *   Signature       of a pair: its two end words, the smaller first; of a fragment: its one end word.
 *   Input order     (run number, template index within the run).
 *   Decision        among pairs of equal signature the one with the highest score is kept, equal scores keep the earliest in input
 *                   order, the rest are duplicates.  A fragment is a duplicate if any pair has the fragment's end word as one of its
 *                   two; otherwise, among the fragments with that end word the best is kept (score, then input order), the rest
 *                   are duplicates.
 *   Marking         every record of a duplicate template that has 0x4 clear gets 0x400 -- primary, secondary and supplementary.
 *                   Nothing else changes: sort order, record offsets and byte counts are those of the unmarked run.
 * A template's descriptor: pair end[0] <= end[1]; fragment end[1] = 0; kind 0: all fields zero. */
typedef struct { uint64_t end[2]; uint32_t score; uint32_t kind; } bwahip_dup_desc_t;   /* 24 bytes */
typedef struct {
	int64_t n_templates[3], n_dup_templates[3];   /* by kind 0, 1, 2 (kind 0 is never a duplicate) */
	int64_t n_marked;                             /* records that got 0x400 */
	int64_t hbm_bytes;                            /* what the stage held: its own buffers, the concatenated descriptors, the runs' tmpl / desc */
	double markdup_ms, decide_ms, mark_ms;        /* GPU time of the stage by HIP events: all of it; the decision (with the descriptors' concatenation); the counts and the marking pass */
} bwahip_markdup_stats_t;
uint64_t bwahip_dup_end_word(int32_t refID, int32_t u5, int reverse);
/* The decision restated on the host (csrc/markdup_host.cpp, no HIP): dup_out[i] = 1 for a duplicate template, else 0; input order = index. */
int  bwahip_markdup_decide_host(const bwahip_dup_desc_t *desc, int64_t n_tmpl, uint8_t *dup_out);
/* bwahip_process_seqs_bam_sorted, and per record (in sorted order, beside keys and offsets) the index of its template in the batch,
 * and per template (n / 2 under BWAHIP_F_PE, else n) its descriptor -- made on the GPU while the batch still knows its mates.  Same
 * buffers and lifetimes. */
int  bwahip_process_seqs_bam_sorted_dup(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, bwahip_seq_t *seqs, const bwahip_pestat_t *pes0,
                                        const uint8_t **bam, int64_t *bam_len, const uint64_t **keys, const int64_t **rec_off, int64_t *n_rec,
                                        const uint32_t **tmpl, const bwahip_dup_desc_t **desc, int64_t *n_tmpl);
/* bwahip_bam_devmerger_add with the run's template indices (one per record) and descriptors (one per template); additionally refuses a
 * tmpl[i] >= n_tmpl with BWAHIP_EINVAL; after a refusal the merger is as before.
 * bwahip_bam_devmerger_finish_markdup: the decision over the templates of all runs (input order = run number, then index) and the marking
 * pass over the runs' records in HBM, then bwahip_bam_devmerger_finish (n_ref < 0: no index, bai_fd is not looked at) or
 * bwahip_bam_devmerger_finish_bai (n_ref >= 0, bai_fd as there).  A merger that holds a run added without descriptors: BWAHIP_EINVAL
 * before a byte is written.  The runs stay marked: a second finish writes the same bytes.  ms may be NULL. */
int  bwahip_bam_devmerger_add_dup(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys, const int64_t *rec_off, int64_t n_rec,
                                  const uint32_t *tmpl, const bwahip_dup_desc_t *desc, int64_t n_tmpl);
int  bwahip_bam_devmerger_finish_markdup(bwahip_bam_devmerger *m, int fd, int bai_fd, int64_t first_member_offset, int32_t n_ref, bwahip_devmerge_stats_t *st,
                                         bwahip_bai_stats_t *bs, bwahip_markdup_stats_t *ms);
/* The HBM marking adds to bwahip_bam_devmerge_hbm_need (no device; -1 for a negative argument), term by term:
 *   the runs     4 bytes per record (tmpl) and 24 per template (desc), allocated to size;
 *   the stage    per template 115 bytes: the descriptors of all runs concatenated (24); the verdict (1); and for the two entries a
 *                template has in the end-word table 45 each -- the two key and two ordinal buffers of the sort, should they have to
 *                grow beyond what the merge itself takes (8 + 8 + 4 + 4), the segment head (4), its scan (8), the segment's best
 *                (8), "a pair is here" (1); plus 4096 for the counters and the scan's last element; grown with an eighth of slack
 *                (DevBuf::ensure).  The sort's histograms are within the 64 MiB bwahip_bam_devmerge_hbm_need counts. */
int64_t bwahip_bam_devmerge_markdup_hbm_need(int64_t n_records, int64_t n_templates);
/* bwahip_stream_run_bam_sorted_dev_bai with marking: every batch leaves its context with tmpl and descriptors, handed device to device to
 * the merger as the records are; the finish is bwahip_bam_devmerger_finish_markdup.  bai_fd < 0: no index is built.  hbm_budget counts
 * bwahip_bam_devmerge_hbm_need, _bai_hbm_need (with an index) and _markdup_hbm_need together.  The file does not depend on the number of
 * contexts, on which context took a batch, or on piece_blocks.  There is NO host fall-back here: when a run does not fit the budget, or
 * its buffers cannot be allocated, the call returns BWAHIP_ECAPACITY and what reached out_fd is not a file; sd->tmp_dir, mem_budget and
 * level are ignored. */
int  bwahip_stream_run_bam_sorted_dev_markdup(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0, const char *fq1, const char *fq2,
                                              int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, int bai_fd, bwahip_markdup_stats_t *ms);
/* Known answers.  bwahip_kat_dup_desc: exactly the batch kernel on the caller's records in input order -- read i's records are
 * rec[off[i] .. off[i+1]) (host pointers, off[0] >= 0, rec holds off[n_reads] bytes); paired: reads 2i and 2i + 1 are one template;
 * desc_out receives n_reads (or n_reads / 2) descriptors.  A record that does not chain, or whose name + CIGAR + sequence + qualities
 * exceed its length: BWAHIP_EINVAL, and no byte outside a record is read.
 * bwahip_kat_markdup: exactly the decision stage on the caller's descriptors, one byte per template; n_tmpl == 0 launches nothing. */
int  bwahip_kat_dup_desc(bwahip_ctx *ctx, const uint8_t *rec, const int64_t *off, int64_t n_reads, int paired, bwahip_dup_desc_t *desc_out);
int  bwahip_kat_markdup(bwahip_ctx *ctx, const bwahip_dup_desc_t *desc, int64_t n_tmpl, uint8_t *dup_out);
float bwahip_kat_dup_desc_ms(bwahip_ctx *ctx);   /* the kernel's milliseconds in the last bwahip_kat_dup_desc, by HIP events (scripts/markdup_rate.py) */
/* Test instrumentation: what the library owns in this process right now -- out[0] device buffers, [1] their bytes, [2] pinned host
 * buffers, [3] their bytes, [4] HIP events, [5] HIP streams.  Memory of the caller's that a context reads (bwahip_init_device,
 * bwahip_batch_attach) does not count.  After the last context and merger are gone the figures are those from before the first. */
int  bwahip_live_resources(int64_t out[6]);

/* ---- Alignment QC summary and depth of coverage of coordinate-sorted BAM (csrc/k_qc.hip on the device, csrc/qc_host.cpp without one) ----
 * One canonical summary, recomputable from the records of the file and the contig lengths alone.  All values are integers.  The result
 * does not depend on the order of the records, on how they are cut into runs or calls, or on the order in which wavefronts run.
 * Equality with the output of samtools flagstat, samtools idxstats or mosdepth is not claimed; the categories are theirs as restated here.
 *   Options         window_shift in [4, 29], 0 means 14 (BAI's linear window); exclude_flags in [0, 65535], < 0 means 1796
 *                   (0x4 | 0x100 | 0x200 | 0x400); min_mapq in [0, 255].  Anything else: BWAHIP_EINVAL before anything is launched.
 *                   The file holds them as resolved.
 *   Per record      every field is bounded by the record's length first.  BWAHIP_EINVAL: a record shorter than 36 bytes; a
 *                   block_size + 4 that is not its length; 36 + l_read_name + 4 * n_cigar_op beyond it; refID >= n_ref; refID >= 0 with
 *                   pos < 0.  The first offending record in the order given decides.  No byte outside a record is read, and of a record
 *                   only its first 36 bytes and its CIGAR.
 *   Counts          count[q][16], q = (flag & 0x200) != 0: [0] total; [1] primary (flag & 0x900 == 0); [2] secondary (0x100);
 *                   [3] supplementary (0x800 without 0x100); [4] duplicates (0x400); [5] primary duplicates; [6] mapped (0x4 clear);
 *                   [7] primary mapped.  [8..15] count primary records with 0x1 only: [8] paired; [9] read1 (0x40); [10] read2 (0x80);
 *                   [11] properly paired (0x2 set, 0x4 clear); [12] itself and mate mapped (0x4 and 0x8 clear); [13] singletons (0x4
 *                   clear, 0x8 set); [14] of [12], next_refID != refID; [15] of [14], mapq >= 5.
 *                   n_no_coor: the records with refID < 0.
 *   Per reference   mapped: the records with that refID and 0x4 clear; placed_unmapped: the same with 0x4 set.
 *   Histograms      mapq_hist[256] over primary mapped records; isize_hist[1025] over primary records with 0x1 and 0x2 set, 0x4 and
 *                   0x8 clear and tlen > 0, bin min(tlen, 1024).
 *   Coverage        a record takes part when refID >= 0, flag & exclude_flags == 0 and mapq >= min_mapq.  Each of its M, =, X and D
 *                   operations covers [p, p + len), p starting at pos and advancing over M D N = X; the interval is clipped to
 *                   [0, contig length); N covers nothing; overlapping mates both count.  depth(r, x) = the intervals over base x of
 *                   reference r.  Per reference: covered = bases of depth >= 1, depth_sum; per reference ceil(len / 2^window_shift)
 *                   windows, each the sum of depth over its bases (the last one short); depth_hist[256] over all bases of all
 *                   references, bin min(depth, 255).
 *   The file        little endian, no padding, 12 580 + 48 * n_ref + 8 * (windows of all references) bytes:
 *                     char[4] "BQC\1" | int32 n_ref | int32 window_shift, exclude_flags, min_mapq | uint64 n_no_coor |
 *                     uint64 count[2][16] | uint64 mapq_hist[256] | uint64 isize_hist[1025] | uint64 depth_hist[256] |
 *                     n_ref x { uint64 len, mapped, placed_unmapped, covered, depth_sum, n_windows } |
 *                     the windows of reference 0, 1, ... as uint64 each.
 * Device-free builder (csrc/qc_host.cpp).  open: the contig lengths (0 .. 2^31 - 1 each) and the options (NULL: all defaults).
 * add_records: whole records, record i is rec[rec_off[i] .. rec_off[i+1]), any cut into calls, any order.  finish: the summary on
 * qc_fd (< 0: built and dropped).  After a refusal every later call returns the same code.  It holds 4 bytes per base of every reference
 * that a record has covered (a difference array of len + 1 words, made at the reference's first covering record), 24 bytes per reference
 * and, during finish, 8 bytes per window. */
typedef struct { int window_shift, exclude_flags, min_mapq; } bwahip_qc_opt_t;
typedef struct {
	int64_t n_windows, qc_bytes;                  /* windows of all references; bytes of the summary */
	int64_t hbm_bytes;                            /* what the stage held (0 after a host fall-back) */
	double qc_ms, record_ms, scan_ms;             /* GPU time by HIP events: the stage (with the clearing of its tables and of the difference array); its record pass; its scan pass */
} bwahip_qc_stats_t;
typedef struct bwahip_qc_builder bwahip_qc_builder;
int  bwahip_qc_builder_open(int32_t n_ref, const int64_t *ref_len, const bwahip_qc_opt_t *opt, bwahip_qc_builder **b);
int  bwahip_qc_builder_add_records(bwahip_qc_builder *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec);
int  bwahip_qc_builder_finish(bwahip_qc_builder *b, int qc_fd);
void bwahip_qc_builder_close(bwahip_qc_builder *b);
/* The host merger with a listener: bwahip_bam_merger_finish and _finish_bai feed the builder every record as it is emitted (NULL: nobody
 * listens, as before); the bytes on fd do not change.  The caller opens, finishes and closes the builder. */
int  bwahip_bam_merger_set_qc(bwahip_bam_merger *m, bwahip_qc_builder *builder);
/* The stage on the device (csrc/k_qc.hip): one pass over the records where they lie (counts reduced per wavefront, histograms per
 * workgroup in LDS, +1 / -1 into a difference array of len + 1 slots per reference, each reference padded to whole tiles of 2048), then
 * a three-phase prefix sum over the array (tile sums, their scan, the tiles again) that feeds depth histogram, covered bases and
 * windows; the compact tables come back in one download and go through the host builder's serialiser.
 * bwahip_kat_qc: exactly that stage on the caller's records (host pointers, any order); the summary into out (out_cap too small:
 * BWAHIP_ECAPACITY, *out_len says what it takes).
 * bwahip_bam_devmerger_set_qc arms a device merger: every finish (_finish, _finish_bai, _finish_markdup) then runs the stage over the
 * runs after the marking, if there is any, and before the order is made, and writes the summary to qc_fd (< 0: built and dropped) once
 * the members are written.  A refusal comes before a byte of the members is written.  opt == NULL disarms (the other arguments are not
 * looked at); an unarmed merger queues what it queued before.  *qs (may be NULL) is filled by every armed finish.
 * bwahip_qc_hbm_need: the HBM the stage takes, with the eighth of slack its buffers grow with (no device; -1 for a negative argument):
 * with S = sum_len + 2048 * n_ref slots (len + 1 per reference, padded), 4 * S for the difference array, 16 * (S / 2048 + n_ref + 1)
 * for the tiles (sum, its scan, the tile's reference), 8 * (1570 + 3 * n_ref + n_windows) for the tables, 24 * (n_ref + 1) for length,
 * first tile and first window of every reference, 4096 for the error word and the scan's own sums.  Nothing is held per record. */
int  bwahip_kat_qc(bwahip_ctx *ctx, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, int32_t n_ref, const int64_t *ref_len, const bwahip_qc_opt_t *opt,
                   uint8_t *out, int64_t out_cap, int64_t *out_len);
int  bwahip_bam_devmerger_set_qc(bwahip_bam_devmerger *m, const bwahip_qc_opt_t *opt, int32_t n_ref, const int64_t *ref_len, int qc_fd, bwahip_qc_stats_t *qs);
int64_t bwahip_qc_hbm_need(int64_t n_ref, int64_t sum_len, int64_t n_windows, int64_t n_records);
/* bwahip_stream_run_bam_sorted_dev_markdup (markdup != 0: its file and rules, no fall-back) or bwahip_stream_run_bam_sorted_dev_bai
 * (markdup == 0: its file and rules; bai_fd < 0: the index is built and dropped) with the summary of the file on qc_fd.  The contig
 * lengths are those of the contexts' index.  hbm_budget counts bwahip_qc_hbm_need too.  After a fall-back the host builder listens to
 * the host merge and writes the same bytes.  qo == NULL: BWAHIP_EINVAL.  ms and qs may be NULL. */
int  bwahip_stream_run_bam_sorted_dev_qc(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0, const char *fq1, const char *fq2,
                                         int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, int bai_fd, bwahip_markdup_stats_t *ms,
                                         int markdup, const bwahip_qc_opt_t *qo, int qc_fd, bwahip_qc_stats_t *qs);

/* ---- Pileup of candidate variant sites of coordinate-sorted BAM (csrc/k_pileup.hip on the device, csrc/pileup_host.cpp without one) ----
 * Where the reads disagree with the reference, and how strongly: one canonical table, recomputable from the records of the file, the
 * contig lengths and the packed reference alone.  All values are integers.  The result does not depend on the order of the records, on
 * how they are cut into runs or calls, or on the order in which wavefronts run.  No indel is normalised or left-aligned.  Equality with
 * the output of samtools mpileup or bcftools is not claimed.
 *   Options         min_mapq in [0, 255]; min_baseq in [0, 93]; exclude_flags in [0, 65535], < 0 means 1796 (0x4 | 0x100 | 0x200 |
 *                   0x400); min_alt in [1, 65535], 0 means 2.  Anything else: BWAHIP_EINVAL before anything is launched.  The file holds
 *                   them as resolved.
 *   Reference       n_ref contigs of ref_len[r] bases (0 .. 2^31 - 1 each); contig r begins at base ref_off[r] = the sum of the earlier
 *                   lengths of the packed sequence, which has .pac's layout: 2 bits per base (A C G T = 0 1 2 3), base i in byte i >> 2
 *                   at shift (~i & 3) << 1; (sum of the lengths + 3) / 4 bytes are read.  A sum of 2^40 or more: BWAHIP_ECAPACITY.
 *                   Inside an ambiguity hole the reference base is whatever .pac holds there, as for the MD tag: there is no hole table.
 *   Per record      the checks of the QC summary above, and two more, both BWAHIP_EINVAL: l_seq < 0; 36 + l_read_name +
 *                   4 * n_cigar_op + (l_seq + 1) / 2 + l_seq beyond the record.  The first offending record in the order given decides.
 *                   No byte outside a record is read.
 *   Taking part     a record takes part when refID >= 0, flag & exclude_flags == 0, mapq >= min_mapq, l_seq > 0 and the query length
 *                   of its CIGAR (the lengths of M I S = X) equals l_seq.  Any other record contributes nothing and is not refused.
 *   Walk            p starts at pos, q at 0.  M = X advance both, I and S advance q, D and N advance p, H, P and the operation codes
 *                   9 .. 15 advance neither; an operation of length 0 gives nothing.  Base q is the BAM code in the high (q even) or
 *                   low nibble of seq[q >> 1].  A base passes when the record's first quality byte is 0xff or its own quality is >=
 *                   min_baseq.  Everything at a p outside [0, contig length) is dropped.
 *   Observations    kind 0, SNV: an M = X base that is one of A C G T (codes 1 2 4 8), passes and differs from the reference base; at
 *                           its own p; len 1, bases = the base as 0 .. 3.
 *                   kind 1, DEL: each D operation; at p = its first base; len = min(length, 2^21 - 1), bases 0.
 *                   kind 2, INS: each I operation whose bases are all A C G T (qualities are not looked at); at p = the reference base
 *                           that follows (dropped when that is the contig's end); len = min(length, 31), bases = its first
 *                           min(length, 8) bases at 2 bits each, the first base lowest.  Longer insertions that agree in these merge.
 *                   Bases other than A C G T are never evidence.  Each observation counts under the record's strand (flag & 0x10).
 *   Sites           an allele is a (refID, p, kind, len, bases) with fwd and rev observations; it is kept when fwd + rev >= min_alt.  A
 *                   site is a (refID, p) with at least one kept allele.  Per site: ref_base (0 .. 3); n_alleles, its kept alleles;
 *                   n_cov, the records taking part whose M = X or D operations cover p (overlapping mates both count); n_ref_fwd and
 *                   n_ref_rev, the M = X bases at p that are one of A C G T, pass and equal the reference base, by strand.
 *   The file        little endian, no padding, 64 + 28 * n_sites + 20 * n_alleles bytes.  Sites ascend by (refID, pos); the alleles
 *                   follow in site order and within a site ascend by (kind, len, bases):
 *                     char[4] "BPU\1" | int32 n_ref | int32 min_mapq, min_baseq, exclude_flags, min_alt | uint64 n_sites, n_alleles |
 *                     uint64 n_obs[3] (all observations by kind, before min_alt) |
 *                     n_sites x { int32 refID, pos; uint32 ref_base, n_alleles, n_cov, n_ref_fwd, n_ref_rev } |
 *                     n_alleles x { uint32 kind, len, bases, fwd, rev }.
 * Device-free builder (csrc/pileup_host.cpp): a judge and a library for small inputs, not wired into the host merger and no fall-back
 * of anything.  open: the contig lengths, the packed reference (copied) and the options (NULL: all defaults).  add_records: whole
 * records, record i is rec[rec_off[i] .. rec_off[i+1]), any cut into calls, any order.  finish: the file on pu_fd (< 0: built and
 * dropped).  After a refusal every later call returns the same code.  It holds 12 bytes per base of every reference that a record has
 * covered (n_cov, n_ref_fwd, n_ref_rev, made at the reference's first covering record), 8 bytes per observation, and its copy of the
 * packed reference. */
typedef struct { int min_mapq, min_baseq, exclude_flags, min_alt; } bwahip_pileup_opt_t;
typedef struct {
	int64_t n_sites, n_alleles, n_obs[3];         /* as in the file */
	int64_t pu_bytes;                             /* bytes of the file */
	int64_t hbm_bytes;                            /* what the stage held, the observation buffers and its share of the context's sort buffers included */
	double pileup_ms, observe_ms, sort_ms, evidence_ms;   /* GPU time by HIP events: the stage; counting and writing the observations; the sort, the alleles and the sites; the evidence pass */
} bwahip_pileup_stats_t;
typedef struct bwahip_pileup_builder bwahip_pileup_builder;
int  bwahip_pileup_builder_open(int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const bwahip_pileup_opt_t *opt, bwahip_pileup_builder **b);
int  bwahip_pileup_builder_add_records(bwahip_pileup_builder *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec);
int  bwahip_pileup_builder_finish(bwahip_pileup_builder *b, int pu_fd);
void bwahip_pileup_builder_close(bwahip_pileup_builder *b);
/* The stage on the device (csrc/k_pileup.hip), 16 lanes per record: the observations of every record are counted and, after a prefix
 * sum, written as 64-bit keys -- position among all contigs' bases (40 bits) | kind (2) | allele (21) | strand (1); the keys go through
 * the stable radix sort of the coordinate sort; alleles and their strand counts are segment lengths of the sorted keys; the kept alleles
 * and the distinct sites are compacted by prefix sums; a second pass over the records adds n_cov and n_ref to the sites inside each
 * record's span (integer atomics); the compact tables come back in one awaited download and go through the host builder's serialiser.
 * More than 2^31 - 1 observations: BWAHIP_ECAPACITY.
 * bwahip_kat_pileup: exactly that stage on the caller's records (host pointers, any order) and the caller's packed reference; the file
 * into out (out_cap too small: BWAHIP_ECAPACITY, *out_len says what it takes).  opt == NULL: all defaults.
 * bwahip_bam_devmerger_set_pileup arms a device merger: every finish (_finish, _finish_bai, _finish_markdup) then runs the stage over the
 * runs after the marking and the QC summary, if there are any, and before the order is made, and writes the file to pu_fd (< 0: built
 * and dropped) once the members are written.  A refusal comes before a byte of the members is written.  pac == NULL: the reference is
 * the context's index, where it lies in HBM; n_ref and ref_len must then equal its contig table (BWAHIP_EINVAL).  Otherwise the merger
 * copies the packed reference and uploads it at the first armed finish that follows.  opt == NULL disarms (the other arguments are not looked at); an
 * unarmed merger queues what it queued before.  *ps (may be NULL) is filled by every armed finish.  The evidence pass would need a
 * second round of windows over spilled runs, so the two do not mix: a merger armed for spilling refuses set_pileup, and once armed for
 * the pileup set_spill and add_spilled are refused, all with BWAHIP_EINVAL.
 * bwahip_pileup_hbm_need: what is known of the stage's HBM before the data, with the eighth of slack its buffers grow with (no device;
 * -1 for a negative argument): 12 bytes per record (its observations' count and their first slot) and 4 096 for the error word, the
 * counters and the contig table's first entries.  The observation buffers -- 24 bytes per observation in the context's sort buffers, 12
 * for the segment flags and their prefix sums, 32 per allele and per site -- are allocated at the finish, when their number is known;
 * hbm_budget does not count them, and a failed allocation there is BWAHIP_ENOMEM before a byte of the members is written. */
int  bwahip_kat_pileup(bwahip_ctx *ctx, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac,
                       const bwahip_pileup_opt_t *opt, uint8_t *out, int64_t out_cap, int64_t *out_len);
int  bwahip_bam_devmerger_set_pileup(bwahip_bam_devmerger *m, const bwahip_pileup_opt_t *opt, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, int pu_fd,
                                     bwahip_pileup_stats_t *ps);
int64_t bwahip_pileup_hbm_need(int64_t n_records);
/* bwahip_stream_run_bam_sorted_dev_markdup (mark != 0) or the device-merged sorted file without marking (mark == 0), with the index for
 * bai_fd >= 0, the QC summary for qc != NULL and the pileup of the file on pu_fd; the reference is the contexts' index.  The BAM file,
 * the index and the QC summary are those of the entry points without the pileup.  Never a host fall-back and never a spilled run: a run
 * that does not fit hbm_budget (which counts bwahip_pileup_hbm_need too) ends the call with BWAHIP_ECAPACITY, as _dev_markdup does;
 * sd->tmp_dir, mem_budget and level are not looked at.  pu == NULL: BWAHIP_EINVAL.  ms, qs and ps may be NULL. */
int  bwahip_stream_run_bam_sorted_dev_pileup(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0, const char *fq1, const char *fq2,
                                             int out_fd, const char *hdr_line, bwahip_stream_t *st, bwahip_sort_dev_t *sd, int bai_fd /* < 0: none */,
                                             int mark, bwahip_markdup_stats_t *ms, const bwahip_qc_opt_t *qc /* NULL: none */, int qc_fd, bwahip_qc_stats_t *qs,
                                             const bwahip_pileup_opt_t *pu, int pu_fd, bwahip_pileup_stats_t *ps);

/* Runs whose record bytes outgrow HBM (csrc/k_bamspill.hip, csrc/spill_store.cpp).  A device merger armed with
 * bwahip_bam_devmerger_set_spill may hold a run spilled: keys, offsets, template indices and descriptors in HBM as for any run, the record
 * bytes in a host-side store -- pinned host memory while host_budget holds, otherwise the whole run in an unlinked file of tmp_dir (its
 * name is gone before a byte is written).  Every finish brings them back one window of window_pieces pieces at a time, through two
 * staging buffers: window w + 1 is uploaded on the copy stream while window w is gathered and deflated.  The order, the output offsets,
 * the piece cuts and the deflate are those of a merger with all runs resident, so for any mix of resident and spilled runs the members,
 * the index, the QC summary and every count of the stats are the same; only hbm_bytes and the timings differ.  The stages that read
 * records run per window on the staged slices -- the marking pass (the store stays unmarked: every finish marks again), the QC record
 * pass, the index parse -- and each record counts once, in the window that holds its first byte or, for the record a window begins
 * with, in that window; their read-backs come after the last window, so a refusal of the QC stage or the index comes after the members
 * are written.  The limit of 2^31 - 1 records per merger stands: all keys are sorted at once; a finish over a spilled run of 0x7f7f7f7f
 * records or more: BWAHIP_ECAPACITY (the cut table's empty cell).
 * set_spill: before the first add (later, or twice: BWAHIP_EINVAL); host_budget < 0 or window_pieces > 65 536: BWAHIP_EINVAL;
 * window_pieces <= 0: 8 (with 1 024 blocks a piece, windows of 535 MB).  The out fields are not touched.  host_budget bounds the store's
 * memory alone.  Beside it a merger that holds a file-backed run pins two bounce buffers of one window each at its finish (what pread
 * fills before the upload: 1.07 GB at the default shapes, also with host_budget 0), and the stream entry point 64 MiB more for the way
 * from HBM to a file; choose window_pieces with that in mind where pinned memory is scarce.
 * add_spilled: bwahip_bam_devmerger_add (tmpl == NULL and desc == NULL) or _add_dup with the run held spilled; the same validation and
 * the same refusals, which leave merger and store as they were; an unarmed merger: BWAHIP_EINVAL; a run that needs a file while tmp_dir
 * is NULL or no directory files can be made in: BWAHIP_EIO.  Resident and spilled runs mix freely; run numbers are shared.
 * spill_stats: the out fields (the in fields are not touched): spilled runs held and the lowest run number among them, the store's
 * bytes by placement, and of the last finish the windows, the HBM of the staging (two buffers, the cut table) and the time its uploads
 * took on the copy stream; download_s: the time the record bytes took to reach the store, over all adds.
 * bwahip_bam_devmerge_spill_hbm_need (no device; -1 for a negative argument, piece_blocks outside 1 .. 4 096 or window_pieces outside
 * 1 .. 65 536): bwahip_bam_devmerge_hbm_need(resident_raw_bytes, n_records, n_runs, piece_blocks) -- the resident record bytes and all
 * records' metadata -- and, with the eighth of slack the working buffers grow with,
 *   staging    2 x min(window_pieces x piece_blocks x 65 280 + 2 x longest_record, spilled_raw_bytes): a window and the two records
 *              that straddle its ends;
 *   pieces     326 730 x (P(resident + spilled) - P(resident)), P(b) = min(blocks of b bytes, piece_blocks): the piece buffers the
 *              resident bytes alone do not count;
 *   cut table  16 x (n_runs + 1) x blocks of (resident + spilled) bytes: a cut and a slice base per run and window, counted for the most
 *              windows any shape gives (one per block), so that the need never falls as piece_blocks or window_pieces grows. */
typedef struct {
	int64_t host_budget;      /* in: bytes of pinned host memory spilled records may take; a run that would exceed it goes whole
	                             to an unlinked file in tmp_dir.  0: every spilled run is a file.  < 0: BWAHIP_EINVAL */
	const char *tmp_dir;      /* in: may be NULL while no run needs a file; unusable when one does: BWAHIP_EIO, merger as before */
	int window_pieces;        /* in: pieces (of piece_blocks x 65 280 bytes) staged per window, 1 .. 65 536; <= 0: 8 */
	/* out */
	int64_t n_spilled_runs, first_spilled_run /* -1: none */, host_bytes, file_bytes, n_windows, window_hbm_bytes;
	double download_s, upload_ms;
} bwahip_spill_t;
int  bwahip_bam_devmerger_set_spill(bwahip_bam_devmerger *m, const bwahip_spill_t *in);
int  bwahip_bam_devmerger_add_spilled(bwahip_bam_devmerger *m, int64_t run_no, const uint8_t *rec, int64_t len, const uint64_t *keys,
                                      const int64_t *rec_off, int64_t n_rec, const uint32_t *tmpl, const bwahip_dup_desc_t *desc, int64_t n_tmpl);
int  bwahip_bam_devmerger_spill_stats(bwahip_bam_devmerger *m, bwahip_spill_t *out);
int64_t bwahip_bam_devmerge_spill_hbm_need(int64_t resident_raw_bytes, int64_t spilled_raw_bytes, int64_t longest_record,
                                           int64_t n_records, int64_t n_runs, int piece_blocks, int window_pieces);
/* The device-merged entry points in one, for samples whose record bytes outgrow HBM: bai_fd >= 0 writes the index, mark != 0 marks
 * duplicates (ms may be NULL), qc != NULL writes the QC summary to qc_fd (qs may be NULL); with none of them the file is that of
 * bwahip_stream_run_bam_sorted_dev.  sd: hbm_budget (0: half of the free HBM) and piece_blocks in, fell_back stays 0, tmp_dir, mem_budget
 * and level are not looked at: there is never a host fall-back.  sp: in as for set_spill, out as from spill_stats.  Runs are decided in
 * input order: a run stays resident while bwahip_bam_devmerge_spill_hbm_need(resident bytes with it, one window of window_pieces x
 * piece_blocks x 65 280 bytes reserved as spilled, longest_record 0, all records and runs so far) plus the enabled stages' needs
 * (_bai_hbm_need, _markdup_hbm_need, bwahip_qc_hbm_need) is within hbm_budget; from the first run that is not, every run is held spilled
 * (first_spilled_run), its record bytes travelling device -> host store.  The split depends on the input and the budgets alone, not on
 * n_ctx, and the files do not depend on the split.  When what stays in HBM of the runs held -- the need with the real spilled bytes and
 * longest record -- exceeds hbm_budget, or a batch's own buffers cannot be allocated: BWAHIP_ECAPACITY, and nothing of the records has
 * been written. */
int  bwahip_stream_run_bam_sorted_dev_spill(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                            const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st,
                                            bwahip_sort_dev_t *sd, bwahip_spill_t *sp, int bai_fd /* < 0: none */,
                                            int mark, bwahip_markdup_stats_t *ms,
                                            const bwahip_qc_opt_t *qc /* NULL: none */, int qc_fd, bwahip_qc_stats_t *qs);

/* ---- Base-quality recalibration table of coordinate-sorted BAM (csrc/k_recal.hip on the device, csrc/recal_host.cpp without one) ----
 * How often a base disagrees with the reference, by reported quality, machine cycle and dinucleotide context, with known variant sites
 * kept out: one canonical table, recomputable from the records of the file, the contig lengths, the packed reference and the mask alone.
 * All values are integers.  The bytes do not depend on the order of the records, on how they are cut into runs, calls or windows, or on
 * the order in which wavefronts run.  No model is fitted and no quality rewritten; indels and read groups are no covariates; equality
 * with the report of GATK's BaseRecalibrator is not claimed.
 *   Options         min_mapq in [0, 255]; min_baseq in [0, 93]; exclude_flags in [0, 65535], < 0 means 3844 (0x4 | 0x100 | 0x200 |
 *                   0x400 | 0x800); max_cycle in [1, 65536], 0 means 1024.  Anything else: BWAHIP_EINVAL before a record is read.
 *                   The file holds them as resolved.
 *   Reference       the contig table and the packed sequence of the pileup above: .pac's layout, no hole table.
 *   Mask            optional, the known sites as a bitmap over the bases of all contigs one after the other: the base at g =
 *                   ref_off[r] + p is masked when bit g & 7 of byte g >> 3 is set; (sum of the lengths + 7) / 8 bytes are read.
 *                   NULL: nothing is masked.
 *   Per record      the checks of the pileup, with its codes; the first offending record in the order given decides.  A record takes
 *                   part when refID >= 0, flag & exclude_flags == 0, mapq >= min_mapq, l_seq > 0, the query length of its CIGAR
 *                   equals l_seq and its first quality byte is not 0xff.  A record that takes part with l_seq > max_cycle is an
 *                   offending record too: BWAHIP_ECAPACITY.  Any other record contributes nothing and is not refused.
 *   Walk            the pileup's.  The base at query index q inside an M = X operation is counted when its code is one of A C G T,
 *                   its p lies inside the contig, its quality byte b is >= min_baseq and g is not masked.  A base that meets the
 *                   other conditions and is masked counts in n_masked and nowhere else.  A counted base is an error when it differs
 *                   from the reference base.
 *   Covariates      Q = min(b, 93).  mate = (flag >> 7) & 1.  The machine cycle c = q, or l_seq - 1 - q on a record with 0x10 (hard
 *                   clips are not counted).  The context is 16 when c == 0 or the base read one cycle earlier -- index q - 1, or
 *                   q + 1 on a reverse record, whatever operation holds it -- is not A C G T; otherwise 4 x prev + this, both 0 .. 3
 *                   in read orientation: on a reverse record both are complemented.
 *   The file        little endian, no padding, 80 + 24 * (n_rows[0] + n_rows[1] + n_rows[2]) bytes:
 *                     char[4] "BRC\1" | int32 n_ref | int32 min_mapq, min_baseq, exclude_flags, max_cycle |
 *                     uint64 n_records (the records taking part), n_bases, n_err, n_masked | uint64 n_rows[3] |
 *                     the quality table, the cycle table, the context table: rows { uint32 Q, x; uint64 n_obs, n_err }.
 *                   Only rows with n_obs > 0, ascending by (Q, x); x = 0 in the quality table, mate << 31 | c in the cycle table, the
 *                   context in the context table.  Every table's n_obs sum to n_bases and its n_err to n_err.
 * Device-free builder (csrc/recal_host.cpp): the judge's twin and the one serialiser, a library for small inputs and no fall-back of
 * anything; the stage of the device merger's finish (below) hands its tables to the same serialiser.
 * open: the contig lengths, the packed reference and the mask (both copied; mask NULL: none) and the options (NULL: all defaults).
 * add_records: whole records, record i is rec[rec_off[i] .. rec_off[i+1]), any cut into calls, any order.  finish: the file on rc_fd
 * (< 0: built and dropped).  After a refusal every later call returns the same code.  It holds dense tables of 64-bit words -- 94 rows
 * of 1 + 2 * max_cycle + 17 cells, a cell n_obs and n_err: 3 MB at the default max_cycle, made at the first record that takes part --
 * the reference and the mask. */
typedef struct { int min_mapq, min_baseq, exclude_flags, max_cycle; } bwahip_recal_opt_t;
typedef struct bwahip_recal_builder bwahip_recal_builder;
int  bwahip_recal_builder_open(int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const uint8_t *mask, const bwahip_recal_opt_t *opt, bwahip_recal_builder **b);
int  bwahip_recal_builder_add_records(bwahip_recal_builder *b, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec);
int  bwahip_recal_builder_finish(bwahip_recal_builder *b, int rc_fd);
void bwahip_recal_builder_close(bwahip_recal_builder *b);
/* The stage on the device (csrc/k_recal.hip), one pass over the records, 16 lanes per record: a workgroup counts a share of 512
 * consecutive records in its LDS -- the context table whole, the cycle table for the cycles below 256 of eight qualities that claim
 * their slots on first use; every other base goes to the dense tables in HBM by 64-bit atomic adds -- and adds its non-zero cells to the
 * dense tables once (the quality table: the context table's row sums); the dense tables come back in one awaited download and go through
 * the host builder's serialiser.  Integers only: the bytes do not depend on scheduling.
 * bwahip_kat_recal: exactly that stage on the caller's records (host pointers, any order), the caller's packed reference and the
 * caller's mask (NULL: none); the file into out (out_cap too small: BWAHIP_ECAPACITY, *out_len says what it takes).  opt == NULL: all
 * defaults.
 * bwahip_bam_devmerger_set_recal arms a device merger: every finish (_finish, _finish_bai, _finish_markdup) then runs the stage over the
 * records last of the record stages, after the marking -- the default exclude_flags hold 0x400, so the table of a marked finish does not
 * count what that finish marked -- and writes the file to rc_fd (< 0: built and dropped) once the members are written.  With all runs
 * resident a refusal comes before a byte of the members is written; the stage reads every record once, so over spilled runs it runs per
 * window as the QC summary does, and a refusal then comes after the members.  It is not interlocked with set_spill.  pac == NULL: the
 * reference is the context's index, where it lies in HBM; n_ref and ref_len must then equal its contig table (BWAHIP_EINVAL).  Otherwise
 * the merger copies the packed reference; the mask is always copied (NULL: nothing is masked); the copies are uploaded at the first armed
 * finish that follows.  opt == NULL disarms (the other arguments are not looked at); an unarmed merger queues what it queued before.
 * *rs (may be NULL) is filled by every armed finish.
 * bwahip_recal_hbm_need: the stage's HBM, with the eighth of slack its buffers grow with (no device; -1 for a negative argument, a sum
 * of 2^40 or more or max_cycle > 65 536; max_cycle 0: 1 024): the dense tables -- 16 x 94 x (1 + 2 x max_cycle + 17) bytes --, the mask's
 * (sum_len + 7) / 8 bytes when with_mask != 0, and 4 096 for the counters, the error word and the contig table's first entries.  A packed
 * reference of the caller's is not counted. */
typedef struct {
	int64_t n_records, n_bases, n_err, n_masked, n_rows[3];   /* as in the file */
	int64_t rc_bytes;                             /* bytes of the file */
	int64_t hbm_bytes;                            /* what the stage held */
	double recal_ms;                              /* GPU time by HIP events: the tables cleared, the records' passes */
} bwahip_recal_stats_t;
int  bwahip_kat_recal(bwahip_ctx *ctx, const uint8_t *rec, const int64_t *rec_off, int64_t n_rec, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const uint8_t *mask,
                      const bwahip_recal_opt_t *opt, uint8_t *out, int64_t out_cap, int64_t *out_len);
int  bwahip_bam_devmerger_set_recal(bwahip_bam_devmerger *m, const bwahip_recal_opt_t *opt, int32_t n_ref, const int64_t *ref_len, const uint8_t *pac, const uint8_t *mask,
                                    int rc_fd, bwahip_recal_stats_t *rs);
int64_t bwahip_recal_hbm_need(int64_t sum_len, int max_cycle, int with_mask);
/* bwahip_stream_run_bam_sorted_dev_spill with the recalibration table of the file on rc_fd: the reference is the contexts' index, mask
 * (NULL: none) covers its contigs' bases.  The BAM file, the index and the QC summary are byte for byte those of _dev_spill with the
 * same arguments; hbm_budget counts bwahip_recal_hbm_need too.  rc == NULL: BWAHIP_EINVAL; bad options are refused before anything
 * starts.  ms, qs and rs may be NULL. */
int  bwahip_stream_run_bam_sorted_dev_recal(bwahip_ctx *const *ctxs, int n_ctx, const bwahip_opt_t *opt, const bwahip_pestat_t *pes0,
                                            const char *fq1, const char *fq2, int out_fd, const char *hdr_line, bwahip_stream_t *st,
                                            bwahip_sort_dev_t *sd, bwahip_spill_t *sp, int bai_fd /* < 0: none */,
                                            int mark, bwahip_markdup_stats_t *ms,
                                            const bwahip_qc_opt_t *qc /* NULL: none */, int qc_fd, bwahip_qc_stats_t *qs,
                                            const bwahip_recal_opt_t *rc, const uint8_t *mask, int rc_fd, bwahip_recal_stats_t *rs);

/* Insert-size statistics (mem_pestat_t[4]: FF, FR, RF, RR; bwamem_pair.c:72) and mate-rescue counters ([0] local alignments
 * run, [1] regions added, [2] most alignments of one pair, [3] pairs that needed any; bwamem_pair.c:137) of the last
 * paired-end batch finalised on the GPU.  Either pointer may be NULL; counters4 receives 4 values. */
int bwahip_last_pe_stats(bwahip_ctx *ctx, bwahip_pestat_t *pes4, uint64_t *counters4);

/* Concatenate seqs[0..n).sam into one malloc()ed buffer (read order; *out_len bytes + a NUL) and free the per-read strings. */
int bwahip_seqs_take_sam(bwahip_seq_t *seqs, int n, char **out, int64_t *out_len);

/* ---- stage-level entry points (parity tests and bench) --------------------
 * Reads are given packed: `seq` holds the concatenated 0..4 codes, read i is seq[off[i] .. off[i+1]).
 * Results come back as "i64 record" streams in malloc()ed buffers (*out, *out_len int64 words) in the
 * same layout the oracle's stage dump uses (oracle/ref_driver.c): see bwahip_stage_* tags. */
#define BWAHIP_STAGE_INTV      1   /* intervals after mem_collect_intv (bwamem.c:137) */
#define BWAHIP_STAGE_CHAIN     2   /* chains after mem_chain (bwamem.c:258), B-tree order */
#define BWAHIP_STAGE_CHAIN_FLT 3   /* chains after mem_chain_flt (bwamem.c:334) */
#define BWAHIP_STAGE_REGS_PRE  5   /* regions after all mem_chain2aln calls (bwamem.c:1079) */
#define BWAHIP_STAGE_REGS      4   /* regions returned by mem_align1_core */
int bwahip_run_stages(bwahip_ctx *ctx, const bwahip_opt_t *opt, int n, const uint8_t *seq, const int64_t *off,
                      int stage_mask, int64_t **out, int64_t *out_len);

/* The same for the paired-end path (reads 2i and 2i+1 are a pair; BWAHIP_F_PE is implied): insert-size statistics, mate rescue and
 * pairing run exactly as bwahip_process_seqs runs them, up to and including the pairing kernel; no output is made.  pes0 and
 * n_processed as for bwahip_process_seqs.  Records: BWAHIP_STAGE_PESTAT once, in front of the first read; per read the header and
 * BWAHIP_STAGE_REGS (the list mem_sam_pe is given), _REGS_PE, _PAIR as asked for. */
#define BWAHIP_STAGE_PESTAT    7   /* mem_pestat (bwamem_pair.c:72): per direction FF, FR, RF, RR low, high, failed and the bit patterns of avg and std */
#define BWAHIP_STAGE_REGS_PE   8   /* regions after all mem_matesw calls, before mem_mark_primary_se (bwamem_pair.c:299); layout of BWAHIP_STAGE_REGS */
#define BWAHIP_STAGE_PAIR      9   /* mem_sam_pe's decisions: paired (bwamem_pair.c:311-384) or not; region of h[i] (paired: z[i]; else the region the
                                      mate information comes from, -1 none); ALT region printed as supplementary or -1; q_se[i] (0 when not paired);
                                      extra_flag as mem_sam_pe holds it at that point (the proper-pair bit of an unpaired end is set later, when
                                      the records are written); and per pair mem_pair's return value, sub and n_sub (0 when mem_pair did not run) */
int bwahip_run_pe_stages(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n, const uint8_t *seq, const int64_t *off,
                         const bwahip_pestat_t *pes0, int stage_mask, int64_t **out, int64_t *out_len);
/* Which paths the paired-end kernels of the last batch took (work counts, kept by the kernels): [0] / [1] mate-rescue alignments run
 * ahead of the sequential pass by the byte / the word kernel, [2] / [3] alignments run inside the sequential pass with the reference
 * window in LDS / in global memory, [4] rescued regions placed without sorting the list again, [5] full sort-and-dedup passes,
 * [6] pairs whose lists stayed in global memory, [7] pairs whose lists were copied by a whole wavefront, [8..11] alignments attempted
 * per orientation FF, FR, RF, RR, [12] windows dropped because their middle lies in another contig than the anchor, [13] pairs with one
 * end rescued by the byte and the other by the word kernel's instantiation.  out[i] for i >= 14 is set to 0. */
int bwahip_last_pe_paths(bwahip_ctx *ctx, uint64_t *out, int n);

/* Device-resident batch for benchmarking: upload once, run the whole hot path (seq codes in HBM ->
 * alignment regions in HBM) any number of times.  kernel_ms (may be NULL) receives the per-kernel
 * durations of the last run measured with HIP events on the launch stream, in launch order
 * (see bwahip_kernel_name). */
int bwahip_batch_upload(bwahip_ctx *ctx, int n, const uint8_t *seq, const int64_t *off);
/* The same for reads that already sit in HBM of the context's device (codes 0..4 concatenated, off_dev[0] == 0): nothing
 * is copied, the buffers stay the caller's and must stay valid until the next upload / attach / destroy. */
int bwahip_batch_attach(bwahip_ctx *ctx, int n, const uint8_t *seq_dev, const int64_t *off_dev, int max_len, int64_t total_bases);
int bwahip_batch_run(bwahip_ctx *ctx, const bwahip_opt_t *opt, float *kernel_ms, int n_kernel_ms);
int bwahip_batch_download(bwahip_ctx *ctx, bwahip_alnreg_v *regs_out);       /* regs of the last run */
/* The whole of mem_process_seqs on a device-resident batch: attach the text the SAM stage prints (qualities: read r at
 * qual_dev + qual_off_dev[r], or qual_off_dev[r] < 0 / qual_dev NULL for none; NUL-terminated names at names_dev +
 * name_off_dev[r], buffer padded by 64 bytes), run hot path + finalisation + SAM text on the GPU (SE, or PE when
 * opt->flag has MEM_F_PE; n_processed / pes0 as in mem_process_seqs), then fetch the text.  kernel_ms: as
 * bwahip_batch_run; entries 11..15 are the finalisation stages (see bwahip_kernel_name). */
int bwahip_batch_attach_text(bwahip_ctx *ctx, const uint8_t *qual_dev, const int64_t *qual_off_dev, const uint8_t *names_dev, const int64_t *name_off_dev);
int bwahip_batch_run_sam(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, const bwahip_pestat_t *pes0, float *kernel_ms, int n_kernel_ms);
int bwahip_batch_sam(bwahip_ctx *ctx, char **out, int64_t *out_len, int64_t *off);
/* The same pair with BAM records as the output (see bwahip_process_seqs_bam; a batch is finalised for one format: run again for the
 * other).  kernel_ms slots as for the SAM passes.  Names of 255 bytes or more: BWAHIP_EINVAL, judged by the name offsets. */
int bwahip_batch_run_bam(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, const bwahip_pestat_t *pes0, float *kernel_ms, int n_kernel_ms);
int bwahip_batch_bam(bwahip_ctx *ctx, uint8_t **out, int64_t *out_len, int64_t *off);
/* The same pair with the records in coordinate order (bwahip_process_seqs_bam_sorted).  sort_ms4 (may be NULL): the sort stage of the run
 * measured with HIP events -- [0] record table, [1] radix sort, [2] gather (milliseconds), [3] the number of radix passes that ran.
 * bwahip_batch_bam_sorted: records, keys (*n_rec) and offsets (*n_rec + 1), each in a malloc()ed buffer. */
int bwahip_batch_run_bam_sorted(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, const bwahip_pestat_t *pes0, float *kernel_ms, int n_kernel_ms, float *sort_ms4);
int bwahip_batch_bam_sorted(bwahip_ctx *ctx, uint8_t **out, int64_t *out_len, uint64_t **keys, int64_t **rec_off, int64_t *n_rec);
/* The same pair with the records as BGZF members (bwahip_process_seqs_bgzf); they stay in HBM until bwahip_batch_bgzf fetches them
 * into a malloc()ed buffer.  deflate_ms (may be NULL): the deflate stage of the run measured with HIP events.  raw_len, n_blocks,
 * n_stored (each may be NULL): the bytes of the records, the members, the members that are stored. */
int bwahip_batch_run_bgzf(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, const bwahip_pestat_t *pes0, float *kernel_ms, int n_kernel_ms, float *deflate_ms);
int bwahip_batch_bgzf(bwahip_ctx *ctx, uint8_t **out, int64_t *out_len, int64_t *raw_len, int64_t *n_blocks, int64_t *n_stored);
int bwahip_n_kernels(void);
const char *bwahip_kernel_name(int i);
/* Algorithmic work counters of the last bwahip_batch_run, counted on the device by the kernels
 * themselves: [0] bwt_extend calls, [1] Occ blocks touched by them,
 * [2] bwt_sa calls, [3] LF steps, [4] intervals written, [5] seeds, [6] DP cells, [7] most bwt_extend
 * calls of one read; [8..15] per-phase maxima over reads (10 ns ticks) and the largest seed / chain
 * counts of one read; [16,17] Occ blocks / intervals of k_smem_heavy, [24,25] of k_smem3 (both are
 * included in [1] and [4]; bench.py subtracts them to attribute bytes to k_smem); [19,20] DP rows
 * with one / several columns per lane; [21..23] dedup phase maxima; [27] ksw_extend2 calls of the extension
 * kernels, [28] those the diagonal rule (knob ext_diag) answered without a DP row; [29] look-ups of the interval
 * table by k_smem's table jump (knob smem_skip; the bwt_extend calls they stand in for are not in [0]), [30] bwt_smem1a calls the
 * jump abandoned and ran again plainly.  n <= 32. */
int bwahip_batch_counters(bwahip_ctx *ctx, uint64_t *counters, int n);

/* Known-answer helpers used by the parity tests: device Occ/extend/SA on arrays of inputs. */
int bwahip_kat_occ4(bwahip_ctx *ctx, int n, const uint64_t *k, uint64_t *cnt4_out);
/* What the index occupies in HBM: interval of the SA table the kernels read (1 = every BWT row; the index files hold every 32nd, bwt.c:86
 * walks the rest), longest string of the interval table (0: none), and the bytes of {BWT with Occ counts, SA table, packed reference,
 * interval table}.  Tunables: BWAHIP_SA_INTV, BWAHIP_KMER_K. */
int bwahip_index_footprint(bwahip_ctx *ctx, int *sa_intv, int *kmer_k, uint64_t *bytes4);
int bwahip_kat_sa(bwahip_ctx *ctx, int n, const uint64_t *k, uint64_t *sa_out);
/* The interval table of the BWT search (strings of up to *k_out bases): every entry of every length against bwt_extend (bwt.c:262) run
 * FORWARD from the entry of the string without its last base (the table itself is filled by backward extensions); *bad_out = mismatches. */
int bwahip_kat_kmer_table(bwahip_ctx *ctx, int *k_out, uint64_t *bad_out);
int bwahip_kat_extend(bwahip_ctx *ctx, int n, const uint64_t *ik3, const int *is_back, uint64_t *ok12_out);
int bwahip_kat_ksw_extend(bwahip_ctx *ctx, int n, const int *params /*n x 10*/, const uint8_t *q, const int64_t *qoff,
                          const uint8_t *t, const int64_t *toff, int *out6 /*n x 6*/);

/* ksw_extend2 (ksw.c:380) as the extension kernels compiled for `cpl` columns per lane run it: the plain form and the windowed one,
 * which must agree (else score = -777777).  params: n x 12 ints (qlen, tlen, w, h0, zdrop, end_bonus, o_del, e_del, o_ins, e_ins,
 * reverse, cpl); reverse = 1 reads both sequences backwards, as the left extension does; cpl is 3, 4, 5 or 11.  mat25: n x 25, one
 * 5x5 matrix per item (the largest entry is taken from it as the kernels take it from the options).  out7: n x 7 (score, qle, tle,
 * gtle, gscore, max_off, path), path = the forms the windowed driver went through, BWAHIP_KAT_EXT_* or-ed, with
 * BWAHIP_KAT_EXT_STOPPED when the early stop (knob ext_early_stop of the context, which both calls follow) ended its loop.
 * BWAHIP_EINVAL: h0 <= 0, an unknown cpl, negative lengths or gap costs, an extension cost below 1, offsets shorter than the lengths;
 * BWAHIP_ECAPACITY: qlen above BWAHIP_MAX_READ_LEN or qlen + 1 above 64 x cpl, tlen above the kernels' window in LDS (2124).  Nothing
 * is launched then. */
#define BWAHIP_KAT_EXT_ROWS1    1     /* windowed rows with 1 .. 4 columns per lane */
#define BWAHIP_KAT_EXT_ROWS2    2
#define BWAHIP_KAT_EXT_ROWS3    4
#define BWAHIP_KAT_EXT_ROWS4    8
#define BWAHIP_KAT_EXT_SHORT    16    /* flank below 64 bases: plain form, one column per lane */
#define BWAHIP_KAT_EXT_WIDE     32    /* band too wide for the window: plain form */
#define BWAHIP_KAT_EXT_BEYOND16 64    /* scores beyond 16 bits: plain form */
#define BWAHIP_KAT_EXT_STOPPED  128   /* the loop ended because no later row could change a result (never with ext_early_stop = 0) */
int bwahip_kat_ksw_extend2(bwahip_ctx *ctx, int n, const int *params /*n x 12*/, const int8_t *mat25 /*n x 25*/, const uint8_t *q, const int64_t *qoff,
                           const uint8_t *t, const int64_t *toff, int *out7 /*n x 7*/);
/* The same call as the extension kernels make it: the windowed driver first tries the diagonal rule (knob ext_diag of the context, DESIGN.md
 * section 4.6), which bwahip_kat_ksw_extend2 never applies -- its path bits and stop counts are those of the DP forms.  A call the rule
 * answered reports BWAHIP_KAT_EXT_DIAG and no other path bit; with ext_diag = 0 no call reports it.  Arguments, results and errors as above. */
#define BWAHIP_KAT_EXT_DIAG     256   /* the diagonal rule answered the call: no DP row ran (never with ext_diag = 0) */
int bwahip_kat_ksw_extend2_diag(bwahip_ctx *ctx, int n, const int *params /*n x 12*/, const int8_t *mat25 /*n x 25*/, const uint8_t *q, const int64_t *qoff,
                                const uint8_t *t, const int64_t *toff, int *out7 /*n x 7*/);

/* ksw_global2 (ksw.c:504) with CIGAR through the code mem_reg2aln's kernels run (DP form by band and length, wavefront backtrack).
 * params: n x 10 ints (qlen, tlen, w, o_del, e_del, o_ins, e_ins, reverse, form, cpl); reverse = 1 reads both sequences backwards, as
 * for a reverse-strand hit (bwa.c:275-280).  form: AUTO_SMALL = what the ordinary CIGAR kernel takes (band forms on its global slab);
 * AUTO_BIG = what the large-task kernel takes (band forms up to 128 diagonals, the row-wise form chosen by qlen above); SCORE_ONLY =
 * the score-only DP of mem_patch_reg at cpl (3, 4, 5 or 11) columns per lane.  cpl is ignored by the first two.  mat25: n x 25.
 * out2: n x 2 (score, n_cigar); n_cigar = -1 (score 0) when the item does not fit the form -- AUTO_SMALL: a band of more than 128
 * diagonals or tlen above 1536; either: more than BWAHIP_KAT_MAX_CIGAR operations -- and 0 for SCORE_ONLY.  cigar: n x
 * BWAHIP_KAT_MAX_CIGAR words, length << 4 | op as ksw.c:493 packs them, the rest zero.
 * BWAHIP_EINVAL: an unknown form or (SCORE_ONLY) cpl, a length below 1, w below 1 or below |tlen - qlen| (the band forms rely on what bwa.c:293-300
 * guarantees), a negative gap cost, an extension cost below 1; BWAHIP_ECAPACITY: qlen above BWAHIP_MAX_READ_LEN, tlen above 8192 (2124
 * for SCORE_ONLY), or qlen + 1 above 64 x cpl for SCORE_ONLY.  Nothing is launched then. */
#define BWAHIP_KAT_GLOBAL_AUTO_SMALL 0
#define BWAHIP_KAT_GLOBAL_AUTO_BIG   1
#define BWAHIP_KAT_GLOBAL_SCORE_ONLY 2
#define BWAHIP_KAT_MAX_CIGAR 512
int bwahip_kat_ksw_global(bwahip_ctx *ctx, int n, const int *params /*n x 10*/, const int8_t *mat25 /*n x 25*/, const uint8_t *q, const int64_t *qoff,
                          const uint8_t *t, const int64_t *toff, int *out2 /*n x 2*/, uint32_t *cigar /*n x BWAHIP_KAT_MAX_CIGAR*/);

/* The region-list sorts (ks_introsort over mem_ars2 / mem_ars keys, bwamem.c:398-402, ksort.h:176) as the kernels run them: the whole
 * wavefront's exact form (csrc/isort_dev.h) and the one-lane restatement of ksort.h on the same n keys {k64, score, qb} (mode 0: by k64;
 * mode 1: score descending, k64, qb).  idx_par / idx_seq: the two permutations; status2[0] = 1 when the parallel form ran to the end
 * (0: the introsort's depth limit -- it hands over to the one-lane form, idx_par is the identity), status2[1] != 0: internal error. */
int bwahip_kat_introsort(bwahip_ctx *ctx, int n, int mode, const int64_t *k64, const int *score, const int *qb, int *idx_par, int *idx_seq, int *status2);

/* The list update of mate rescue (mem_matesw, bwamem_pair.c:186-203) through the code k_matesw runs, on caller lists: n_items independent
 * items, one wavefront each.  Item i: a start list of list_off[i + 1] - list_off[i] regions in any arrangement (ties and duplicates
 * allowed) and the steps step_off[i] .. step_off[i + 1]; a step is one orientation in which the alignment was attempted -- step_hit != 0:
 * it produced the region given, which goes into the list; 0: no hit -- and at whose end the reference calls mem_sort_dedup_patch
 * (bns == 0).  The item starts as k_matesw starts an end (list not known to be clean).  Regions travel as the 19 words per region of
 * BWAHIP_STAGE_REGS_PE (the words the device keeps no field for are ignored and come back 0); a step without a hit still owns 19 words.
 * Of opt only max_chain_gap and mask_level_redun are read.  mode 0: as shipped (incr_insert where its conditions hold); 1: never
 * incremental, every step ends in the full sort-and-dedup.  where 0: lists of capacity (start length + steps) up to 224 regions are
 * worked on in LDS, longer ones in global memory, as k_matesw decides; 1: global memory always.  out_words: 19 words per region, item i
 * from region list_off[i] + step_off[i] on (room for its capacity); out_n[i]: its final length; out_cnt3: per item the regions placed by
 * incr_insert, the regions placed by score in front of a full pass, and the orientations that ended in a full pass.
 * BWAHIP_EINVAL: a negative length, offsets that do not start at 0 or do not ascend.  n_items == 0 launches nothing. */
int bwahip_kat_mate_insert(bwahip_ctx *ctx, const bwahip_opt_t *opt, int n_items, const int64_t *list_off, const int64_t *list_words, const int64_t *step_off,
                           const int32_t *step_hit, const int64_t *step_words, int mode, int where, int64_t *out_words, int32_t *out_n, int32_t *out_cnt3);

/* Chaining and the chain filter (mem_chain's seed loop bwamem.c:280-317, mem_chain_flt bwamem.c:334-392) through the kernels of
 * csrc/k_chain.hip, on caller seed lists: the buffers, their sizes and the launches are those of the stage chain, under the context's
 * knobs (chain_big_min, chain_mid_max, chain_big_max, chain_glb_grid).  Read i: read_len[i] bases (1 .. BWAHIP_MAX_READ_LEN); its seeds
 * seeds4[4 * seed_off[i] .. 4 * seed_off[i + 1]) as (rbeg, qbeg, len, rid) in look-up order -- rid the contig of bns_intv2rid, -1 for a
 * seed mem_chain skips; its intervals intv3[3 * intv_off[i] ..) as (x[2], qbeg, qend) in sorted order, read only for frac_rep.
 * *out: a malloc()ed stream of i64 records, per read [100: i, len], BWAHIP_STAGE_CHAIN (the chains before the filter; w, kept, first 0),
 * BWAHIP_STAGE_CHAIN_FLT.  diag (may be NULL): BWAHIP_CHAIN_DIAG_N ints per read -- [0] who took the read: -1 k_chain (one read per lane),
 * 0..3 the class of k_chain_big (B-tree in 14 / 77 / 150 KB of LDS, in global memory), 4 a class 1 / 2 read that the global-memory kernel
 * took off the queue; [1] B-tree nodes used; [2] tree height; [3] the sort by weight: 0 fewer than two chains, 1 k_chain's one-lane
 * introsort, 2 the wavefront's, 3 one lane because the sort area was too small, 4 one lane because the depth limit was hit; [4] the
 * overlap filter: 0 none, 1 sequential, 2 k_chain_flt; [5] chains before the filter.
 * BWAHIP_EINVAL: offsets that do not start at 0 or do not ascend, a seed outside its read or the reference, a contig that does not
 * exist.  n_reads == 0 launches nothing. */
#define BWAHIP_CHAIN_DIAG_N 8
int bwahip_kat_chain(bwahip_ctx *ctx, const bwahip_opt_t *opt, int n_reads, const int32_t *read_len, const int64_t *seed_off, const int64_t *seeds4,
                     const int64_t *intv_off, const int64_t *intv3, int64_t **out, int64_t *out_len, int32_t *diag);

/* The stage between the region list and the output (mem_mark_primary_se bwamem.c:528, mem_reorder_primary5 bwamem.c:988 under
 * BWAHIP_F_PRIMARY5, the record filter of mem_reg2sam bwamem.c:1025-1031, the XA membership of mem_gen_alt bwamem_extra.c:131-145,
 * mem_approx_mapq_se bwamem.c:962) through k_mark of csrc/k_final.hip, on caller region lists: the finalisation's own buffers, sizes and
 * launch, only the lists come from the caller.  Read i of the batch (its id for the tie-breaking hash follows from n_processed, i and
 * BWAHIP_F_PE as in mem_process_seqs) has the regions reg_words[19 * reg_off[i] .. 19 * reg_off[i + 1]), 19 words per region in the
 * layout of BWAHIP_STAGE_REGS (sub, alt_sc, secondary, secondary_all are not read).  plan 1: k_mark as the single-end path launches it,
 * with the selection; 0: as the paired-end path does, without.  pairs (may be NULL): n_pairs distinct pair indices (reads 2p, 2p + 1);
 * the batch is then marked by the two launches of the paired-end path -- every pair but the listed ones, then the listed ones -- instead
 * of one.
 * *out: a malloc()ed stream of i64 records, per read [100: i, n] and [BWAHIP_KAT_MARK_TAG: n, n_pri, regions with an alignment task,
 * regions with a record, then BWAHIP_KAT_MARK_WORDS words per region in the final order: the 19 words of a stage record with sub,
 * alt_sc, secondary, secondary_all as marked; hash; the index the region had in the input list; need (1: prints a record, 2: listed in
 * an XA tag); the region whose XA tag lists it, or -1; mem_approx_mapq_se of the region (of every region, secondary or not); 1 where
 * that needs a logarithm beyond the table (a span, sub_n + 1 or seedcov of 65536 and more: the output path reports an error), mapQ 0
 * then].  With plan 0 need, the XA region and the two counts are 0.
 * BWAHIP_EINVAL: offsets that do not start at 0 or descend, qe < qb, re < rb, a contig that does not exist, an odd n_reads with
 * BWAHIP_F_PE or with pairs, a pair index out of range or given twice.  n_reads == 0 launches nothing. */
#define BWAHIP_KAT_MARK_TAG   41
#define BWAHIP_KAT_MARK_WORDS 25
int bwahip_kat_mark(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n_reads, const int64_t *reg_off, const int64_t *reg_words,
                    int plan, const int32_t *pairs, int n_pairs, int64_t **out, int64_t *out_len);

/* mem_pair (bwamem_pair.c:208-272) and the decisions of mem_sam_pe (bwamem_pair.c:303-365, 397-411) through k_pair of csrc/k_pair.hip, on
 * caller region lists.  Reads 2p and 2p + 1 form pair p (id n_processed / 2 + p); BWAHIP_F_PE is implied.  The lists (as for
 * bwahip_kat_mark) are laid into the paired-end list buffers with exactly n slots per read -- the tightest layout: the 16 bytes of scratch
 * per slot hold v, the spare region array the keys of the bitonic sort --, marked by k_mark exactly as the paired-end path marks them (one
 * launch; with pairs the two launches: every pair but the listed ones, then the listed ones) and paired by k_pair with the same subsets.
 * pes[4]: the insert-size statistics per orientation as mem_pestat would give them; the penalty table is made from them as in the product.
 * *out: a malloc()ed stream of i64 records, per read [100: i, n] and [BWAHIP_KAT_PAIR_TAG: the 8 words of BWAHIP_STAGE_PAIR, n, n_pri,
 * regions with an alignment task, regions with a record, then BWAHIP_KAT_PAIR_WORDS words per region in the final order: the 19 words of
 * a stage record as k_pair left them (sub, secondary, secondary_all), the index the region had in the input list, need (1: prints a
 * record, 2: listed in the XA tag of a printed record, 4: only the mate information of the other end), the region whose XA tag lists it
 * or -1].  Everything a launch must write starts as 0xff.
 * BWAHIP_EINVAL: what bwahip_kat_mark refuses, pes == NULL, an odd n_reads, a live orientation with high - low above 2^26.
 * BWAHIP_EINTERNAL: an error code from the kernels (61: n_sub + 1 beyond the log table, 62: a span beyond it).  n_reads == 0 launches nothing. */
#define BWAHIP_KAT_PAIR_TAG   43
#define BWAHIP_KAT_PAIR_WORDS 22
int bwahip_kat_pair(bwahip_ctx *ctx, const bwahip_opt_t *opt, int64_t n_processed, int n_reads, const int64_t *reg_off, const int64_t *reg_words,
                    const bwahip_pestat_t pes[4], const int32_t *pairs, int n_pairs, int64_t **out, int64_t *out_len);

/* mem_sort_dedup_patch (bwamem.c:444-496, with mem_patch_reg bwamem.c:413) and the is_alt marking of bwamem.c:1091-1095 through the
 * dedup kernels of csrc/k_extend.hip, on caller region lists.  Read i has the bases seq[off[i] .. off[i + 1]) (codes 0..4; mem_patch_reg
 * aligns the query) and the regions reg_words[19 * reg_off[i] .. 19 * reg_off[i + 1]), 19 words per region in the layout of
 * BWAHIP_STAGE_REGS (alt_sc, secondary, secondary_all are not carried: they come back 0); heavy (may be NULL): heavy[i] != 0 puts read i
 * on the heavy reads' list instead of the bulk's.  The lists are laid into the extension stage's own buffers as k_extend leaves them --
 * the sizing and the launch record are the ones of the hot path (one function for both), slots from an exclusive scan with exactly n
 * slots per read, reg_n and the dedup lists filled -- and the launches are those that follow k_extend (one function for both); the
 * kernel for the longest read, ext_lds_window and rank_sort_min are chosen as in the product.
 * form BWAHIP_KAT_DEDUP_PRODUCT: heavy list through k_dedup, bulk through k_dedup_fast, what that refuses through k_dedup;
 * BWAHIP_KAT_DEDUP_FULL: both lists straight through k_dedup; BWAHIP_KAT_DEDUP_SLAB: every read through a known-answer kernel that runs
 * k_extend_big's dedup body (window in the global-memory slab, list in global memory whatever its length, query fetched on demand).
 * with_diag != 0: the instantiations of the kernels that also fill diag (the product's compile the diagnostics out); 0: the product's own
 * instantiations: diag comes back 0 but for the reads handed over, which the slab kernel -- it always fills diag -- describes.
 * A read whose patch window exceeds the LDS window is handed over by k_dedup, which has permuted (longer than 32 regions) its list in
 * place by then: the entry uploads the ORIGINAL list of every such read again, runs those reads through the slab kernel and counts them in
 * *n_handed.  This differs from the product, where k_extend_big rebuilds such a read's list from its chains before the same dedup body.
 * out_n[i]: the final length; out_words: the final regions of read i at 19 * reg_off[i]; diag[i]: the BWAHIP_KAT_DEDUP_* word below.
 * BWAHIP_EINVAL: offsets that do not start at 0 or descend, a list of fewer than 2 regions (k_extend finishes those itself), qe < qb,
 * re < rb, qb < 0, qe beyond the read, a contig that does not exist, a region that leaves its contig (or, on the reverse strand, the
 * contig's mirror image) and so any region across l_pac.  n_reads == 0 launches nothing. */
#define BWAHIP_KAT_DEDUP_PRODUCT 0
#define BWAHIP_KAT_DEDUP_FULL    1
#define BWAHIP_KAT_DEDUP_SLAB    2
/* diag word: who finished the read (one of the first four bits) */
#define BWAHIP_KAT_DEDUP_FAST    0x1        /* k_dedup_fast */
#define BWAHIP_KAT_DEDUP_STAGED  0x2        /* k_dedup, list in LDS (at most 32 regions) */
#define BWAHIP_KAT_DEDUP_GLOBAL  0x4        /* k_dedup, list in global memory */
#define BWAHIP_KAT_DEDUP_SLABBED 0x8        /* the slab kernel */
#define BWAHIP_KAT_DEDUP_HANDED  0x10       /* k_dedup handed the read over (patch window beyond the LDS window) */
#define BWAHIP_KAT_DEDUP_LANE1   0x20       /* the sort by re ran as the one-lane introsort (else the wavefront's sort) */
#define BWAHIP_KAT_DEDUP_LANE2   0x40       /* the same for the sort by (score, rb, qb) */
#define BWAHIP_KAT_DEDUP_WHY_SHIFT 7        /* 2 bits: why k_dedup_fast refused a list of at most 8 -- 1 tie in the first sort, 2 patch candidate, 3 tie in the second */
#define BWAHIP_KAT_DEDUP_ALN_SHIFT 9        /* 11 bits: patch alignments run by whoever finished the read (held at 2047) */
#define BWAHIP_KAT_DEDUP_MRG_SHIFT 20       /* 11 bits: of these, merged */
int bwahip_kat_dedup(bwahip_ctx *ctx, const bwahip_opt_t *opt, int n_reads, const uint8_t *seq, const int64_t *off, const int64_t *reg_off,
                     const int64_t *reg_words, const uint8_t *heavy, int form, int with_diag, int32_t *out_n, int64_t *out_words, int32_t *diag, int32_t *n_handed);

/* The stable LSD radix sort of the coordinate-sorted BAM output (csrc/k_bamsort.hip) on caller keys: exactly the product's passes for
 * keys of key_bits (1..64) significant bits -- 8 bits per pass, passes in which all keys agree skipped.  idx_out[i] = input position of
 * the i-th key in sorted order, equal keys in input order; *tile_out (may be NULL): items one workgroup ranks per pass.  n <= 1 launches
 * nothing. */
int bwahip_kat_radix_sort(bwahip_ctx *ctx, int64_t n, const uint64_t *keys, int key_bits, uint32_t *idx_out, int *tile_out);

/* The deflate stage of the BGZF output (csrc/k_bgzf.hip) on caller bytes: exactly the product's kernels.  `len` bytes are cut every
 * 65 280; out receives one complete member per block (18-byte header with BSIZE, a raw deflate stream -- a dynamic block, or the
 * stored form where that is not larger --, CRC32, ISIZE; never more than 65 536 bytes), concatenated; *n_blocks members, *n_stored of
 * them stored.  out_cap below n_blocks x 65 536: BWAHIP_ECAPACITY.  len == 0: no member, nothing is launched. */
int bwahip_kat_bgzf(bwahip_ctx *ctx, const void *data, int64_t len, uint8_t *out, int64_t out_cap, int64_t *out_len, int64_t *n_blocks, int64_t *n_stored);

/* ksw_align2 (ksw.c:343) on the device, byte or word kernel as xtra's KSW_XBYTE says.  params: n x 8 ints
 * (qlen, tlen, xtra, o_del, e_del, o_ins, e_ins, 0); mat25 NULL = the default 1/-4 matrix; out7: n x 7
 * (score, te, qe, score2, te2, tb, qb). */
int bwahip_kat_ksw_align(bwahip_ctx *ctx, int n, const int *params, const int8_t *mat25, const uint8_t *q, const int64_t *qoff,
                         const uint8_t *t, const int64_t *toff, int *out7);

/* Tuning knobs of the heavy-read hand-off kernels (tests force each one onto ordinary reads): keys intv_cap,
 * smem_lanes, heavy_mult, chain_big_min, rank_sort_min, spec_min_chains, ext_lds_window, verbose; and ext_early_stop (default 1): every
 * device form of ksw_extend2 ends its row loop once no later row can change score, qle, tle, gtle, gscore or max_off --
 * 0 runs every row to the end as the reference does (same results, more rows); and ext_diag (0 or 1, default 1): the extension kernels
 * answer a ksw_extend2 call whose flank holds only ACGT and at most K mismatches (K = 1 at the default scores) from the main diagonal,
 * without a DP row -- 0 runs the rows of every call (same results); and smem_skip (-1, 0 or >= 2, default -1): the
 * depth J of k_smem's table jump -- a bwt_smem1a call of passes 1-2 starts at the interval table's entry of its
 * first J bases and materialises the J - 1 shorter ends by one look-up each; -1 takes the largest J with 4^J <= text length / 16, 0 runs
 * every call plainly, and any depth is held to the table's and to min_seed_len (same intervals; 1 is refused); and sorted_piece_blocks (1 .. 4096, default 1024): the
 * BGZF blocks a device merger gathers and deflates at a time (bwahip_bam_devmerger_open with piece_blocks <= 0; the bytes do not depend on it);
 * and incr_insert (0 or 1, default 1): mate rescue places a rescued region into a list that the last mem_sort_dedup_patch left free of
 * ties without sorting the list again -- 0 ends every orientation in the full sort-and-dedup, as the reference does.  The knob changes
 * no result: lists, pairing and output are the same with either value, only bwahip_last_pe_paths [4] and [5] differ;
 * and chain_mid_max / chain_big_max (defaults 1536 / 3200, larger values are held to these): the seeds up to which a read taken by a
 * wavefront (more than chain_big_min seeds, and more than 256) keeps its B-tree in 77 KB / 150 KB of LDS, beyond chain_big_max in
 * global memory; chain_glb_grid (1 .. 65536, default 2048, at least 64 are launched): the workgroups of that last kernel.  None of
 * the three changes a result.
 * The same knobs are read from the environment (BWAHIP_<KEY>) once, when the context is created. */
int bwahip_ctx_tune(bwahip_ctx *ctx, const char *key, int value);

const char *bwahip_version(void);

#ifdef __cplusplus
}
#endif
#endif
