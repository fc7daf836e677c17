// The three stages bwahip_process_seqs_text / _bam consist of, as the stream driver (stream.cpp) runs them: stage-in of batch k+1 and
// stage-out of batch k-1 beside the kernels of batch k, every one on a thread of its own.  Implemented in final_rt.hip.
//
// A context has PIPE_SETS input sets (device copies of bases / qualities / names / comments with their offsets, and the pinned buffer they
// travel through) and PIPE_SETS output sets (SAM text or BAM records in HBM, and the pinned buffer they come back into); the working set
// between them stays single, because one batch computes at a time per context.  The driver owns the bookkeeping: a set goes
//   input:  free -> pipe_stage_in -> pipe_compute -> free once pipe_stage_out has seen the batch's kernels end
//   output: free -> pipe_compute -> pipe_stage_out -> the writer -> free once the bytes are on the descriptor
// and no stage touches (let alone reallocates) a set another stage holds.  Not part of the C ABI.
#pragma once
#include "../../include/bwahip.h"
#include "ctx_internal.h"                                       // OutForm, DevRun

constexpr int PIPE_SETS = 2;

// Makes the context's sets (first call) and starts its n_threads - 1 long-lived staging threads (the caller of pipe_stage_in is the n-th).
int pipe_open(bwahip_ctx *c, int n_threads);
// Waits for everything the stages queued on the context's streams and ends the staging threads; the buffers stay for the next run.
void pipe_close(bwahip_ctx *c);
// Offsets, longest read, gather into the pinned buffer of input set `in`, asynchronous copies to HBM on the copy stream; returns when the
// copies are done (the caller is a staging thread with nothing else to do), so `seqs` may be released on return.  Nothing is written to `seqs`.
int pipe_stage_in(bwahip_ctx *c, int in, const bwahip_opt_t *opt, int n, const bwahip_seq_t *seqs, OutForm form, double *t_copy_begin);
// k_nt4_conv, the hot path and the finalisation of input set `in` into output set `out`; returns when the write pass is queued
// (OutForm::BamSorted: when the gather is queued; the sort stage awaits two small read-backs on the way, the record count and the bits that differ
// between the keys, so the caller is held until the write pass has ended; OutForm::Bgzf: the deflate stage is queued behind the write pass).
int pipe_compute(bwahip_ctx *c, int in, int out, const bwahip_opt_t *opt, int64_t n_processed, const bwahip_pestat_t *pes0, OutForm form, double *t_hot_end);
// Waits for the batch's kernels (*t_kernels_end; from here on the input set it used is free), then copies output set `out` to its pinned buffer:
// *text stays valid until the set is handed to pipe_compute again.
int pipe_stage_out(bwahip_ctx *c, int out, const char **text, int64_t *len, double *t_kernels_end);
// After pipe_stage_out of a batch computed as OutForm::BamSorted (coordinate-sorted records): the records' keys and offsets, valid as long as the
// text; *sort_ms: the GPU time of the sort stage (record table, radix sort, gather).
int pipe_stage_out_sorted(bwahip_ctx *c, int out, const uint64_t **keys, const int64_t **rec_off, int64_t *n_rec, double *sort_ms);
// After pipe_stage_out of a batch computed as OutForm::Bgzf (BGZF members, k_bgzf.hip): the uncompressed bytes of the records, the number of
// members and of stored ones, and the GPU time of the deflate stage.
int pipe_stage_out_bgzf(bwahip_ctx *c, int out, int64_t *raw_len, int64_t *n_blocks, int64_t *n_stored, double *deflate_ms);
// The stage-out of a batch computed as OutForm::BamSorted whose run stays in HBM (bwahip_stream_run_bam_sorted_dev): nothing is downloaded.  Waits for
// the batch's kernels (*t_kernels_end; the input set is free from here on), allocates the run's own device buffers and copies records,
// keys and offsets device to device on the copy stream (awaited: output set `out` is free on return).  *run == nullptr with a return of 0:
// the buffers could not be allocated -- the caller downloads the set with pipe_stage_out / pipe_stage_out_sorted instead.
int pipe_stage_out_devrun(bwahip_ctx *c, int out, DevRun **run, int64_t *raw_len, int64_t *n_rec, double *sort_ms, double *t_kernels_end);
// buffers freed and allocated again since the library was loaded (DevBuf / HostBuf ::ensure)
long pipe_realloc_count();
