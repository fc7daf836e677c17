"""ctypes binding of libbwahip.so -- the host-side mirror of the reference interface.

The product is the C-ABI shared library (include/bwahip.h); this module only makes it callable from
the Python test-suite and bench.py.  It never computes anything itself and it never falls back to a
CPU implementation: if the HIP library has not been built, importing the library fails loudly.

Mirrors: mem_opt_t / mem_opt_init (bwa.h:86, bwamem.c:74), mem_process_seqs (bwamem.h:69),
mem_align1_core (bwamem.c:1061) and the stage boundaries used by the parity tests.
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BWAHIP_LIB") or os.path.join(_HERE, "libbwahip.so")
TOOLS = os.path.join(_HERE, "tools")


class Opt(C.Structure):  # bwahip_opt_t == mem_opt_t (bwa.h:86-118)
    _fields_ = [("max_mem_intv", C.c_uint64), ("a", C.c_int), ("b", C.c_int), ("o_del", C.c_int), ("e_del", C.c_int),
                ("o_ins", C.c_int), ("e_ins", C.c_int), ("pen_unpaired", C.c_int), ("pen_clip5", C.c_int),
                ("pen_clip3", C.c_int), ("w", C.c_int), ("zdrop", C.c_int), ("T", C.c_int), ("flag", C.c_int),
                ("min_seed_len", C.c_int), ("min_chain_weight", C.c_int), ("max_chain_extend", C.c_int),
                ("split_factor", C.c_float), ("split_width", C.c_int), ("max_occ", C.c_int), ("max_chain_gap", C.c_int),
                ("n_threads", C.c_int), ("chunk_size", C.c_int), ("mask_level", C.c_float), ("drop_ratio", C.c_float),
                ("XA_drop_ratio", C.c_float), ("mask_level_redun", C.c_float), ("mapQ_coef_len", C.c_float),
                ("mapQ_coef_fac", C.c_int), ("max_ins", C.c_int), ("max_matesw", C.c_int), ("max_XA_hits", C.c_int),
                ("max_XA_hits_alt", C.c_int), ("mat", C.c_int8 * 25)]


class Seq(C.Structure):  # bwahip_seq_t == bseq1_t (bwa.h:58-63)
    _fields_ = [("l_seq", C.c_int), ("id", C.c_int), ("name", C.c_char_p), ("comment", C.c_char_p),
                ("seq", C.POINTER(C.c_char)), ("qual", C.c_char_p), ("sam", C.POINTER(C.c_char)),
                ("l_name", C.c_int8), ("l_comment", C.c_int8), ("l_qual", C.c_int16)]


class AlnReg(C.Structure):  # bwahip_alnreg_t == mem_alnreg_t (bwa.h:145-163)
    _fields_ = [("rb", C.c_int64), ("re", C.c_int64), ("hash", C.c_uint64), ("frac_rep", C.c_float),
                ("qb", C.c_int), ("qe", C.c_int), ("rid", C.c_int), ("score", C.c_int), ("truesc", C.c_int),
                ("sub", C.c_int), ("alt_sc", C.c_int), ("csub", C.c_int), ("sub_n", C.c_int), ("w", C.c_int),
                ("seedcov", C.c_int), ("secondary", C.c_int), ("secondary_all", C.c_int), ("seedlen0", C.c_int),
                ("n_comp", C.c_int, 30), ("is_alt", C.c_int, 2)]


class AlnRegV(C.Structure):
    _fields_ = [("n", C.c_int), ("m", C.c_int), ("a", C.POINTER(AlnReg))]


class Bwt(C.Structure):  # bwahip_bwt_t == bwt_t (bwt.h:48-60)
    _fields_ = [("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64), ("bwt_size", C.c_uint64),
                ("bwt", C.c_void_p), ("cnt_table", C.c_uint32 * 256), ("sa_intv", C.c_int), ("n_sa", C.c_uint64), ("sa", C.c_void_p)]


class Ann(C.Structure):  # bwahip_ann_t == bntann1_t (bntseq.h:41-48)
    _fields_ = [("offset", C.c_int64), ("len", C.c_int32), ("n_ambs", C.c_int32), ("gi", C.c_uint32), ("is_alt", C.c_int32),
                ("name", C.c_char_p), ("anno", C.c_char_p)]


class Bns(C.Structure):  # bwahip_bns_t == bntseq_t (bntseq.h:56-64)
    _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("seed", C.c_uint32), ("anns", C.POINTER(Ann)), ("n_holes", C.c_int32),
                ("ambs", C.c_void_p), ("fp_pac", C.c_void_p)]


class PeStat(C.Structure):
    _fields_ = [("low", C.c_int), ("high", C.c_int), ("failed", C.c_int), ("avg", C.c_double), ("std", C.c_double)]


class StreamStats(C.Structure):  # bwahip_stream_t
    _fields_ = [("chunk_bases", C.c_int64), ("max_reads", C.c_int64), ("keep_comments", C.c_int), ("reader_threads", C.c_int),
                ("n_reads", C.c_int64), ("n_batches", C.c_int64), ("sam_bytes", C.c_int64), ("seconds", C.c_double),
                ("reader_wait_s", C.c_double), ("gpu_busy_s", C.c_double), ("write_s", C.c_double)]


class SortStats(C.Structure):  # bwahip_sort_t
    _fields_ = [("tmp_dir", C.c_char_p), ("mem_budget", C.c_int64), ("n_records", C.c_int64), ("n_runs", C.c_int64), ("spilled_bytes", C.c_int64),
                ("sort_ms", C.c_double), ("merge_s", C.c_double)]


class BgzfStats(C.Structure):  # bwahip_bgzf_stats_t
    _fields_ = [("raw_bytes", C.c_int64), ("bgzf_bytes", C.c_int64), ("n_blocks", C.c_int64), ("n_stored", C.c_int64), ("deflate_ms", C.c_double)]


class DevMergeStats(C.Structure):  # bwahip_devmerge_stats_t
    _fields_ = [("n_records", C.c_int64), ("n_runs", C.c_int64), ("raw_bytes", C.c_int64), ("bgzf_bytes", C.c_int64), ("n_blocks", C.c_int64),
                ("n_stored", C.c_int64), ("hbm_bytes", C.c_int64), ("sort_ms", C.c_double), ("gather_ms", C.c_double), ("deflate_ms", C.c_double),
                ("finish_s", C.c_double)]


class SortDevStats(C.Structure):  # bwahip_sort_dev_t
    _fields_ = [("tmp_dir", C.c_char_p), ("mem_budget", C.c_int64), ("level", C.c_int), ("hbm_budget", C.c_int64), ("piece_blocks", C.c_int),
                ("fell_back", C.c_int), ("fell_back_at_run", C.c_int64), ("n_records", C.c_int64), ("n_runs", C.c_int64), ("spilled_bytes", C.c_int64),
                ("sort_ms", C.c_double), ("merge_s", C.c_double), ("dev", DevMergeStats)]


class BaiStats(C.Structure):  # bwahip_bai_stats_t
    _fields_ = [("n_chunks", C.c_int64), ("n_windows", C.c_int64), ("n_no_coor", C.c_int64), ("bai_bytes", C.c_int64), ("hbm_bytes", C.c_int64),
                ("index_ms", C.c_double)]


class DupDesc(C.Structure):  # bwahip_dup_desc_t
    _fields_ = [("end", C.c_uint64 * 2), ("score", C.c_uint32), ("kind", C.c_uint32)]


DUP_DESC_DTYPE = np.dtype([("end", np.uint64, (2,)), ("score", np.uint32), ("kind", np.uint32)])   # the same 24 bytes as a numpy record


class MarkdupStats(C.Structure):  # bwahip_markdup_stats_t
    _fields_ = [("n_templates", C.c_int64 * 3), ("n_dup_templates", C.c_int64 * 3), ("n_marked", C.c_int64), ("hbm_bytes", C.c_int64),
                ("markdup_ms", C.c_double), ("decide_ms", C.c_double), ("mark_ms", C.c_double)]


class QcOpt(C.Structure):  # bwahip_qc_opt_t
    _fields_ = [("window_shift", C.c_int), ("exclude_flags", C.c_int), ("min_mapq", C.c_int)]


class QcStats(C.Structure):  # bwahip_qc_stats_t
    _fields_ = [("n_windows", C.c_int64), ("qc_bytes", C.c_int64), ("hbm_bytes", C.c_int64), ("qc_ms", C.c_double), ("record_ms", C.c_double),
                ("scan_ms", C.c_double)]


class PileupOpt(C.Structure):  # bwahip_pileup_opt_t
    _fields_ = [("min_mapq", C.c_int), ("min_baseq", C.c_int), ("exclude_flags", C.c_int), ("min_alt", C.c_int)]


class PileupStats(C.Structure):  # bwahip_pileup_stats_t
    _fields_ = [("n_sites", C.c_int64), ("n_alleles", C.c_int64), ("n_obs", C.c_int64 * 3), ("pu_bytes", C.c_int64), ("hbm_bytes", C.c_int64),
                ("pileup_ms", C.c_double), ("observe_ms", C.c_double), ("sort_ms", C.c_double), ("evidence_ms", C.c_double)]


class RecalOpt(C.Structure):  # bwahip_recal_opt_t
    _fields_ = [("min_mapq", C.c_int), ("min_baseq", C.c_int), ("exclude_flags", C.c_int), ("max_cycle", C.c_int)]


class RecalStats(C.Structure):  # bwahip_recal_stats_t
    _fields_ = [("n_records", C.c_int64), ("n_bases", C.c_int64), ("n_err", C.c_int64), ("n_masked", C.c_int64), ("n_rows", C.c_int64 * 3), ("rc_bytes", C.c_int64),
                ("hbm_bytes", C.c_int64), ("recal_ms", C.c_double)]


class SpillStats(C.Structure):  # bwahip_spill_t
    _fields_ = [("host_budget", C.c_int64), ("tmp_dir", C.c_char_p), ("window_pieces", C.c_int), ("n_spilled_runs", C.c_int64), ("first_spilled_run", C.c_int64),
                ("host_bytes", C.c_int64), ("file_bytes", C.c_int64), ("n_windows", C.c_int64), ("window_hbm_bytes", C.c_int64), ("download_s", C.c_double),
                ("upload_ms", C.c_double)]


ERRORS = {0: "ok", -1: "EINVAL", -2: "ENODEV", -3: "ENOMEM", -4: "EIO", -5: "ECAPACITY", -6: "EINTERNAL"}

STAGE_INTV, STAGE_CHAIN, STAGE_CHAIN_FLT, STAGE_REGS, STAGE_REGS_PRE, STAGE_SEEDS = 1, 2, 3, 4, 5, 6
STAGE_PESTAT, STAGE_REGS_PE, STAGE_PAIR = 7, 8, 9        # bwahip_run_pe_stages
PE_PATHS = ("ahead_byte", "ahead_word", "inline_lds", "inline_slab", "incr_insert", "general_dedup", "big_pairs", "copy_big_pairs",
            "try_ff", "try_fr", "try_rf", "try_rr", "off_contig", "both_kernels")   # bwahip_last_pe_paths
TAG_READ = 100
# bwahip_kat_chain's per-read diagnostics (bwahip.h): columns, who took the read, which sort, which filter
CHAIN_DIAG_N = 8
CHAIN_BY_LANE, CHAIN_BY_HELPED = -1, 4                      # 0..3: the class of k_chain_big
CHAIN_SORT_NONE, CHAIN_SORT_LANE, CHAIN_SORT_WAVE, CHAIN_SORT_LANE_AREA, CHAIN_SORT_LANE_DEPTH = 0, 1, 2, 3, 4
CHAIN_FLT_NONE, CHAIN_FLT_SEQ, CHAIN_FLT_WAVE = 0, 1, 2
# known-answer DP entries (bwahip.h): forms of bwahip_kat_ksw_global, CIGAR words per item, path bits of bwahip_kat_ksw_extend2
KAT_GLOBAL_AUTO_SMALL, KAT_GLOBAL_AUTO_BIG, KAT_GLOBAL_SCORE_ONLY = 0, 1, 2
KAT_MAX_CIGAR = 512
KAT_MARK_TAG, KAT_MARK_WORDS = 41, 25                       # bwahip_kat_mark's record: 4 header words, then 25 per region
KAT_PAIR_TAG, KAT_PAIR_WORDS = 43, 22                       # bwahip_kat_pair's record: 12 header words, then 22 per region
# bwahip_kat_dedup (bwahip.h): forms, and the diag word -- who finished the read, handed over, one-lane sorts, why k_dedup_fast refused, counts
KAT_DEDUP_PRODUCT, KAT_DEDUP_FULL, KAT_DEDUP_SLAB = 0, 1, 2
KAT_DEDUP_FAST, KAT_DEDUP_STAGED, KAT_DEDUP_GLOBAL, KAT_DEDUP_SLABBED, KAT_DEDUP_HANDED, KAT_DEDUP_LANE1, KAT_DEDUP_LANE2 = 1, 2, 4, 8, 16, 32, 64
KAT_DEDUP_WHY_SHIFT, KAT_DEDUP_ALN_SHIFT, KAT_DEDUP_MRG_SHIFT = 7, 9, 20
KAT_DEDUP_WHY_TIE1, KAT_DEDUP_WHY_PATCH, KAT_DEDUP_WHY_TIE2 = 1, 2, 3
KAT_EXT_ROWS1, KAT_EXT_ROWS2, KAT_EXT_ROWS3, KAT_EXT_ROWS4, KAT_EXT_SHORT, KAT_EXT_WIDE, KAT_EXT_BEYOND16, KAT_EXT_STOPPED = 1, 2, 4, 8, 16, 32, 64, 128
KAT_EXT_DIAG = 256


class BwahipError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libbwahip.so.  There is no fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BwahipError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the hot path)")
    L = C.CDLL(LIB_PATH)
    vp, i64p, u64p, ip = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    L.bwahip_version.restype = C.c_char_p
    L.bwahip_opt_init.argtypes = [C.POINTER(Opt)]
    L.bwahip_opt_fill_scmat.argtypes = [C.POINTER(Opt)]
    L.bwahip_ctx_tune.argtypes = [vp, C.c_char_p, C.c_int]
    L.bwahip_kat_ksw_align.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bwahip_init_from_files.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.bwahip_rccl_unique_id.argtypes = [vp]
    L.bwahip_init_rccl.argtypes = [C.c_char_p, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.bwahip_ctx_clone.argtypes = [vp, C.POINTER(vp)]
    L.bwahip_ctx_clone_on.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.bwahip_stream_run.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Opt), C.POINTER(PeStat), C.c_char_p, C.c_char_p, C.c_int, C.POINTER(StreamStats)]
    L.bwahip_process_seqs_text.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, C.POINTER(Seq), C.c_void_p, C.POINTER(C.c_char_p), i64p, C.POINTER(i64p)]
    L.bwahip_process_seqs_bam.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, C.POINTER(Seq), C.c_void_p, C.POINTER(vp), i64p, C.POINTER(i64p)]
    L.bwahip_batch_run_bam.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.POINTER(PeStat), C.POINTER(C.c_float), C.c_int]
    L.bwahip_batch_bam.argtypes = [vp, C.POINTER(vp), i64p, vp]
    L.bwahip_bam_header.argtypes = [C.POINTER(Bns), C.c_char_p, C.POINTER(vp), i64p]
    L.bwahip_bgzf_write.argtypes = [C.c_int, vp, C.c_int64, C.c_int, C.c_int]
    L.bwahip_bgzf_eof.argtypes = [C.c_int]
    L.bwahip_bns.argtypes = [vp]
    L.bwahip_bns.restype = C.POINTER(Bns)
    L.bwahip_stream_run_bam.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Opt), C.POINTER(PeStat), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int,
                                        C.POINTER(StreamStats)]
    L.bwahip_process_seqs_bam_sorted.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, C.POINTER(Seq), C.c_void_p, C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp), i64p]
    L.bwahip_batch_run_bam_sorted.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.POINTER(PeStat), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float)]
    L.bwahip_batch_bam_sorted.argtypes = [vp, C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp), i64p]
    L.bwahip_bam_sort_key.argtypes = [C.POINTER(Bns), C.c_int32, C.c_int32, C.c_int]
    L.bwahip_bam_sort_key.restype = C.c_uint64
    L.bwahip_bam_sort_key_bits.argtypes = [C.POINTER(Bns)]
    L.bwahip_bam_sort_key_for.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int]
    L.bwahip_bam_sort_key_for.restype = C.c_uint64
    L.bwahip_bam_sort_key_bits_for.argtypes = [C.c_int32, C.c_int32]
    L.bwahip_bam_header_sorted.argtypes = [C.POINTER(Bns), C.c_char_p, C.POINTER(vp), i64p]
    L.bwahip_bam_merger_open.argtypes = [C.c_char_p, C.c_int64, C.POINTER(vp)]
    L.bwahip_bam_merger_add.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int64]
    L.bwahip_bam_merger_finish.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.bwahip_bam_merger_stats.argtypes = [vp, i64p, i64p, i64p, C.POINTER(C.c_double)]
    L.bwahip_bam_merger_close.argtypes = [vp]
    L.bwahip_bam_merger_close.restype = None
    L.bwahip_stream_run_bam_sorted.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Opt), C.POINTER(PeStat), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int,
                                               C.POINTER(StreamStats), C.POINTER(SortStats)]
    L.bwahip_bam_devmerger_open.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.bwahip_bam_devmerger_add.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int64]
    L.bwahip_bam_devmerger_finish.argtypes = [vp, C.c_int, C.POINTER(DevMergeStats)]
    L.bwahip_bam_devmerger_close.argtypes = [vp]
    L.bwahip_bam_devmerger_close.restype = None
    L.bwahip_bam_devmerge_hbm_need.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    L.bwahip_bam_devmerge_hbm_need.restype = C.c_int64
    # the ten leading arguments of every device-merged sorted entry point: contexts, options, files, header, the two stats structs
    sorted_dev = [C.POINTER(vp), C.c_int, C.POINTER(Opt), C.POINTER(PeStat), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(StreamStats), C.POINTER(SortDevStats)]
    L.bwahip_stream_run_bam_sorted_dev.argtypes = sorted_dev
    L.bwahip_kat_bgzf.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, i64p, i64p, i64p]
    L.bwahip_process_seqs_bgzf.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, C.POINTER(Seq), C.c_void_p, C.POINTER(vp), i64p, i64p, i64p]
    L.bwahip_batch_run_bgzf.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.POINTER(PeStat), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float)]
    L.bwahip_batch_bgzf.argtypes = [vp, C.POINTER(vp), i64p, i64p, i64p, i64p]
    L.bwahip_stream_run_bam_dev.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Opt), C.POINTER(PeStat), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p,
                                            C.POINTER(StreamStats), C.POINTER(BgzfStats)]
    L.bwahip_bai_builder_open.argtypes = [C.c_int32, C.c_int64, C.POINTER(vp)]
    L.bwahip_bai_builder_add_records.argtypes = [vp, vp, vp, C.c_int64]
    L.bwahip_bai_builder_add_members.argtypes = [vp, vp, C.c_int64]
    L.bwahip_bai_builder_finish.argtypes = [vp, C.c_int]
    L.bwahip_bai_builder_close.argtypes = [vp]
    L.bwahip_bai_builder_close.restype = None
    L.bwahip_bai_check_contigs.argtypes = [C.POINTER(Bns)]
    L.bwahip_bgzf_write_lens.argtypes = [C.c_int, vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int64, i64p]
    L.bwahip_bam_merger_finish_bai.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.bwahip_bam_devmerger_finish_bai.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_int32, C.POINTER(DevMergeStats), C.POINTER(BaiStats)]
    L.bwahip_kat_bai.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int32, vp, C.c_int64, i64p]
    L.bwahip_bam_devmerge_bai_hbm_need.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64]
    L.bwahip_bam_devmerge_bai_hbm_need.restype = C.c_int64
    L.bwahip_stream_run_bam_sorted_bai.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Opt), C.POINTER(PeStat), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int,
                                                   C.POINTER(StreamStats), C.POINTER(SortStats), C.c_int]
    L.bwahip_stream_run_bam_sorted_dev_bai.argtypes = sorted_dev + [C.c_int]
    L.bwahip_dup_end_word.argtypes = [C.c_int32, C.c_int32, C.c_int]
    L.bwahip_dup_end_word.restype = C.c_uint64
    L.bwahip_markdup_decide_host.argtypes = [vp, C.c_int64, vp]
    L.bwahip_process_seqs_bam_sorted_dup.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, C.POINTER(Seq), C.c_void_p, C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp), i64p,
                                                     C.POINTER(vp), C.POINTER(vp), i64p]
    L.bwahip_bam_devmerger_add_dup.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, C.c_int64]
    L.bwahip_bam_devmerger_finish_markdup.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_int32, C.POINTER(DevMergeStats), C.POINTER(BaiStats), C.POINTER(MarkdupStats)]
    L.bwahip_bam_devmerge_markdup_hbm_need.argtypes = [C.c_int64, C.c_int64]
    L.bwahip_bam_devmerge_markdup_hbm_need.restype = C.c_int64
    L.bwahip_stream_run_bam_sorted_dev_markdup.argtypes = sorted_dev + [C.c_int, C.POINTER(MarkdupStats)]
    L.bwahip_kat_dup_desc.argtypes = [vp, vp, vp, C.c_int64, C.c_int, vp]
    L.bwahip_kat_markdup.argtypes = [vp, vp, C.c_int64, vp]
    L.bwahip_kat_dup_desc_ms.argtypes = [vp]
    L.bwahip_kat_dup_desc_ms.restype = C.c_float
    L.bwahip_live_resources.argtypes = [i64p]
    L.bwahip_qc_builder_open.argtypes = [C.c_int32, vp, C.POINTER(QcOpt), C.POINTER(vp)]
    L.bwahip_qc_builder_add_records.argtypes = [vp, vp, vp, C.c_int64]
    L.bwahip_qc_builder_finish.argtypes = [vp, C.c_int]
    L.bwahip_qc_builder_close.argtypes = [vp]
    L.bwahip_qc_builder_close.restype = None
    L.bwahip_bam_merger_set_qc.argtypes = [vp, vp]
    L.bwahip_kat_qc.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, vp, C.POINTER(QcOpt), vp, C.c_int64, i64p]
    L.bwahip_bam_devmerger_set_qc.argtypes = [vp, C.POINTER(QcOpt), C.c_int32, vp, C.c_int, C.POINTER(QcStats)]
    L.bwahip_qc_hbm_need.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64]
    L.bwahip_qc_hbm_need.restype = C.c_int64
    L.bwahip_pileup_builder_open.argtypes = [C.c_int32, vp, vp, C.POINTER(PileupOpt), C.POINTER(vp)]
    L.bwahip_pileup_builder_add_records.argtypes = [vp, vp, vp, C.c_int64]
    L.bwahip_pileup_builder_finish.argtypes = [vp, C.c_int]
    L.bwahip_pileup_builder_close.argtypes = [vp]
    L.bwahip_pileup_builder_close.restype = None
    L.bwahip_kat_pileup.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, vp, vp, C.POINTER(PileupOpt), vp, C.c_int64, i64p]
    L.bwahip_bam_devmerger_set_pileup.argtypes = [vp, C.POINTER(PileupOpt), C.c_int32, vp, vp, C.c_int, C.POINTER(PileupStats)]
    L.bwahip_pileup_hbm_need.argtypes = [C.c_int64]
    L.bwahip_pileup_hbm_need.restype = C.c_int64
    L.bwahip_stream_run_bam_sorted_dev_pileup.argtypes = sorted_dev + [C.c_int, C.c_int, C.POINTER(MarkdupStats), C.POINTER(QcOpt), C.c_int,
                                                          C.POINTER(QcStats), C.POINTER(PileupOpt), C.c_int, C.POINTER(PileupStats)]
    L.bwahip_stream_run_bam_sorted_dev_qc.argtypes = sorted_dev + [C.c_int, C.POINTER(MarkdupStats), C.c_int, C.POINTER(QcOpt), C.c_int,
                                                      C.POINTER(QcStats)]
    L.bwahip_bam_devmerger_set_spill.argtypes = [vp, C.POINTER(SpillStats)]
    L.bwahip_bam_devmerger_add_spilled.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, C.c_int64]
    L.bwahip_bam_devmerger_spill_stats.argtypes = [vp, C.POINTER(SpillStats)]
    L.bwahip_bam_devmerge_spill_hbm_need.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int]
    L.bwahip_bam_devmerge_spill_hbm_need.restype = C.c_int64
    L.bwahip_stream_run_bam_sorted_dev_spill.argtypes = sorted_dev + [C.POINTER(SpillStats), C.c_int, C.c_int, C.POINTER(MarkdupStats),
                                                         C.POINTER(QcOpt), C.c_int, C.POINTER(QcStats)]
    L.bwahip_recal_builder_open.argtypes = [C.c_int32, vp, vp, vp, C.POINTER(RecalOpt), C.POINTER(vp)]
    L.bwahip_recal_builder_add_records.argtypes = [vp, vp, vp, C.c_int64]
    L.bwahip_recal_builder_finish.argtypes = [vp, C.c_int]
    L.bwahip_recal_builder_close.argtypes = [vp]
    L.bwahip_recal_builder_close.restype = None
    L.bwahip_kat_recal.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, vp, vp, vp, C.POINTER(RecalOpt), vp, C.c_int64, i64p]
    L.bwahip_bam_devmerger_set_recal.argtypes = [vp, C.POINTER(RecalOpt), C.c_int32, vp, vp, vp, C.c_int, C.POINTER(RecalStats)]
    L.bwahip_recal_hbm_need.argtypes = [C.c_int64, C.c_int, C.c_int]
    L.bwahip_recal_hbm_need.restype = C.c_int64
    L.bwahip_stream_run_bam_sorted_dev_recal.argtypes = sorted_dev + [C.POINTER(SpillStats), C.c_int, C.c_int, C.POINTER(MarkdupStats),
                                                         C.POINTER(QcOpt), C.c_int, C.POINTER(QcStats), C.POINTER(RecalOpt), vp, C.c_int, C.POINTER(RecalStats)]
    L.bwahip_kat_radix_sort.argtypes = [vp, C.c_int64, vp, C.c_int, vp, C.POINTER(C.c_int)]
    L.bwahip_fastq_open.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.bwahip_fastq_next.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(C.POINTER(Seq)), C.POINTER(C.c_int)]
    L.bwahip_fastq_close.argtypes = [vp]
    L.bwahip_fastq_close.restype = None
    L.bwahip_fastq_open_mt.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp)]
    L.bwahip_fastq_next_batch.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(vp), C.POINTER(C.POINTER(Seq)), C.POINTER(C.c_int)]
    L.bwahip_fastq_batch_seqs.argtypes = [vp, C.POINTER(C.c_int)]
    L.bwahip_fastq_batch_seqs.restype = C.POINTER(Seq)
    L.bwahip_fastq_batch_release.argtypes = [vp]
    L.bwahip_fastq_batch_release.restype = None
    L.bwahip_ctx_set_rg_id.argtypes = [vp, C.c_char_p]
    L.bwahip_init_device.argtypes = [C.POINTER(Bwt), C.POINTER(Bns), vp, C.c_int, C.POINTER(vp)]
    L.bwahip_destroy.argtypes = [vp]
    L.bwahip_run_stages.argtypes = [vp, C.POINTER(Opt), C.c_int, vp, vp, C.c_int, C.POINTER(i64p), i64p]
    L.bwahip_batch_upload.argtypes = [vp, C.c_int, vp, vp]
    L.bwahip_batch_attach.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int64]
    L.bwahip_batch_attach_text.argtypes = [vp, vp, vp, vp, vp]
    L.bwahip_batch_run_sam.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.POINTER(PeStat), C.POINTER(C.c_float), C.c_int]
    L.bwahip_batch_sam.argtypes = [vp, C.POINTER(vp), i64p, vp]
    L.bwahip_batch_run.argtypes = [vp, C.POINTER(Opt), C.POINTER(C.c_float), C.c_int]
    L.bwahip_batch_counters.argtypes = [vp, u64p, C.c_int]
    L.bwahip_kernel_name.restype = C.c_char_p
    L.bwahip_kat_introsort.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.bwahip_kat_mate_insert.argtypes = [vp, C.POINTER(Opt), C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.bwahip_kat_chain.argtypes = [vp, C.POINTER(Opt), C.c_int, vp, vp, vp, vp, vp, C.POINTER(i64p), i64p, vp]
    L.bwahip_kat_dedup.argtypes = [vp, C.POINTER(Opt), C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(C.c_int32)]
    L.bwahip_kat_mark.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.POINTER(i64p), i64p]
    L.bwahip_kat_pair.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, vp, vp, C.POINTER(PeStat), vp, C.c_int, C.POINTER(i64p), i64p]
    L.bwahip_kat_occ4.argtypes = [vp, C.c_int, vp, vp]
    L.bwahip_index_footprint.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.bwahip_kat_sa.argtypes = [vp, C.c_int, vp, vp]
    L.bwahip_kat_kmer_table.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.bwahip_kat_extend.argtypes = [vp, C.c_int, vp, vp, vp]
    L.bwahip_kat_ksw_extend.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.bwahip_kat_ksw_extend2.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bwahip_kat_ksw_extend2_diag.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bwahip_kat_ksw_global.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.bwahip_align_batch.argtypes = [vp, C.POINTER(Opt), C.c_int, C.POINTER(Seq), C.POINTER(AlnRegV)]
    L.bwahip_process_seqs.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, C.POINTER(Seq), C.POINTER(PeStat)]
    L.bwahip_batch_download.argtypes = [vp, C.POINTER(AlnRegV)]
    L.bwahip_last_pe_stats.argtypes = [vp, C.POINTER(PeStat), u64p]
    L.bwahip_last_pe_paths.argtypes = [vp, u64p, C.c_int]
    L.bwahip_run_pe_stages.argtypes = [vp, C.POINTER(Opt), C.c_int64, C.c_int, vp, vp, C.POINTER(PeStat), C.c_int, C.POINTER(i64p), i64p]
    L.bwahip_seqs_take_sam.argtypes = [C.POINTER(Seq), C.c_int, C.POINTER(vp), i64p]
    _lib = L
    return L


def big_bytes(ptr, n):
    """n bytes at ptr as a bytes object; ctypes.string_at takes a C int, and a batch's SAM text can exceed 2^31 bytes."""
    addr = ptr.value if hasattr(ptr, "value") else ptr
    if isinstance(addr, bytes):                                # a c_char_p: take the address of its buffer
        addr = C.cast(ptr, C.c_void_p).value
    if n <= 0:
        return b""
    return bytes((C.c_char * n).from_address(addr))


def _check(rc, what):
    if rc != 0:
        raise BwahipError(f"{what} failed: {ERRORS.get(rc, rc)}")


def _free(ptr):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(ptr)


def seq_array(names, seqs, quals=None, comments=None):
    """A bseq1_t array of ASCII reads for the process_seqs_*_array calls; returns (array, the buffers it points into).  The library
    converts the bases in place, so an array serves one call."""
    n = len(seqs)
    arr = (Seq * n)()
    keep = []
    for i in range(n):
        sb = C.create_string_buffer(bytes(seqs[i]), len(seqs[i]) + 1)
        keep.append(sb)
        arr[i].l_seq, arr[i].id = len(seqs[i]), i
        arr[i].name = bytes(names[i])
        arr[i].comment = bytes(comments[i]) if comments is not None and comments[i] is not None else None
        arr[i].seq = C.cast(sb, C.POINTER(C.c_char))
        arr[i].qual = bytes(quals[i]) if quals is not None and quals[i] is not None else None
    return arr, keep


def bam_header(bns, hdr_line=None):
    """bwahip_bam_header: the uncompressed BAM header (magic, text, reference table) of a Bns (or of a Context's index); no device."""
    if isinstance(bns, Context):
        bns = lib().bwahip_bns(bns._h).contents
    out, ln = C.c_void_p(), C.c_int64()
    if isinstance(hdr_line, str):
        hdr_line = hdr_line.encode()
    _check(lib().bwahip_bam_header(C.byref(bns), hdr_line, C.byref(out), C.byref(ln)), "bwahip_bam_header")
    b = big_bytes(out, ln.value)
    _free(out)
    return b


def _bns_of(bns):
    return lib().bwahip_bns(bns._h).contents if isinstance(bns, Context) else bns


def bam_header_sorted(bns, hdr_line=None):
    """bwahip_bam_header_sorted: bam_header with "@HD\tVN:1.6\tSO:coordinate" as the first line of the text; an @HD line in hdr_line: EINVAL."""
    out, ln = C.c_void_p(), C.c_int64()
    if isinstance(hdr_line, str):
        hdr_line = hdr_line.encode()
    _check(lib().bwahip_bam_header_sorted(C.byref(_bns_of(bns)), hdr_line, C.byref(out), C.byref(ln)), "bwahip_bam_header_sorted")
    b = big_bytes(out, ln.value)
    _free(out)
    return b


def bam_sort_key(bns, ref_id, pos, reverse):
    """bwahip_bam_sort_key: the coordinate-sort key of a record with this refID, pos and strand under the index's contig table; no device."""
    return int(lib().bwahip_bam_sort_key(C.byref(_bns_of(bns)), ref_id, pos, int(bool(reverse))))


def bam_sort_key_bits(bns):
    r = lib().bwahip_bam_sort_key_bits(C.byref(_bns_of(bns)))
    if r < 0:
        _check(r, "bwahip_bam_sort_key_bits")
    return r


def bam_sort_key_for(n_seqs, longest, ref_id, pos, reverse):
    """bwahip_bam_sort_key_for: bam_sort_key under any index with n_seqs contigs whose longest has `longest` bases."""
    return int(lib().bwahip_bam_sort_key_for(n_seqs, longest, ref_id, pos, int(bool(reverse))))


def bam_sort_key_bits_for(n_seqs, longest):
    r = lib().bwahip_bam_sort_key_bits_for(n_seqs, longest)
    if r < 0:
        _check(r, "bwahip_bam_sort_key_bits_for")
    return r


class BamMerger:
    """bwahip_bam_merger_*: sorted runs in (records, keys, record offsets), one coordinate-sorted BGZF stream out; no device."""

    def __init__(self, tmp_dir=None, mem_budget=1 << 30):
        self._h = C.c_void_p()
        _check(lib().bwahip_bam_merger_open(os.fsencode(tmp_dir) if tmp_dir is not None else None, mem_budget, C.byref(self._h)), "bwahip_bam_merger_open")

    def add(self, run_no, rec, keys, rec_off):
        rec = bytes(rec)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        _check(lib().bwahip_bam_merger_add(self._h, run_no, rec, len(rec), keys.ctypes.data, rec_off.ctypes.data, len(keys)), "bwahip_bam_merger_add")

    def finish(self, fd, level=1, n_threads=1):
        _check(lib().bwahip_bam_merger_finish(self._h, fd, level, n_threads), "bwahip_bam_merger_finish")

    def finish_bai(self, fd, builder, level=1, n_threads=1):
        """bwahip_bam_merger_finish_bai: finish with a BaiBuilder listening (the caller finishes the builder)."""
        _check(lib().bwahip_bam_merger_finish_bai(self._h, fd, level, n_threads, builder._h), "bwahip_bam_merger_finish_bai")

    def set_qc(self, builder):
        """bwahip_bam_merger_set_qc: finish and finish_bai feed this QcBuilder every record as it is emitted (None: nobody listens)."""
        self._qc = builder                                       # the builder outlives the merge
        _check(lib().bwahip_bam_merger_set_qc(self._h, builder._h if builder is not None else None), "bwahip_bam_merger_set_qc")

    def stats(self):
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        _check(lib().bwahip_bam_merger_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "bwahip_bam_merger_stats")
        return dict(n_records=a.value, n_runs=b.value, spilled_bytes=c.value, merge_s=d.value)

    def close(self):
        if self._h:
            lib().bwahip_bam_merger_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DevMerger:
    """bwahip_bam_devmerger_*: BamMerger with the runs in the context's HBM and the merge, the gather and the deflate on its device
    (csrc/k_bammerge.hip).  piece_blocks: BGZF blocks gathered and deflated at a time (0: the context's sorted_piece_blocks)."""

    def __init__(self, ctx, piece_blocks=0):
        self._h = C.c_void_p()
        self._ctx = ctx                                          # the context outlives the merger
        _check(lib().bwahip_bam_devmerger_open(ctx._h, piece_blocks, C.byref(self._h)), "bwahip_bam_devmerger_open")

    def add(self, run_no, rec, keys, rec_off):
        rec = bytes(rec)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        _check(lib().bwahip_bam_devmerger_add(self._h, run_no, rec, len(rec), keys.ctypes.data, rec_off.ctypes.data, len(keys)), "bwahip_bam_devmerger_add")

    def finish(self, fd=-1):
        """The members of all records on fd (no header, no EOF block); returns the filled DevMergeStats."""
        st = DevMergeStats()
        _check(lib().bwahip_bam_devmerger_finish(self._h, fd, C.byref(st)), "bwahip_bam_devmerger_finish")
        return st

    def add_dup(self, run_no, rec, keys, rec_off, tmpl, desc):
        """bwahip_bam_devmerger_add_dup: add, with the records' template indices (uint32) and the templates' descriptors (DUP_DESC_DTYPE)."""
        rec = bytes(rec)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        tmpl = np.ascontiguousarray(tmpl, dtype=np.uint32)
        desc = np.ascontiguousarray(desc, dtype=DUP_DESC_DTYPE)
        _check(lib().bwahip_bam_devmerger_add_dup(self._h, run_no, rec, len(rec), keys.ctypes.data, rec_off.ctypes.data, len(keys), tmpl.ctypes.data, desc.ctypes.data, len(desc)),
               "bwahip_bam_devmerger_add_dup")

    def finish_markdup(self, fd=-1, bai_fd=-1, first_member_offset=0, n_ref=-1):
        """bwahip_bam_devmerger_finish_markdup: duplicates marked in HBM (csrc/k_markdup.hip), then finish (n_ref < 0: no index) or
        finish_bai; returns (DevMergeStats, BaiStats, MarkdupStats)."""
        st, bs, ms = DevMergeStats(), BaiStats(), MarkdupStats()
        _check(lib().bwahip_bam_devmerger_finish_markdup(self._h, fd, bai_fd, first_member_offset, n_ref, C.byref(st), C.byref(bs), C.byref(ms)),
               "bwahip_bam_devmerger_finish_markdup")
        return st, bs, ms

    def set_qc(self, ref_len=None, qc_fd=-1, opt=()):
        """bwahip_bam_devmerger_set_qc: every later finish runs the QC stage (csrc/k_qc.hip) over the runs and writes the summary to qc_fd;
        opt = (window_shift, exclude_flags, min_mapq), () for the defaults; ref_len None disarms.  Returns the QcStats every armed finish fills."""
        if ref_len is None or opt is None:
            self._qc = None
            _check(lib().bwahip_bam_devmerger_set_qc(self._h, None, 0, None, -1, None), "bwahip_bam_devmerger_set_qc")
            return None
        o, lens, qs = qc_opt(*opt), np.ascontiguousarray(ref_len, dtype=np.int64), QcStats()
        _check(lib().bwahip_bam_devmerger_set_qc(self._h, C.byref(o), len(lens), lens.ctypes.data if len(lens) else None, qc_fd, C.byref(qs)), "bwahip_bam_devmerger_set_qc")
        self._qc = qs                                            # the merger writes into it
        return qs

    def set_pileup(self, ref_len=None, pac=None, pu_fd=-1, opt=()):
        """bwahip_bam_devmerger_set_pileup: every later finish runs the pileup stage (csrc/k_pileup.hip) over the runs and writes the file to
        pu_fd; pac: the packed reference of these contigs (bytes), None for the context's index; opt = (min_mapq, min_baseq, exclude_flags,
        min_alt), () for the defaults; ref_len None disarms.  Returns the PileupStats every armed finish fills."""
        if ref_len is None or opt is None:
            self._pu = None
            _check(lib().bwahip_bam_devmerger_set_pileup(self._h, None, 0, None, None, -1, None), "bwahip_bam_devmerger_set_pileup")
            return None
        o, lens, ps = pileup_opt(*opt), np.ascontiguousarray(ref_len, dtype=np.int64), PileupStats()
        pac = bytes(pac) if pac is not None else None
        _check(lib().bwahip_bam_devmerger_set_pileup(self._h, C.byref(o), len(lens), lens.ctypes.data if len(lens) else None, pac, pu_fd, C.byref(ps)),
               "bwahip_bam_devmerger_set_pileup")
        self._pu = ps                                            # the merger writes into it
        return ps

    def set_recal(self, ref_len=None, pac=None, mask=None, rc_fd=-1, opt=()):
        """bwahip_bam_devmerger_set_recal: every later finish runs the recalibration-table stage (csrc/k_recal.hip) over the records and writes
        the file to rc_fd; pac: the packed reference of these contigs (bytes), None for the context's index; mask: the known sites (bytes), None
        for none; opt = (min_mapq, min_baseq, exclude_flags, max_cycle), () for the defaults; ref_len None disarms.  Returns the RecalStats
        every armed finish fills."""
        if ref_len is None or opt is None:
            self._rc = None
            _check(lib().bwahip_bam_devmerger_set_recal(self._h, None, 0, None, None, None, -1, None), "bwahip_bam_devmerger_set_recal")
            return None
        o, lens, rs = recal_opt(*opt), np.ascontiguousarray(ref_len, dtype=np.int64), RecalStats()
        _check(lib().bwahip_bam_devmerger_set_recal(self._h, C.byref(o), len(lens), lens.ctypes.data if len(lens) else None, bytes(pac) if pac is not None else None,
                                                    bytes(mask) if mask is not None else None, rc_fd, C.byref(rs)), "bwahip_bam_devmerger_set_recal")
        self._rc = rs                                            # the merger writes into it
        return rs

    def finish_bai(self, fd=-1, bai_fd=-1, first_member_offset=0, n_ref=0):
        """bwahip_bam_devmerger_finish_bai: finish, and the BAI index of the sorted records on bai_fd (csrc/k_bai.hip); returns
        (DevMergeStats, BaiStats)."""
        st, bs = DevMergeStats(), BaiStats()
        _check(lib().bwahip_bam_devmerger_finish_bai(self._h, fd, bai_fd, first_member_offset, n_ref, C.byref(st), C.byref(bs)), "bwahip_bam_devmerger_finish_bai")
        return st, bs

    def set_spill(self, host_budget=0, tmp_dir=None, window_pieces=0):
        """bwahip_bam_devmerger_set_spill: before the first add; runs added with add_spilled keep their record bytes in a host-side store
        (pinned memory up to host_budget bytes, otherwise unlinked files in tmp_dir) and every finish stages them window by window
        (csrc/k_bamspill.hip); window_pieces <= 0: the default, 8."""
        sp = SpillStats()
        sp.host_budget, sp.tmp_dir, sp.window_pieces = host_budget, os.fsencode(tmp_dir) if tmp_dir is not None else None, window_pieces
        _check(lib().bwahip_bam_devmerger_set_spill(self._h, C.byref(sp)), "bwahip_bam_devmerger_set_spill")

    def add_spilled(self, run_no, rec, keys, rec_off, tmpl=None, desc=None):
        """bwahip_bam_devmerger_add_spilled: add (tmpl and desc None) or add_dup, the run held spilled."""
        rec = bytes(rec)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        t = np.ascontiguousarray(tmpl, dtype=np.uint32) if tmpl is not None else None
        d = np.ascontiguousarray(desc, dtype=DUP_DESC_DTYPE) if desc is not None else None
        _check(lib().bwahip_bam_devmerger_add_spilled(self._h, run_no, rec, len(rec), keys.ctypes.data, rec_off.ctypes.data, len(keys), t.ctypes.data if t is not None else None,
                                                      d.ctypes.data if d is not None else None, len(d) if d is not None else 0), "bwahip_bam_devmerger_add_spilled")

    def spill_stats(self):
        """bwahip_bam_devmerger_spill_stats: the SpillStats of the runs held and of the last finish."""
        sp = SpillStats()
        _check(lib().bwahip_bam_devmerger_spill_stats(self._h, C.byref(sp)), "bwahip_bam_devmerger_spill_stats")
        return sp

    def close(self):
        if self._h:
            lib().bwahip_bam_devmerger_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def bam_devmerge_hbm_need(raw_bytes, n_records, n_runs, piece_blocks):
    """bwahip_bam_devmerge_hbm_need: the HBM a device merger takes for these runs, finish included (no device)."""
    return lib().bwahip_bam_devmerge_hbm_need(raw_bytes, n_records, n_runs, piece_blocks)


def bam_devmerge_spill_hbm_need(resident_raw_bytes, spilled_raw_bytes, longest_record, n_records, n_runs, piece_blocks, window_pieces):
    """bwahip_bam_devmerge_spill_hbm_need: the HBM a device merger with spilled runs takes, finish included (no device)."""
    return lib().bwahip_bam_devmerge_spill_hbm_need(resident_raw_bytes, spilled_raw_bytes, longest_record, n_records, n_runs, piece_blocks, window_pieces)


def bam_devmerge_markdup_hbm_need(n_records, n_templates):
    """bwahip_bam_devmerge_markdup_hbm_need: the HBM duplicate marking adds to bam_devmerge_hbm_need (no device)."""
    return lib().bwahip_bam_devmerge_markdup_hbm_need(n_records, n_templates)


def recal_opt(min_mapq=0, min_baseq=0, exclude_flags=-1, max_cycle=0):
    """bwahip_recal_opt_t; the defaults resolve to 0, 0, 3844, 1024."""
    o = RecalOpt()
    o.min_mapq, o.min_baseq, o.exclude_flags, o.max_cycle = min_mapq, min_baseq, exclude_flags, max_cycle
    return o


def recal_hbm_need(sum_len, max_cycle=0, with_mask=False):
    """bwahip_recal_hbm_need: the HBM of the recalibration-table stage for contigs of sum_len bases in all (no device)."""
    return lib().bwahip_recal_hbm_need(sum_len, max_cycle, int(bool(with_mask)))


class _Builder:
    """What the builders of the files beside a sorted BAM file share: bwahip_<_what>_builder_add_records, _finish and _close on self._h."""
    _what = None

    def _call(self, name, *args):
        name = f"bwahip_{self._what}_builder_{name}"
        return getattr(lib(), name)(*args), name

    def add_records(self, rec, rec_off):
        rec = bytes(rec)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        _check(*self._call("add_records", self._h, rec, rec_off.ctypes.data, len(rec_off) - 1))

    def finish(self, fd=-1):
        _check(*self._call("finish", self._h, fd))

    def close(self):
        if self._h:
            self._call("close", self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class RecalBuilder(_Builder):
    """bwahip_recal_builder_*: the recalibration table (BRC\1) of BAM records fed in any cut and any order, for these contig lengths, this
    packed reference and this mask of known sites (None: none); no device.  opt = (min_mapq, min_baseq, exclude_flags, max_cycle), () for
    the defaults."""

    _what = "recal"

    def __init__(self, ref_len, pac, mask=None, opt=()):
        self._h = C.c_void_p()
        lens = np.ascontiguousarray(ref_len, dtype=np.int64)
        _check(lib().bwahip_recal_builder_open(len(lens), lens.ctypes.data if len(lens) else None, bytes(pac) if pac is not None else None,
                                               bytes(mask) if mask is not None else None, C.byref(recal_opt(*opt)), C.byref(self._h)), "bwahip_recal_builder_open")


def dup_end_word(ref_id, u5, reverse):
    """bwahip_dup_end_word: the end word of a mapped primary record (no device)."""
    return int(lib().bwahip_dup_end_word(ref_id, u5, int(bool(reverse))))


def markdup_decide_host(desc):
    """bwahip_markdup_decide_host: one byte per template, 1 = duplicate (the decision restated on the host; no device)."""
    desc = np.ascontiguousarray(desc, dtype=DUP_DESC_DTYPE)
    dup = np.zeros(max(1, len(desc)), dtype=np.uint8)
    _check(lib().bwahip_markdup_decide_host(desc.ctypes.data if len(desc) else None, len(desc), dup.ctypes.data), "bwahip_markdup_decide_host")
    return dup[:len(desc)]


def bam_devmerge_bai_hbm_need(n_records, n_blocks, n_ref, n_windows):
    """bwahip_bam_devmerge_bai_hbm_need: the HBM the index stage takes beside bam_devmerge_hbm_need (no device)."""
    return lib().bwahip_bam_devmerge_bai_hbm_need(n_records, n_blocks, n_ref, n_windows)


def qc_opt(window_shift=0, exclude_flags=-1, min_mapq=0):
    """bwahip_qc_opt_t; the defaults resolve to 14, 1796, 0."""
    o = QcOpt()
    o.window_shift, o.exclude_flags, o.min_mapq = window_shift, exclude_flags, min_mapq
    return o


def qc_hbm_need(n_ref, sum_len, n_windows, n_records):
    """bwahip_qc_hbm_need: the HBM the QC stage takes (no device)."""
    return lib().bwahip_qc_hbm_need(n_ref, sum_len, n_windows, n_records)


class QcBuilder(_Builder):
    """bwahip_qc_builder_*: the QC summary (BQC\1) of BAM records fed in any cut and any order, for these contig lengths; no device.
    opt = (window_shift, exclude_flags, min_mapq), () for the defaults."""

    _what = "qc"

    def __init__(self, ref_len, opt=()):
        self._h = C.c_void_p()
        lens = np.ascontiguousarray(ref_len, dtype=np.int64)
        _check(lib().bwahip_qc_builder_open(len(lens), lens.ctypes.data if len(lens) else None, C.byref(qc_opt(*opt)), C.byref(self._h)), "bwahip_qc_builder_open")


def pileup_opt(min_mapq=0, min_baseq=0, exclude_flags=-1, min_alt=0):
    """bwahip_pileup_opt_t; the defaults resolve to 0, 0, 1796, 2."""
    o = PileupOpt()
    o.min_mapq, o.min_baseq, o.exclude_flags, o.min_alt = min_mapq, min_baseq, exclude_flags, min_alt
    return o


def pileup_hbm_need(n_records):
    """bwahip_pileup_hbm_need: what is known of the pileup stage's HBM before the data (no device)."""
    return lib().bwahip_pileup_hbm_need(n_records)


class PileupBuilder(_Builder):
    """bwahip_pileup_builder_*: the pileup (BPU\1) of BAM records fed in any cut and any order, for these contig lengths and this packed
    reference; no device.  opt = (min_mapq, min_baseq, exclude_flags, min_alt), () for the defaults."""

    _what = "pileup"

    def __init__(self, ref_len, pac, opt=()):
        self._h = C.c_void_p()
        lens = np.ascontiguousarray(ref_len, dtype=np.int64)
        _check(lib().bwahip_pileup_builder_open(len(lens), lens.ctypes.data if len(lens) else None, bytes(pac) if pac is not None else None, C.byref(pileup_opt(*opt)),
                                                C.byref(self._h)), "bwahip_pileup_builder_open")


class BaiBuilder(_Builder):
    """bwahip_bai_builder_*: the BAI index of a coordinate-sorted BAM file from its records and the lengths of its BGZF members, fed
    in file order in any interleaving; no device."""

    _what = "bai"

    def __init__(self, n_ref, first_member_offset=0):
        self._h = C.c_void_p()
        _check(lib().bwahip_bai_builder_open(n_ref, first_member_offset, C.byref(self._h)), "bwahip_bai_builder_open")

    def add_members(self, member_len):
        member_len = np.ascontiguousarray(member_len, dtype=np.int32)
        _check(*self._call("add_members", self._h, member_len.ctypes.data, len(member_len)))


def bai_check_contigs(bns):
    """bwahip_bai_check_contigs: ECAPACITY for a contig table BAI cannot index (a contig above 2^29 bases); no device."""
    _check(lib().bwahip_bai_check_contigs(C.byref(_bns_of(bns))), "bwahip_bai_check_contigs")


def bgzf_write_lens(fd, data, level=1, n_threads=1, cap=None):
    """bwahip_bgzf_write_lens: bgzf_write that returns the lengths of the members it wrote (int32 array)."""
    data = bytes(data)
    cap = (len(data) + 65279) // 65280 if cap is None else cap
    lens = np.zeros(max(cap, 1), dtype=np.int32)
    n = C.c_int64()
    _check(lib().bwahip_bgzf_write_lens(fd, data, len(data), level, n_threads, lens.ctypes.data, cap, C.byref(n)), "bwahip_bgzf_write_lens")
    return lens[:n.value].copy()


def bgzf_write(fd, data, level=1, n_threads=1, eof=False):
    """bwahip_bgzf_write: data as BGZF blocks on fd; eof: the end-of-file block after them (bwahip_bgzf_eof)."""
    data = bytes(data)
    _check(lib().bwahip_bgzf_write(fd, data, len(data), level, n_threads), "bwahip_bgzf_write")
    if eof:
        _check(lib().bwahip_bgzf_eof(fd), "bwahip_bgzf_eof")


def live_resources():
    """(device buffers, device bytes, pinned buffers, pinned bytes, events, streams) the library owns in this process right now."""
    out = (C.c_int64 * 6)()
    _check(lib().bwahip_live_resources(out), "bwahip_live_resources")
    return tuple(out)


def default_opt():
    o = Opt()
    lib().bwahip_opt_init(C.byref(o))
    return o


NT4 = np.full(256, 4, dtype=np.uint8)
for _c, _v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
    NT4[_c] = _v
NT4[ord("-")] = 5


def pack_reads(reads):
    """list of ASCII/bytes reads -> (codes uint8 concatenated, offsets int64[n+1])."""
    lens = np.fromiter((len(r) for r in reads), dtype=np.int64, count=len(reads))
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    buf = b"".join(r if isinstance(r, bytes) else r.encode() for r in reads)
    codes = NT4[np.frombuffer(buf, dtype=np.uint8)] if buf else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(codes), off


def parse_records(words):
    """int64 record stream [tag, n, n values]* -> list of (tag, ndarray)."""
    out, i, n = [], 0, len(words)
    while i < n:
        tag, cnt = int(words[i]), int(words[i + 1])
        out.append((tag, words[i + 2:i + 2 + cnt]))
        i += 2 + cnt
    return out


def read_record_file(path):
    return parse_records(np.fromfile(path, dtype=np.int64))


class Context:
    """One GPU, one index resident in HBM (bwahip_ctx)."""

    def __init__(self, prefix, device=0):
        self._h = C.c_void_p()
        self._keep = None
        if prefix is not None:
            _check(lib().bwahip_init_from_files(os.fsencode(prefix), device, C.byref(self._h)), "bwahip_init_from_files")

    @classmethod
    def from_device_arrays(cls, meta, bwt_ptr, sa_ptr, pac_ptr, device=0):
        """Adopt index arrays that already sit in HBM (bwahip_init_device), e.g. after the RCCL broadcast."""
        self = cls(None, device)
        b = Bwt()
        b.primary = meta["primary"]
        for i in range(5):
            b.L2[i] = meta["L2"][i]
        b.seq_len, b.bwt_size, b.bwt = meta["seq_len"], meta["bwt_words"], bwt_ptr
        b.sa_intv, b.n_sa, b.sa = meta["sa_intv"], meta["n_sa"], sa_ptr
        anns = (Ann * len(meta["contigs"]))()
        for i, (name, off, ln, alt) in enumerate(meta["contigs"]):
            anns[i].offset, anns[i].len, anns[i].is_alt = off, ln, alt
            anns[i].name, anns[i].anno = name.encode(), b""
        n = Bns()
        n.l_pac, n.n_seqs, n.seed, n.anns = meta["l_pac"], len(meta["contigs"]), 11, anns
        self._keep = (b, anns, n)
        _check(lib().bwahip_init_device(C.byref(b), C.byref(n), pac_ptr, device, C.byref(self._h)), "bwahip_init_device")
        return self

    @staticmethod
    def rccl_unique_id():
        """128-byte ncclUniqueId (made on one rank; hand it to the others before from_rccl)."""
        buf = C.create_string_buffer(128)
        _check(lib().bwahip_rccl_unique_id(buf), "bwahip_rccl_unique_id")
        return buf.raw

    @classmethod
    def from_rccl(cls, prefix, rank, world, unique_id, device=0):
        """Collective: rank 0 loads `prefix`, all ranks receive the index over RCCL into their own HBM (bwahip_init_rccl)."""
        self = cls(None, device)
        idb = C.create_string_buffer(bytes(unique_id), 128)
        _check(lib().bwahip_init_rccl(os.fsencode(prefix) if prefix is not None else None, rank, world, idb, device, C.byref(self._h)), "bwahip_init_rccl")
        return self

    def clone(self):
        """A further context on the same GPU sharing this one's index in HBM (bwahip_ctx_clone); keep `self` alive longer."""
        other = Context(None)
        _check(lib().bwahip_ctx_clone(self._h, C.byref(other._h)), "bwahip_ctx_clone")
        other._keep = self
        return other

    def clone_on(self, device):
        """A context on another GPU with its own copy of the index, made device to device (bwahip_ctx_clone_on)."""
        other = Context(None)
        _check(lib().bwahip_ctx_clone_on(self._h, device, C.byref(other._h)), "bwahip_ctx_clone_on")
        other._keep = self
        return other

    def close(self):
        if self._h:
            lib().bwahip_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run_stages(self, codes, off, stages, opt=None):
        opt = opt or default_opt()
        mask = 0
        for s in stages:
            mask |= 1 << s
        out, n = C.POINTER(C.c_int64)(), C.c_int64()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        _check(lib().bwahip_run_stages(self._h, C.byref(opt), len(off) - 1, codes.ctypes.data, off.ctypes.data, mask,
                                       C.byref(out), C.byref(n)), "bwahip_run_stages")
        words = np.ctypeslib.as_array(out, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.int64)
        C.CDLL(None).free(out)
        return parse_records(words)

    def kat_chain(self, read_len, seed_off, seeds, intv_off, intv, opt=None):
        """bwahip_kat_chain: chaining and the chain filter on caller seed lists -- seeds [n x 4] (rbeg, qbeg, len, rid) in look-up order,
        intv [m x 3] (x[2], qbeg, qend), both by offsets per read.  -> (records: per read TAG_READ, STAGE_CHAIN, STAGE_CHAIN_FLT;
        diag [n_reads x CHAIN_DIAG_N]: who took the read (CHAIN_BY_*), nodes, height, sort (CHAIN_SORT_*), filter (CHAIN_FLT_*), chains)."""
        opt = opt or default_opt()
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        seed_off = np.ascontiguousarray(seed_off, dtype=np.int64); intv_off = np.ascontiguousarray(intv_off, dtype=np.int64)
        seeds = np.ascontiguousarray(seeds, dtype=np.int64).reshape(-1, 4); intv = np.ascontiguousarray(intv, dtype=np.int64).reshape(-1, 3)
        n = len(read_len)
        assert len(seed_off) == n + 1 and len(intv_off) == n + 1 and len(seeds) >= seed_off[-1] and len(intv) >= intv_off[-1]
        diag = np.zeros((n, CHAIN_DIAG_N), dtype=np.int32)
        out, m = C.POINTER(C.c_int64)(), C.c_int64()
        _check(lib().bwahip_kat_chain(self._h, C.byref(opt), n, read_len.ctypes.data, seed_off.ctypes.data, seeds.ctypes.data, intv_off.ctypes.data,
                                      intv.ctypes.data, C.byref(out), C.byref(m), diag.ctypes.data), "bwahip_kat_chain")
        words = np.ctypeslib.as_array(out, shape=(m.value,)).copy() if m.value else np.zeros(0, dtype=np.int64)
        C.CDLL(None).free(out)
        return parse_records(words), diag

    def kat_mark(self, reg_off, regs, opt=None, n_processed=0, plan=1, pairs=None):
        """bwahip_kat_mark: primary marking, -5, the selection and mapQ on caller region lists -- regs [m x 19] in the layout of STAGE_REGS,
        by offsets per read; plan 1 / 0: k_mark as the single-end / the paired-end path launches it; pairs: the pair indices the second of
        the paired-end path's two launches takes.  -> records: per read TAG_READ [i, n] and KAT_MARK_TAG [n, n_pri, tasks, records, then
        KAT_MARK_WORDS per region: the 19 words as marked, hash, input index, need, XA owner, mapQ, bad]."""
        opt = opt or default_opt()
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=np.int64).reshape(-1, 19)
        n = len(reg_off) - 1
        assert n >= 0 and (n == 0 or len(regs) >= reg_off[-1])
        n_pairs = 0 if pairs is None else len(pairs)
        pl = None if pairs is None else np.ascontiguousarray(list(pairs) + [0], dtype=np.int32)      # (never an empty array: its pointer says "a list was given")
        out, m = C.POINTER(C.c_int64)(), C.c_int64()
        _check(lib().bwahip_kat_mark(self._h, C.byref(opt), n_processed, n, reg_off.ctypes.data, regs.ctypes.data, plan,
                                     None if pl is None else pl.ctypes.data, n_pairs, C.byref(out), C.byref(m)), "bwahip_kat_mark")
        words = np.ctypeslib.as_array(out, shape=(m.value,)).copy() if m.value else np.zeros(0, dtype=np.int64)
        C.CDLL(None).free(out)
        return parse_records(words)

    def kat_pair(self, reg_off, regs, pes, opt=None, n_processed=0, pairs=None):
        """bwahip_kat_pair: mem_pair and the decisions of mem_sam_pe (k_pair) on caller region lists, reads 2p and 2p + 1 a pair -- regs
        [m x 19] as for kat_mark, pes: (PeStat * 4) or None, pairs: the pair indices the second of the two launches takes.  -> records: per
        read TAG_READ [i, n] and KAT_PAIR_TAG [the 8 words of STAGE_PAIR, n, n_pri, tasks, records, then KAT_PAIR_WORDS per region: the 19
        words as k_pair left them, input index, need, XA owner]."""
        opt = opt or default_opt()
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=np.int64).reshape(-1, 19)
        n = len(reg_off) - 1
        assert n >= 0 and (n == 0 or len(regs) >= reg_off[-1])
        n_pairs = 0 if pairs is None else len(pairs)
        pl = None if pairs is None else np.ascontiguousarray(list(pairs) + [0], dtype=np.int32)      # (never an empty array: its pointer says "a list was given")
        out, m = C.POINTER(C.c_int64)(), C.c_int64()
        _check(lib().bwahip_kat_pair(self._h, C.byref(opt), n_processed, n, reg_off.ctypes.data, regs.ctypes.data, pes,
                                     None if pl is None else pl.ctypes.data, n_pairs, C.byref(out), C.byref(m)), "bwahip_kat_pair")
        words = np.ctypeslib.as_array(out, shape=(m.value,)).copy() if m.value else np.zeros(0, dtype=np.int64)
        C.CDLL(None).free(out)
        return parse_records(words)

    def kat_dedup(self, codes, off, reg_off, regs, opt=None, heavy=None, form=KAT_DEDUP_PRODUCT, diag=True):
        """bwahip_kat_dedup: mem_sort_dedup_patch and the is_alt marking through the dedup kernels on caller region lists -- reads as codes by
        offsets, regs [m x 19] in the layout of STAGE_REGS by offsets per read (at least two per read), heavy[i]: read i enters the heavy
        reads' list; form KAT_DEDUP_*; diag False: the product's own instantiations.  -> (per read its final regions [n x 19], diag words
        [n_reads], number of reads handed over to the slab kernel)."""
        opt = opt or default_opt()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=np.int64).reshape(-1, 19)
        n = len(reg_off) - 1
        assert n >= 0 and len(off) == n + 1 and (n == 0 or (len(regs) >= reg_off[-1] and len(codes) >= off[-1]))
        hv = None if heavy is None else np.ascontiguousarray(heavy, dtype=np.uint8)
        assert hv is None or len(hv) == n
        out_n, dg = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
        out = np.zeros((len(regs) + 1, 19), dtype=np.int64)
        handed = C.c_int32(0)
        _check(lib().bwahip_kat_dedup(self._h, C.byref(opt), n, codes.ctypes.data, off.ctypes.data, reg_off.ctypes.data, regs.ctypes.data,
                                      None if hv is None else hv.ctypes.data, form, 1 if diag else 0, out_n.ctypes.data, out.ctypes.data, dg.ctypes.data,
                                      C.byref(handed)), "bwahip_kat_dedup")
        return [out[reg_off[i]:reg_off[i] + out_n[i]] for i in range(n)], dg[:n], handed.value

    def run_pe_stages(self, codes, off, stages, opt=None, n_processed=0, pes0=None):
        """bwahip_run_pe_stages: reads 2i, 2i+1 are a pair; -> records (STAGE_PESTAT first, then per read TAG_READ and the stages asked for)."""
        opt = opt or default_opt()
        mask = 0
        for s in stages:
            mask |= 1 << s
        out, n = C.POINTER(C.c_int64)(), C.c_int64()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        _check(lib().bwahip_run_pe_stages(self._h, C.byref(opt), n_processed, len(off) - 1, codes.ctypes.data, off.ctypes.data, pes0, mask,
                                          C.byref(out), C.byref(n)), "bwahip_run_pe_stages")
        words = np.ctypeslib.as_array(out, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.int64)
        C.CDLL(None).free(out)
        return parse_records(words)

    def last_pe_paths(self):
        """bwahip_last_pe_paths as a dict over PE_PATHS: which paths the paired-end kernels of the last batch took."""
        cnt = (C.c_uint64 * len(PE_PATHS))()
        _check(lib().bwahip_last_pe_paths(self._h, cnt, len(PE_PATHS)), "bwahip_last_pe_paths")
        return {k: int(cnt[i]) for i, k in enumerate(PE_PATHS)}

    def tune(self, **kw):
        """Set hand-off thresholds of the heavy-read kernels (bwahip_ctx_tune): intv_cap, smem_lanes, heavy_mult, ...; and
        ext_early_stop (default 1): ksw_extend2 ends once no later row can change its results; 0 = every row to the end, as the
        reference (same results, more rows); and ext_diag (default 1): ksw_extend2 answers a flank of at most K mismatches (1 at the default
        scores) from its main diagonal, without a DP row; 0 = every call runs its rows (same results); and incr_insert (default 1): mate rescue places a region into a tie-free list without
        sorting it again; 0 = every orientation ends in the full sort-and-dedup (same lists, pairing and output); and smem_skip (default -1):
        depth of k_smem's table jump, -1 = derived from the text length, 0 = off, n >= 2 = that depth (same intervals)."""
        for k, v in kw.items():
            _check(lib().bwahip_ctx_tune(self._h, k.encode(), int(v)), f"bwahip_ctx_tune({k})")

    def set_rg_id(self, rg_id):
        """Read-group id printed as RG:Z: on every record (bwa mem -R '@RG\\tID:<id>...', bwa_set_rg bwa.c:562); None / '' = none."""
        _check(lib().bwahip_ctx_set_rg_id(self._h, rg_id.encode() if rg_id else None), "bwahip_ctx_set_rg_id")

    def process_seqs(self, names, seqs, quals=None, opt=None, n_processed=0, pes0=None, comments=None):
        """mem_process_seqs: list of names / ASCII reads (/ quals) -> list of SAM text (bytes) per read."""
        opt = opt or default_opt()
        n = len(seqs)
        arr = (Seq * n)()
        keep = []
        for i in range(n):
            sb = C.create_string_buffer(bytes(seqs[i]), len(seqs[i]) + 1)
            keep.append(sb)
            arr[i].l_seq, arr[i].id = len(seqs[i]), i
            arr[i].name = bytes(names[i])
            arr[i].comment = bytes(comments[i]) if comments is not None and comments[i] is not None else None
            arr[i].seq = C.cast(sb, C.POINTER(C.c_char))
            arr[i].qual = bytes(quals[i]) if quals is not None else None
        _check(lib().bwahip_process_seqs(self._h, C.byref(opt), n_processed, n, arr, pes0), "bwahip_process_seqs")
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        out = []
        for i in range(n):
            out.append(C.string_at(arr[i].sam))
            libc.free(C.cast(arr[i].sam, C.c_void_p))
        return out

    def process_seqs_array(self, arr, n, opt=None, n_processed=0, pes0=None):
        """bwahip_process_seqs on a bseq1_t array (e.g. a FastqReader batch); returns the batch's SAM text (bwahip_seqs_take_sam)."""
        opt = opt or default_opt()
        _check(lib().bwahip_process_seqs(self._h, C.byref(opt), n_processed, n, arr, pes0), "bwahip_process_seqs")
        out, ln = C.c_void_p(), C.c_int64()
        _check(lib().bwahip_seqs_take_sam(arr, n, C.byref(out), C.byref(ln)), "bwahip_seqs_take_sam")
        sam = big_bytes(out, ln.value)
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        libc.free(out)
        return sam

    def process_seqs_text_array(self, arr, n, opt=None, n_processed=0, pes0=None, want_offsets=False):
        """bwahip_process_seqs_text on a bseq1_t array: the batch's SAM as one bytes object (copied out of the context's buffer)."""
        opt = opt or default_opt()
        sam, ln, off = C.c_char_p(), C.c_int64(), C.POINTER(C.c_int64)()
        _check(lib().bwahip_process_seqs_text(self._h, C.byref(opt), n_processed, n, arr, pes0, C.byref(sam), C.byref(ln), C.byref(off)), "bwahip_process_seqs_text")
        text = big_bytes(sam, ln.value)
        return (text, [off[i] for i in range(n + 1)]) if want_offsets else text

    def process_seqs_bam_array(self, arr, n, opt=None, n_processed=0, pes0=None, want_offsets=False):
        """bwahip_process_seqs_bam on a bseq1_t array: the batch's BAM records (no header, uncompressed) as one bytes object."""
        opt = opt or default_opt()
        bam, ln, off = C.c_void_p(), C.c_int64(), C.POINTER(C.c_int64)()
        _check(lib().bwahip_process_seqs_bam(self._h, C.byref(opt), n_processed, n, arr, pes0, C.byref(bam), C.byref(ln), C.byref(off)), "bwahip_process_seqs_bam")
        rec = big_bytes(bam, ln.value)
        return (rec, [off[i] for i in range(n + 1)]) if want_offsets else rec

    def process_seqs_bam(self, names, seqs, quals=None, opt=None, n_processed=0, pes0=None, comments=None, want_offsets=False):
        """The same from lists of names / ASCII reads (/ qualities, comments)."""
        arr, keep = seq_array(names, seqs, quals, comments)
        return self.process_seqs_bam_array(arr, len(seqs), opt, n_processed, pes0, want_offsets)

    def process_seqs_bam_sorted_array(self, arr, n, opt=None, n_processed=0, pes0=None):
        """bwahip_process_seqs_bam_sorted on a bseq1_t array: (records in coordinate order, keys as uint64 array, record offsets as int64 array)."""
        opt = opt or default_opt()
        bam, ln, keys, off, nr = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int64()
        _check(lib().bwahip_process_seqs_bam_sorted(self._h, C.byref(opt), n_processed, n, arr, pes0, C.byref(bam), C.byref(ln), C.byref(keys), C.byref(off), C.byref(nr)),
               "bwahip_process_seqs_bam_sorted")
        k = np.frombuffer(big_bytes(keys, nr.value * 8), dtype=np.uint64).copy()
        o = np.frombuffer(big_bytes(off, (nr.value + 1) * 8), dtype=np.int64).copy()
        return big_bytes(bam, ln.value), k, o

    def process_seqs_bam_sorted(self, names, seqs, quals=None, opt=None, n_processed=0, pes0=None, comments=None):
        """The same from lists of names / ASCII reads (/ qualities, comments)."""
        arr, keep = seq_array(names, seqs, quals, comments)
        return self.process_seqs_bam_sorted_array(arr, len(seqs), opt, n_processed, pes0)

    def process_seqs_bam_sorted_dup_array(self, arr, n, opt=None, n_processed=0, pes0=None):
        """bwahip_process_seqs_bam_sorted_dup: process_seqs_bam_sorted_array's three, then the records' template indices (uint32 array) and the
        templates' descriptors (DUP_DESC_DTYPE array)."""
        opt = opt or default_opt()
        bam, ln, keys, off, nr = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int64()
        tmpl, desc, nt = C.c_void_p(), C.c_void_p(), C.c_int64()
        _check(lib().bwahip_process_seqs_bam_sorted_dup(self._h, C.byref(opt), n_processed, n, arr, pes0, C.byref(bam), C.byref(ln), C.byref(keys), C.byref(off), C.byref(nr),
                                                        C.byref(tmpl), C.byref(desc), C.byref(nt)), "bwahip_process_seqs_bam_sorted_dup")
        k = np.frombuffer(big_bytes(keys, nr.value * 8), dtype=np.uint64).copy()
        o = np.frombuffer(big_bytes(off, (nr.value + 1) * 8), dtype=np.int64).copy()
        t = np.frombuffer(big_bytes(tmpl, nr.value * 4), dtype=np.uint32).copy()
        d = np.frombuffer(big_bytes(desc, nt.value * 24), dtype=DUP_DESC_DTYPE).copy()
        return big_bytes(bam, ln.value), k, o, t, d

    def process_seqs_bam_sorted_dup(self, names, seqs, quals=None, opt=None, n_processed=0, pes0=None, comments=None):
        """The same from lists of names / ASCII reads (/ qualities, comments)."""
        arr, keep = seq_array(names, seqs, quals, comments)
        return self.process_seqs_bam_sorted_dup_array(arr, len(seqs), opt, n_processed, pes0)

    def process_seqs_bgzf_array(self, arr, n, opt=None, n_processed=0, pes0=None):
        """bwahip_process_seqs_bgzf on a bseq1_t array: (the BGZF members of the batch's BAM records as one bytes object, the uncompressed
        bytes of the records, the number of members).  No file header, no end-of-file block."""
        opt = opt or default_opt()
        out, ln, raw, nb = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().bwahip_process_seqs_bgzf(self._h, C.byref(opt), n_processed, n, arr, pes0, C.byref(out), C.byref(ln), C.byref(raw), C.byref(nb)),
               "bwahip_process_seqs_bgzf")
        return big_bytes(out, ln.value), raw.value, nb.value

    def process_seqs_bgzf(self, names, seqs, quals=None, opt=None, n_processed=0, pes0=None, comments=None):
        """The same from lists of names / ASCII reads (/ qualities, comments)."""
        arr, keep = seq_array(names, seqs, quals, comments)
        return self.process_seqs_bgzf_array(arr, len(seqs), opt, n_processed, pes0)

    def last_pe_stats(self):
        """(pestat[4] as dicts, mate-rescue alignments run on the GPU, regions they added) of the last PE batch."""
        pes = (PeStat * 4)()
        cnt = (C.c_uint64 * 4)()
        _check(lib().bwahip_last_pe_stats(self._h, pes, cnt), "bwahip_last_pe_stats")
        self.pe_counters = dict(sw=int(cnt[0]), added=int(cnt[1]), max_sw_per_pair=int(cnt[2]), pairs_rescued=int(cnt[3]))
        return [dict(low=p.low, high=p.high, failed=p.failed, avg=p.avg, std=p.std) for p in pes], int(cnt[0]), int(cnt[1])

    def batch_upload(self, codes, off):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        _check(lib().bwahip_batch_upload(self._h, len(off) - 1, codes.ctypes.data, off.ctypes.data), "bwahip_batch_upload")

    def batch_attach(self, n, seq_ptr, off_ptr, max_len, total_bases):
        """Use reads already resident in HBM (device pointers); nothing is copied."""
        _check(lib().bwahip_batch_attach(self._h, n, seq_ptr, off_ptr, max_len, total_bases), "bwahip_batch_attach")

    def batch_attach_text(self, qual_ptr, qual_off_ptr, names_ptr, name_off_ptr):
        _check(lib().bwahip_batch_attach_text(self._h, qual_ptr, qual_off_ptr, names_ptr, name_off_ptr), "bwahip_batch_attach_text")

    def batch_run_sam(self, opt=None, n_processed=0, pes0=None):
        """Hot path + finalisation + SAM text, all on the GPU, over the attached batch; returns per-stage milliseconds."""
        opt = opt or default_opt()
        nk = lib().bwahip_n_kernels()
        ms = (C.c_float * nk)()
        _check(lib().bwahip_batch_run_sam(self._h, C.byref(opt), n_processed, pes0, ms, nk), "bwahip_batch_run_sam")
        return {lib().bwahip_kernel_name(i).decode(): float(ms[i]) for i in range(nk)}

    def batch_sam(self):
        out, ln = C.c_void_p(), C.c_int64()
        _check(lib().bwahip_batch_sam(self._h, C.byref(out), C.byref(ln), None), "bwahip_batch_sam")
        sam = big_bytes(out, ln.value)
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        libc.free(out)
        return sam

    def batch_run_bam(self, opt=None, n_processed=0, pes0=None):
        """batch_run_sam with BAM records as the output (the same kernel_ms slots)."""
        opt = opt or default_opt()
        nk = lib().bwahip_n_kernels()
        ms = (C.c_float * nk)()
        _check(lib().bwahip_batch_run_bam(self._h, C.byref(opt), n_processed, pes0, ms, nk), "bwahip_batch_run_bam")
        return {lib().bwahip_kernel_name(i).decode(): float(ms[i]) for i in range(nk)}

    def batch_bam(self):
        out, ln = C.c_void_p(), C.c_int64()
        _check(lib().bwahip_batch_bam(self._h, C.byref(out), C.byref(ln), None), "bwahip_batch_bam")
        rec = big_bytes(out, ln.value)
        _free(out)
        return rec

    def batch_run_bam_sorted(self, opt=None, n_processed=0, pes0=None):
        """batch_run_bam with the records in coordinate order; the stage milliseconds gain sort_table / sort_radix / sort_gather and
        sort_passes (the radix passes that ran)."""
        opt = opt or default_opt()
        nk = lib().bwahip_n_kernels()
        ms, sm = (C.c_float * nk)(), (C.c_float * 4)()
        _check(lib().bwahip_batch_run_bam_sorted(self._h, C.byref(opt), n_processed, pes0, ms, nk, sm), "bwahip_batch_run_bam_sorted")
        d = {lib().bwahip_kernel_name(i).decode(): float(ms[i]) for i in range(nk)}
        d.update(sort_table=float(sm[0]), sort_radix=float(sm[1]), sort_gather=float(sm[2]), sort_passes=int(sm[3]))
        return d

    def batch_bam_sorted(self):
        """(records, keys, record offsets) of the last batch_run_bam_sorted."""
        out, ln, keys, off, nr = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int64()
        _check(lib().bwahip_batch_bam_sorted(self._h, C.byref(out), C.byref(ln), C.byref(keys), C.byref(off), C.byref(nr)), "bwahip_batch_bam_sorted")
        rec = big_bytes(out, ln.value)
        k = np.frombuffer(big_bytes(keys, nr.value * 8), dtype=np.uint64).copy()
        o = np.frombuffer(big_bytes(off, (nr.value + 1) * 8), dtype=np.int64).copy()
        for p in (out, keys, off):
            _free(p)
        return rec, k, o

    def batch_run_bgzf(self, opt=None, n_processed=0, pes0=None):
        """batch_run_bam with the records deflated into BGZF members on the GPU (they stay in HBM); the stage milliseconds gain
        `deflate`, the deflate stage by HIP events."""
        opt = opt or default_opt()
        nk = lib().bwahip_n_kernels()
        ms, dm = (C.c_float * nk)(), C.c_float()
        _check(lib().bwahip_batch_run_bgzf(self._h, C.byref(opt), n_processed, pes0, ms, nk, C.byref(dm)), "bwahip_batch_run_bgzf")
        d = {lib().bwahip_kernel_name(i).decode(): float(ms[i]) for i in range(nk)}
        d["deflate"] = float(dm.value)
        return d

    def batch_bgzf(self):
        """(members, uncompressed bytes, members, stored members) of the last batch_run_bgzf."""
        out, ln, raw, nb, ns = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().bwahip_batch_bgzf(self._h, C.byref(out), C.byref(ln), C.byref(raw), C.byref(nb), C.byref(ns)), "bwahip_batch_bgzf")
        data = big_bytes(out, ln.value)
        _free(out)
        return data, raw.value, nb.value, ns.value

    def kat_bgzf(self, data):
        """(members, n_blocks, n_stored): the product's deflate stage (csrc/k_bgzf.hip) on these bytes, cut every 65 280."""
        data = bytes(data)
        cap = max(1, (len(data) + 65279) // 65280 * 65536)
        out = np.empty(cap, dtype=np.uint8)
        src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        ln, nb, ns = C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().bwahip_kat_bgzf(self._h, src.ctypes.data, len(data), out.ctypes.data, cap if data else 0, C.byref(ln), C.byref(nb), C.byref(ns)), "bwahip_kat_bgzf")
        return out[:ln.value].tobytes(), nb.value, ns.value

    def kat_bai(self, rec, rec_off, member_len, first_member_offset, n_ref):
        """The index stage of the device merger (csrc/k_bai.hip) on these records (file order) and member lengths: the .bai bytes."""
        rec = bytes(rec)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        member_len = np.ascontiguousarray(member_len, dtype=np.int32)
        src = np.frombuffer(rec, dtype=np.uint8) if rec else np.zeros(1, dtype=np.uint8)
        ln = C.c_int64()
        out = np.empty(1 << 20, dtype=np.uint8)
        for _ in range(2):
            rc = lib().bwahip_kat_bai(self._h, src.ctypes.data, rec_off.ctypes.data, len(rec_off) - 1, member_len.ctypes.data, len(member_len), first_member_offset, n_ref,
                                      out.ctypes.data, len(out), C.byref(ln))
            if rc != -5 or ln.value <= len(out):
                break
            out = np.empty(ln.value, dtype=np.uint8)                # the first answer said how much it takes
        _check(rc, "bwahip_kat_bai")
        return out[:ln.value].tobytes()

    def kat_qc(self, rec, rec_off, ref_len, opt=()):
        """The QC stage of the device merger (csrc/k_qc.hip) on these records (any order) for these contig lengths: the BQC\1 bytes.
        opt = (window_shift, exclude_flags, min_mapq), () for the defaults."""
        rec = bytes(rec)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        lens = np.ascontiguousarray(ref_len, dtype=np.int64)
        src = np.frombuffer(rec, dtype=np.uint8) if rec else np.zeros(1, dtype=np.uint8)
        ln = C.c_int64()
        out = np.empty(1 << 20, dtype=np.uint8)
        for _ in range(2):
            rc = lib().bwahip_kat_qc(self._h, src.ctypes.data, rec_off.ctypes.data, len(rec_off) - 1, len(lens), lens.ctypes.data if len(lens) else None, C.byref(qc_opt(*opt)),
                                     out.ctypes.data, len(out), C.byref(ln))
            if rc != -5 or ln.value <= len(out):
                break
            out = np.empty(ln.value, dtype=np.uint8)                # the first answer said how much it takes
        _check(rc, "bwahip_kat_qc")
        return out[:ln.value].tobytes()

    def kat_pileup(self, rec, rec_off, ref_len, pac, opt=()):
        """The pileup stage of the device merger (csrc/k_pileup.hip) on these records (any order) for these contig lengths and this packed
        reference: the BPU\1 bytes.  opt = (min_mapq, min_baseq, exclude_flags, min_alt), () for the defaults."""
        rec = bytes(rec)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        lens = np.ascontiguousarray(ref_len, dtype=np.int64)
        src = np.frombuffer(rec, dtype=np.uint8) if rec else np.zeros(1, dtype=np.uint8)
        ln = C.c_int64()
        out = np.empty(1 << 20, dtype=np.uint8)
        for _ in range(2):
            rc = lib().bwahip_kat_pileup(self._h, src.ctypes.data, rec_off.ctypes.data, len(rec_off) - 1, len(lens), lens.ctypes.data if len(lens) else None,
                                         bytes(pac) if pac is not None else None, C.byref(pileup_opt(*opt)), out.ctypes.data, len(out), C.byref(ln))
            if rc != -5 or ln.value <= len(out):
                break
            out = np.empty(ln.value, dtype=np.uint8)                # the first answer said how much it takes
        _check(rc, "bwahip_kat_pileup")
        return out[:ln.value].tobytes()

    def kat_recal(self, rec, rec_off, ref_len, pac, mask=None, opt=()):
        """The recalibration-table stage of the device merger (csrc/k_recal.hip) on these records (any order) for these contig lengths, this
        packed reference and this mask of known sites (None: none): the BRC\1 bytes.  opt = (min_mapq, min_baseq, exclude_flags, max_cycle),
        () for the defaults."""
        rec = bytes(rec)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        lens = np.ascontiguousarray(ref_len, dtype=np.int64)
        src = np.frombuffer(rec, dtype=np.uint8) if rec else np.zeros(1, dtype=np.uint8)
        ln = C.c_int64()
        out = np.empty(1 << 20, dtype=np.uint8)
        for _ in range(2):
            rc = lib().bwahip_kat_recal(self._h, src.ctypes.data, rec_off.ctypes.data, len(rec_off) - 1, len(lens), lens.ctypes.data if len(lens) else None,
                                        bytes(pac) if pac is not None else None, bytes(mask) if mask is not None else None, C.byref(recal_opt(*opt)), out.ctypes.data,
                                        len(out), C.byref(ln))
            if rc != -5 or ln.value <= len(out):
                break
            out = np.empty(ln.value, dtype=np.uint8)                # the first answer said how much it takes
        _check(rc, "bwahip_kat_recal")
        return out[:ln.value].tobytes()

    def kat_dup_desc(self, rec, off, paired=False):
        """The batch's descriptor kernel (csrc/k_markdup.hip) on these records in input order: read i = rec[off[i]:off[i+1]]; one
        descriptor per read, or per two reads (paired), as a DUP_DESC_DTYPE array."""
        rec = bytes(rec)
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        src = np.frombuffer(rec, dtype=np.uint8) if rec else np.zeros(1, dtype=np.uint8)
        desc = np.zeros(max(1, n // 2 if paired else n), dtype=DUP_DESC_DTYPE)
        _check(lib().bwahip_kat_dup_desc(self._h, src.ctypes.data, off.ctypes.data, n, int(bool(paired)), desc.ctypes.data), "bwahip_kat_dup_desc")
        return desc[:n // 2 if paired else n]

    def kat_dup_desc_ms(self):
        """The descriptor kernel's GPU milliseconds in the last kat_dup_desc (HIP events around the kernel alone)."""
        return float(lib().bwahip_kat_dup_desc_ms(self._h))

    def kat_markdup(self, desc):
        """The decision stage of a marked finish (csrc/k_markdup.hip) on these descriptors: one byte per template, 1 = duplicate."""
        desc = np.ascontiguousarray(desc, dtype=DUP_DESC_DTYPE)
        dup = np.zeros(max(1, len(desc)), dtype=np.uint8)
        _check(lib().bwahip_kat_markdup(self._h, desc.ctypes.data if len(desc) else None, len(desc), dup.ctypes.data), "bwahip_kat_markdup")
        return dup[:len(desc)]

    def kat_radix_sort(self, keys, key_bits=64):
        """(permutation, tile): the product's stable radix sort on these uint64 keys; tile = items one workgroup ranks per pass."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        idx = np.empty(len(keys), dtype=np.uint32)
        tile = C.c_int()
        _check(lib().bwahip_kat_radix_sort(self._h, len(keys), keys.ctypes.data, key_bits, idx.ctypes.data, C.byref(tile)), "bwahip_kat_radix_sort")
        return idx, tile.value

    def batch_run(self, opt=None):
        opt = opt or default_opt()
        nk = lib().bwahip_n_kernels()
        ms = (C.c_float * nk)()
        _check(lib().bwahip_batch_run(self._h, C.byref(opt), ms, nk), "bwahip_batch_run")
        return {lib().bwahip_kernel_name(i).decode(): float(ms[i]) for i in range(nk)}

    @staticmethod
    def stage_names():
        return ["k_smem(passes 1-2)+k_smem_heavy+k_smem3(pass 3)+k_intv_sort", "k_seeds", "k_chain(+k_chain_big,k_chain_flt)", "k_seed_sw (only with -W / reads > 700 bp)",
                "k_extend_spec+k_extend(+k_extend_big, dedup/patch)", "pe_rescue = PE: k_pestat + k_pe_prepare + k_pe_copy (insert sizes, lists; the rescue kernels k_matesw_sw / k_matesw start on the second stream)",
                "k_mark (mark primary) + PE: k_pair (pairing) beside the rescue kernels, then both for the rescued pairs",
                "k_cigar (mem_reg2aln: mapQ, CIGAR by ksw_global2 backtrack, NM/MD)", "k_sam size + scan + write (SAM text)"]

    @staticmethod
    def output_description(paired):
        return "SAM text of the batch in HBM (== seqs[i].sam of mem_process_seqs, " + ("paired-end: mate rescue, pairing, paired records)" if paired else "single-end)")

    def counters(self):
        buf = (C.c_uint64 * 32)()
        _check(lib().bwahip_batch_counters(self._h, buf, 32), "bwahip_batch_counters")
        names = ["extend", "blocks", "sa", "lf", "intv", "seeds", "cells", "max_extends", "chain_build_max", "chain_sort_max", "chain_flt_max",
                 "chain_write_max", "max_seeds", "max_chains", "ext_max", "ext_dedup_max", "heavy_blocks", "heavy_intv", "heavy_reads",
                 "dp_rows_1col", "dp_rows_ncol", "dedup_sort1_max", "dedup_loop_max", "dedup_sort2_max",
                 "pass3_blocks", "pass3_intv", "pass3_jumped", "ext_calls", "ext_diag", "smem_lookups", "smem_fallbacks", "_31"]
        return {k: int(buf[i]) for i, k in enumerate(names)}

    def kat_introsort(self, k64, score, qb, mode):
        """(idx_par, idx_seq, ran_parallel): the wavefront's exact introsort and the one-lane restatement of ksort.h on the same keys."""
        k64 = np.ascontiguousarray(k64, dtype=np.int64); score = np.ascontiguousarray(score, dtype=np.int32); qb = np.ascontiguousarray(qb, dtype=np.int32)
        n = len(k64)
        a = np.empty(n, dtype=np.int32); b = np.empty(n, dtype=np.int32); st = np.zeros(2, dtype=np.int32)
        _check(lib().bwahip_kat_introsort(self._h, n, mode, k64.ctypes.data, score.ctypes.data, qb.ctypes.data, a.ctypes.data, b.ctypes.data, st.ctypes.data), "bwahip_kat_introsort")
        assert st[1] == 0
        return a, b, bool(st[0])

    def kat_mate_insert(self, list_off, list_words, step_off, step_hit, step_words, opt=None, mode=0, where=0):
        """bwahip_kat_mate_insert: the list update of mate rescue on caller lists (19 words per region, the layout of STAGE_REGS_PE).
        mode 0: as shipped, 1: never incremental; where 0: LDS up to 224 regions of capacity, 1: global memory always.
        -> (out_words [capacity x 19, item i from row list_off[i] + step_off[i]], out_n, out_cnt [n_items x 3: by incr_insert, by score, full passes])."""
        opt = opt or default_opt()
        list_off = np.ascontiguousarray(list_off, dtype=np.int64); step_off = np.ascontiguousarray(step_off, dtype=np.int64)
        list_words = np.ascontiguousarray(list_words, dtype=np.int64).reshape(-1, 19); step_words = np.ascontiguousarray(step_words, dtype=np.int64).reshape(-1, 19)
        step_hit = np.ascontiguousarray(step_hit, dtype=np.int32)
        n = len(list_off) - 1
        assert len(step_off) == n + 1 and len(list_words) >= list_off.max() and len(step_words) >= step_off.max() and len(step_hit) == len(step_words)
        out = np.zeros((max(0, int(list_off[-1] + step_off[-1])), 19), dtype=np.int64); out_n = np.zeros(n, dtype=np.int32); cnt = np.zeros((n, 3), dtype=np.int32)
        _check(lib().bwahip_kat_mate_insert(self._h, C.byref(opt), n, list_off.ctypes.data, list_words.ctypes.data, step_off.ctypes.data, step_hit.ctypes.data, step_words.ctypes.data,
                                            mode, where, out.ctypes.data, out_n.ctypes.data, cnt.ctypes.data), "bwahip_kat_mate_insert")
        return out, out_n, cnt

    def kat_occ4(self, k):
        k = np.ascontiguousarray(k, dtype=np.uint64)
        out = np.zeros((len(k), 4), dtype=np.uint64)
        _check(lib().bwahip_kat_occ4(self._h, len(k), k.ctypes.data, out.ctypes.data), "bwahip_kat_occ4")
        return out

    def kat_sa(self, k):
        k = np.ascontiguousarray(k, dtype=np.uint64)
        out = np.zeros(len(k), dtype=np.uint64)
        _check(lib().bwahip_kat_sa(self._h, len(k), k.ctypes.data, out.ctypes.data), "bwahip_kat_sa")
        return out

    def index_footprint(self):
        """{'sa_intv', 'kmer_k', 'bwt_gb', 'sa_gb', 'pac_gb', 'interval_table_gb'} of the index in HBM (bwahip_index_footprint)."""
        a, k, b = C.c_int(), C.c_int(), (C.c_uint64 * 4)()
        _check(lib().bwahip_index_footprint(self._h, C.byref(a), C.byref(k), b), "bwahip_index_footprint")
        return {"sa_intv": a.value, "kmer_k": k.value, "bwt_gb": round(b[0] / 1e9, 2), "sa_gb": round(b[1] / 1e9, 2), "pac_gb": round(b[2] / 1e9, 2),
                "interval_table_gb": round(b[3] / 1e9, 2)}

    def kat_kmer_table(self):
        """(K, mismatches): the interval table against forward bwt_extend calls (bwahip_kat_kmer_table)."""
        k, bad = C.c_int(), C.c_uint64()
        _check(lib().bwahip_kat_kmer_table(self._h, C.byref(k), C.byref(bad)), "bwahip_kat_kmer_table")
        return k.value, bad.value

    def kat_ksw_extend(self, params, q, qoff, t, toff):
        params = np.ascontiguousarray(params, dtype=np.int32)
        q, t = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)
        qoff, toff = np.ascontiguousarray(qoff, dtype=np.int64), np.ascontiguousarray(toff, dtype=np.int64)
        out = np.zeros((len(params), 6), dtype=np.int32)
        _check(lib().bwahip_kat_ksw_extend(self._h, len(params), params.ctypes.data, q.ctypes.data, qoff.ctypes.data, t.ctypes.data,
                                           toff.ctypes.data, out.ctypes.data), "bwahip_kat_ksw_extend")
        return out

    def kat_ksw_extend2(self, params, mat, q, qoff, t, toff, diag=False):
        """ksw_extend2 at a given number of columns per lane (bwahip_kat_ksw_extend2); params n x 12 (qlen, tlen, w, h0, zdrop, end_bonus,
        o_del, e_del, o_ins, e_ins, reverse, cpl), mat n x 25 -> n x 7 (six results, path mask KAT_EXT_*; KAT_EXT_STOPPED: the early
        stop ended the loop -- the entry follows the context's ext_early_stop).  diag: bwahip_kat_ksw_extend2_diag, the call as the
        extension kernels make it -- the diagonal rule first (knob ext_diag), KAT_EXT_DIAG alone in the mask of a call it answered."""
        params = np.ascontiguousarray(params, dtype=np.int32).reshape(-1, 12)
        mat = np.ascontiguousarray(mat, dtype=np.int8).reshape(-1, 25)
        q, t = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)
        qoff, toff = np.ascontiguousarray(qoff, dtype=np.int64), np.ascontiguousarray(toff, dtype=np.int64)
        assert len(mat) == len(params) and len(qoff) == len(params) + 1 and len(toff) == len(params) + 1
        out = np.zeros((len(params), 7), dtype=np.int32)
        fn = lib().bwahip_kat_ksw_extend2_diag if diag else lib().bwahip_kat_ksw_extend2
        _check(fn(self._h, len(params), params.ctypes.data, mat.ctypes.data, q.ctypes.data, qoff.ctypes.data, t.ctypes.data,
                  toff.ctypes.data, out.ctypes.data), "bwahip_kat_ksw_extend2_diag" if diag else "bwahip_kat_ksw_extend2")
        return out

    def kat_ksw_global(self, params, mat, q, qoff, t, toff):
        """ksw_global2 with CIGAR through the kernels' own code (bwahip_kat_ksw_global); params n x 10 (qlen, tlen, w, o_del, e_del, o_ins, e_ins,
        reverse, form KAT_GLOBAL_*, cpl), mat n x 25 -> (n x 2 (score, n_cigar or -1), n x KAT_MAX_CIGAR words)."""
        params = np.ascontiguousarray(params, dtype=np.int32).reshape(-1, 10)
        mat = np.ascontiguousarray(mat, dtype=np.int8).reshape(-1, 25)
        q, t = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)
        qoff, toff = np.ascontiguousarray(qoff, dtype=np.int64), np.ascontiguousarray(toff, dtype=np.int64)
        assert len(mat) == len(params) and len(qoff) == len(params) + 1 and len(toff) == len(params) + 1
        out = np.zeros((len(params), 2), dtype=np.int32)
        cig = np.zeros((len(params), KAT_MAX_CIGAR), dtype=np.uint32)
        _check(lib().bwahip_kat_ksw_global(self._h, len(params), params.ctypes.data, mat.ctypes.data, q.ctypes.data, qoff.ctypes.data, t.ctypes.data,
                                           toff.ctypes.data, out.ctypes.data, cig.ctypes.data), "bwahip_kat_ksw_global")
        return out, cig

    def kat_ksw_align(self, params, q, qoff, t, toff, mat=None):
        """ksw_align2 on the device; params n x 8 (qlen, tlen, xtra, o_del, e_del, o_ins, e_ins, 0) -> n x 7."""
        params = np.ascontiguousarray(params, dtype=np.int32)
        q, t = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)
        qoff, toff = np.ascontiguousarray(qoff, dtype=np.int64), np.ascontiguousarray(toff, dtype=np.int64)
        out = np.zeros((len(params), 7), dtype=np.int32)
        m = np.ascontiguousarray(mat, dtype=np.int8) if mat is not None else None
        _check(lib().bwahip_kat_ksw_align(self._h, len(params), params.ctypes.data, m.ctypes.data if m is not None else None, q.ctypes.data,
                                          qoff.ctypes.data, t.ctypes.data, toff.ctypes.data, out.ctypes.data), "bwahip_kat_ksw_align")
        return out

    def kat_extend(self, ik3, is_back):
        ik3 = np.ascontiguousarray(ik3, dtype=np.uint64)
        is_back = np.ascontiguousarray(is_back, dtype=np.int32)
        out = np.zeros((len(is_back), 12), dtype=np.uint64)
        _check(lib().bwahip_kat_extend(self._h, len(is_back), ik3.ctypes.data, is_back.ctypes.data, out.ctypes.data), "bwahip_kat_extend")
        return out


# ---------------------------------------------------------------- tooling wrappers (synthetic data, index build)
class FastqReader:
    """bwahip_fastq_*: batches of a FASTA/FASTQ file (pair), plain or gzip, as bseq_read (bwa.c:191) cuts them."""

    def __init__(self, path1, path2=None, threads=0):
        self._h = C.c_void_p()
        _check(lib().bwahip_fastq_open_mt(os.fsencode(path1), os.fsencode(path2) if path2 else None, threads, C.byref(self._h)), "bwahip_fastq_open_mt")

    def next(self, chunk_bases, keep_comments=False):
        """-> (pointer to the bseq1_t array owned by the reader, n); n == 0 at the end of the input."""
        arr, n = C.POINTER(Seq)(), C.c_int()
        _check(lib().bwahip_fastq_next(self._h, chunk_bases, 1 if keep_comments else 0, C.byref(arr), C.byref(n)), "bwahip_fastq_next")
        return arr, n.value

    def next_batch(self, chunk_bases, keep_comments=False):
        """-> (batch handle, pointer to its bseq1_t array, n): an owned batch, valid until release_batch(handle); (None, None, 0) at the end."""
        h, arr, n = C.c_void_p(), C.POINTER(Seq)(), C.c_int()
        _check(lib().bwahip_fastq_next_batch(self._h, chunk_bases, 1 if keep_comments else 0, C.byref(h), C.byref(arr), C.byref(n)), "bwahip_fastq_next_batch")
        return (h, arr, n.value) if n.value else (None, None, 0)

    @staticmethod
    def release_batch(h):
        if h:
            lib().bwahip_fastq_batch_release(h)

    def close(self):
        if self._h:
            lib().bwahip_fastq_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def stream_run(ctxs, fq1, fq2=None, out_fd=-1, opt=None, chunk_bases=0, max_reads=0, keep_comments=False, reader_threads=0, pes0=None):
    """bwahip_stream_run: FASTQ files -> SAM text on out_fd over the given contexts (the library's own reader, workers and writer;
    no Python in the data path).  Returns the filled StreamStats."""
    opt = opt or default_opt()
    st = StreamStats()
    st.chunk_bases, st.max_reads, st.keep_comments, st.reader_threads = chunk_bases, max_reads, int(keep_comments), reader_threads
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(lib().bwahip_stream_run(arr, len(ctxs), C.byref(opt), C.byref(pes0) if pes0 is not None else None, os.fsencode(fq1),
                                   os.fsencode(fq2) if fq2 else None, out_fd, C.byref(st)), "bwahip_stream_run")
    return st


def stream_run_bam(ctxs, fq1, fq2=None, out_fd=-1, hdr_line=None, level=1, opt=None, chunk_bases=0, max_reads=0, keep_comments=False,
                   reader_threads=0, pes0=None):
    """bwahip_stream_run_bam: FASTQ files -> a BAM file (header, BGZF blocks, EOF block) on out_fd.  Returns the filled StreamStats
    (sam_bytes = uncompressed bytes of the records)."""
    opt = opt or default_opt()
    st = StreamStats()
    st.chunk_bases, st.max_reads, st.keep_comments, st.reader_threads = chunk_bases, max_reads, int(keep_comments), reader_threads
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    if isinstance(hdr_line, str):
        hdr_line = hdr_line.encode()
    _check(lib().bwahip_stream_run_bam(arr, len(ctxs), C.byref(opt), C.byref(pes0) if pes0 is not None else None, os.fsencode(fq1),
                                       os.fsencode(fq2) if fq2 else None, out_fd, hdr_line, level, C.byref(st)), "bwahip_stream_run_bam")
    return st


def stream_run_bam_dev(ctxs, fq1, fq2=None, out_fd=-1, hdr_line=None, opt=None, chunk_bases=0, max_reads=0, keep_comments=False,
                       reader_threads=0, pes0=None):
    """bwahip_stream_run_bam_dev: FASTQ files -> a BAM file on out_fd whose BGZF blocks are deflated and checksummed on the GPU.
    Returns (StreamStats, BgzfStats)."""
    opt = opt or default_opt()
    st, bs = StreamStats(), BgzfStats()
    st.chunk_bases, st.max_reads, st.keep_comments, st.reader_threads = chunk_bases, max_reads, int(keep_comments), reader_threads
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    if isinstance(hdr_line, str):
        hdr_line = hdr_line.encode()
    _check(lib().bwahip_stream_run_bam_dev(arr, len(ctxs), C.byref(opt), C.byref(pes0) if pes0 is not None else None, os.fsencode(fq1),
                                           os.fsencode(fq2) if fq2 else None, out_fd, hdr_line, C.byref(st), C.byref(bs)), "bwahip_stream_run_bam_dev")
    return st, bs


def stream_run_bam_sorted(ctxs, fq1, fq2=None, out_fd=-1, hdr_line=None, level=1, opt=None, chunk_bases=0, max_reads=0, keep_comments=False,
                          reader_threads=0, pes0=None, tmp_dir=None, mem_budget=1 << 30):
    """bwahip_stream_run_bam_sorted: FASTQ files -> a coordinate-sorted BAM file on out_fd.  Returns (StreamStats, SortStats)."""
    opt = opt or default_opt()
    st, so = StreamStats(), SortStats()
    st.chunk_bases, st.max_reads, st.keep_comments, st.reader_threads = chunk_bases, max_reads, int(keep_comments), reader_threads
    so.tmp_dir, so.mem_budget = os.fsencode(tmp_dir) if tmp_dir is not None else None, mem_budget
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    if isinstance(hdr_line, str):
        hdr_line = hdr_line.encode()
    _check(lib().bwahip_stream_run_bam_sorted(arr, len(ctxs), C.byref(opt), C.byref(pes0) if pes0 is not None else None, os.fsencode(fq1),
                                              os.fsencode(fq2) if fq2 else None, out_fd, hdr_line, level, C.byref(st), C.byref(so)), "bwahip_stream_run_bam_sorted")
    return st, so


def _sorted_dev(name, ctxs, fq1, fq2, out_fd, hdr_line, opt, pes0, reader, hbm_budget, piece_blocks, tmp_dir=None, mem_budget=0, level=1):
    """What the stream_run_bam_sorted_dev* wrappers share: StreamStats filled from reader = (chunk_bases, max_reads, keep_comments,
    reader_threads), SortDevStats from the budgets (tmp_dir, mem_budget and level are the host merger's after a fall-back), the context
    array and the encoded header.  Returns (st, sd, call): call(*rest) runs entry point `name` with the ten leading arguments all of them
    take, then rest, and raises on an error."""
    opt = opt or default_opt()
    st, sd = StreamStats(), SortDevStats()
    st.chunk_bases, st.max_reads, st.keep_comments, st.reader_threads = reader[0], reader[1], int(reader[2]), reader[3]
    sd.tmp_dir, sd.mem_budget, sd.level = os.fsencode(tmp_dir) if tmp_dir is not None else None, mem_budget, level
    sd.hbm_budget, sd.piece_blocks = hbm_budget, piece_blocks
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    if isinstance(hdr_line, str):
        hdr_line = hdr_line.encode()

    def call(*rest):
        _check(getattr(lib(), name)(arr, len(ctxs), C.byref(opt), C.byref(pes0) if pes0 is not None else None, os.fsencode(fq1), os.fsencode(fq2) if fq2 else None,
                                    out_fd, hdr_line, C.byref(st), C.byref(sd), *rest), name)
    return st, sd, call


def _spill_stats(host_budget, tmp_dir, window_pieces):
    sp = SpillStats()
    sp.host_budget, sp.tmp_dir, sp.window_pieces = host_budget, os.fsencode(tmp_dir) if tmp_dir is not None else None, window_pieces
    return sp


def _opt_ref(make, values):
    """byref of the options struct made of `values`, or None to pass no options"""
    return C.byref(make(*values)) if values is not None else None


def stream_run_bam_sorted_dev(ctxs, fq1, fq2=None, out_fd=-1, hdr_line=None, opt=None, chunk_bases=0, max_reads=0, keep_comments=False,
                              reader_threads=0, pes0=None, hbm_budget=0, piece_blocks=0, tmp_dir=None, mem_budget=1 << 30, level=1):
    """bwahip_stream_run_bam_sorted_dev: FASTQ files -> a coordinate-sorted BAM file on out_fd, the runs kept, merged and deflated in HBM;
    tmp_dir, mem_budget and level are the host merger's after a fall-back.  Returns (StreamStats, SortDevStats)."""
    st, sd, call = _sorted_dev("bwahip_stream_run_bam_sorted_dev", ctxs, fq1, fq2, out_fd, hdr_line, opt, pes0, (chunk_bases, max_reads, keep_comments, reader_threads),
                               hbm_budget, piece_blocks, tmp_dir, mem_budget, level)
    call()
    return st, sd


def stream_run_bam_sorted_bai(ctxs, fq1, fq2=None, out_fd=-1, bai_fd=-1, hdr_line=None, level=1, opt=None, chunk_bases=0, max_reads=0, keep_comments=False,
                              reader_threads=0, pes0=None, tmp_dir=None, mem_budget=1 << 30):
    """bwahip_stream_run_bam_sorted_bai: stream_run_bam_sorted with the BAI index of the file on bai_fd.  Returns (StreamStats, SortStats)."""
    opt = opt or default_opt()
    st, so = StreamStats(), SortStats()
    st.chunk_bases, st.max_reads, st.keep_comments, st.reader_threads = chunk_bases, max_reads, int(keep_comments), reader_threads
    so.tmp_dir, so.mem_budget = os.fsencode(tmp_dir) if tmp_dir is not None else None, mem_budget
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    if isinstance(hdr_line, str):
        hdr_line = hdr_line.encode()
    _check(lib().bwahip_stream_run_bam_sorted_bai(arr, len(ctxs), C.byref(opt), C.byref(pes0) if pes0 is not None else None, os.fsencode(fq1),
                                                  os.fsencode(fq2) if fq2 else None, out_fd, hdr_line, level, C.byref(st), C.byref(so), bai_fd), "bwahip_stream_run_bam_sorted_bai")
    return st, so


def stream_run_bam_sorted_dev_bai(ctxs, fq1, fq2=None, out_fd=-1, bai_fd=-1, hdr_line=None, opt=None, chunk_bases=0, max_reads=0, keep_comments=False,
                                  reader_threads=0, pes0=None, hbm_budget=0, piece_blocks=0, tmp_dir=None, mem_budget=1 << 30, level=1):
    """bwahip_stream_run_bam_sorted_dev_bai: stream_run_bam_sorted_dev with the BAI index of the file on bai_fd, built on the device (after
    a fall-back: by the host builder).  Returns (StreamStats, SortDevStats)."""
    st, sd, call = _sorted_dev("bwahip_stream_run_bam_sorted_dev_bai", ctxs, fq1, fq2, out_fd, hdr_line, opt, pes0, (chunk_bases, max_reads, keep_comments, reader_threads),
                               hbm_budget, piece_blocks, tmp_dir, mem_budget, level)
    call(bai_fd)
    return st, sd


def stream_run_bam_sorted_dev_markdup(ctxs, fq1, fq2=None, out_fd=-1, bai_fd=-1, hdr_line=None, opt=None, chunk_bases=0, max_reads=0, keep_comments=False,
                                      reader_threads=0, pes0=None, hbm_budget=0, piece_blocks=0):
    """bwahip_stream_run_bam_sorted_dev_markdup: stream_run_bam_sorted_dev_bai with duplicates marked on the device before the deflate
    (bai_fd < 0: no index).  No host fall-back: a run that does not fit hbm_budget raises ECAPACITY.  Returns (StreamStats, SortDevStats,
    MarkdupStats)."""
    st, sd, call = _sorted_dev("bwahip_stream_run_bam_sorted_dev_markdup", ctxs, fq1, fq2, out_fd, hdr_line, opt, pes0, (chunk_bases, max_reads, keep_comments, reader_threads),
                               hbm_budget, piece_blocks)
    ms = MarkdupStats()
    call(bai_fd, C.byref(ms))
    return st, sd, ms


def stream_run_bam_sorted_dev_qc(ctxs, fq1, fq2=None, out_fd=-1, bai_fd=-1, qc_fd=-1, markdup=False, qc=(), hdr_line=None, opt=None, chunk_bases=0, max_reads=0,
                                 keep_comments=False, reader_threads=0, pes0=None, hbm_budget=0, piece_blocks=0, tmp_dir=None, mem_budget=1 << 30, level=1):
    """bwahip_stream_run_bam_sorted_dev_qc: stream_run_bam_sorted_dev_markdup (markdup) or stream_run_bam_sorted_dev_bai with the QC summary of
    the file on qc_fd (csrc/k_qc.hip; after a fall-back: the host builder).  qc = (window_shift, exclude_flags, min_mapq).  Returns
    (StreamStats, SortDevStats, MarkdupStats, QcStats)."""
    st, sd, call = _sorted_dev("bwahip_stream_run_bam_sorted_dev_qc", ctxs, fq1, fq2, out_fd, hdr_line, opt, pes0, (chunk_bases, max_reads, keep_comments, reader_threads),
                               hbm_budget, piece_blocks, tmp_dir, mem_budget, level)
    ms, qs = MarkdupStats(), QcStats()
    call(bai_fd, C.byref(ms), int(bool(markdup)), C.byref(qc_opt(*qc)), qc_fd, C.byref(qs))
    return st, sd, ms, qs


def stream_run_bam_sorted_dev_pileup(ctxs, fq1, fq2=None, out_fd=-1, bai_fd=-1, qc_fd=-1, pu_fd=-1, markdup=False, qc=None, pileup=(), hdr_line=None, opt=None,
                                     chunk_bases=0, max_reads=0, keep_comments=False, reader_threads=0, pes0=None, hbm_budget=0, piece_blocks=0):
    """bwahip_stream_run_bam_sorted_dev_pileup: the device-merged sorted BAM file with the pileup of the file on pu_fd (csrc/k_pileup.hip), over
    the contexts' reference.  bai_fd >= 0: the index; markdup: duplicates marked; qc = (window_shift, exclude_flags, min_mapq) or (): the QC
    summary on qc_fd; pileup = (min_mapq, min_baseq, exclude_flags, min_alt), None to pass no options.  No host fall-back.  Returns
    (StreamStats, SortDevStats, MarkdupStats, QcStats, PileupStats)."""
    st, sd, call = _sorted_dev("bwahip_stream_run_bam_sorted_dev_pileup", ctxs, fq1, fq2, out_fd, hdr_line, opt, pes0, (chunk_bases, max_reads, keep_comments, reader_threads),
                               hbm_budget, piece_blocks)
    ms, qs, ps = MarkdupStats(), QcStats(), PileupStats()
    call(bai_fd, int(bool(markdup)), C.byref(ms), _opt_ref(qc_opt, qc), qc_fd, C.byref(qs), _opt_ref(pileup_opt, pileup), pu_fd, C.byref(ps))
    return st, sd, ms, qs, ps


def stream_run_bam_sorted_dev_spill(ctxs, fq1, fq2=None, out_fd=-1, bai_fd=-1, qc_fd=-1, markdup=False, qc=None, hdr_line=None, opt=None, chunk_bases=0, max_reads=0,
                                    keep_comments=False, reader_threads=0, pes0=None, hbm_budget=0, piece_blocks=0, host_budget=0, tmp_dir=None, window_pieces=0):
    """bwahip_stream_run_bam_sorted_dev_spill: the device-merged sorted BAM file for samples whose record bytes outgrow HBM -- runs that do
    not fit hbm_budget keep their record bytes in a host-side store (host_budget, tmp_dir) and the finish stages them window by window.
    bai_fd >= 0: the index; markdup: duplicates marked; qc = (window_shift, exclude_flags, min_mapq) or (): the QC summary on qc_fd.
    Returns (StreamStats, SortDevStats, SpillStats, MarkdupStats, QcStats)."""
    st, sd, call = _sorted_dev("bwahip_stream_run_bam_sorted_dev_spill", ctxs, fq1, fq2, out_fd, hdr_line, opt, pes0, (chunk_bases, max_reads, keep_comments, reader_threads),
                               hbm_budget, piece_blocks)
    sp, ms, qs = _spill_stats(host_budget, tmp_dir, window_pieces), MarkdupStats(), QcStats()
    call(C.byref(sp), bai_fd, int(bool(markdup)), C.byref(ms), _opt_ref(qc_opt, qc), qc_fd, C.byref(qs))
    return st, sd, sp, ms, qs


def stream_run_bam_sorted_dev_recal(ctxs, fq1, fq2=None, out_fd=-1, bai_fd=-1, qc_fd=-1, rc_fd=-1, markdup=False, qc=None, recal=(), mask=None, hdr_line=None, opt=None,
                                    chunk_bases=0, max_reads=0, keep_comments=False, reader_threads=0, pes0=None, hbm_budget=0, piece_blocks=0, host_budget=0, tmp_dir=None,
                                    window_pieces=0):
    """bwahip_stream_run_bam_sorted_dev_recal: stream_run_bam_sorted_dev_spill with the recalibration table of the file on rc_fd
    (csrc/k_recal.hip), over the contexts' reference and this mask of known sites (bytes, None: none).  recal = (min_mapq, min_baseq,
    exclude_flags, max_cycle), None to pass no options.  Returns (StreamStats, SortDevStats, SpillStats, MarkdupStats, QcStats, RecalStats)."""
    st, sd, call = _sorted_dev("bwahip_stream_run_bam_sorted_dev_recal", ctxs, fq1, fq2, out_fd, hdr_line, opt, pes0, (chunk_bases, max_reads, keep_comments, reader_threads),
                               hbm_budget, piece_blocks)
    sp, ms, qs, rs = _spill_stats(host_budget, tmp_dir, window_pieces), MarkdupStats(), QcStats(), RecalStats()
    call(C.byref(sp), bai_fd, int(bool(markdup)), C.byref(ms), _opt_ref(qc_opt, qc), qc_fd, C.byref(qs), _opt_ref(recal_opt, recal), bytes(mask) if mask is not None else None,
         rc_fd, C.byref(rs))
    return st, sd, sp, ms, qs, rs


def _tool(name):
    path = os.path.join(TOOLS, name)
    if not os.path.exists(path):
        raise BwahipError(f"{path} is missing: run __graft_entry__.build()")
    return path


def make_genome(fa, seed, lens, repeats=True):
    subprocess.check_call([_tool("simgen"), "genome", fa, str(seed), "1" if repeats else "0"] + [str(x) for x in lens])


def make_reads(fa, fq1, fq2, n, length, sub_ppm, indel_ppm, n_ppm, seed, chim_ppm=0):
    subprocess.check_call([_tool("simgen"), "reads", fa, fq1, fq2 or "-", str(n), str(length), str(sub_ppm), str(indel_ppm),
                           str(n_ppm), str(seed), str(chim_ppm)])


def make_index(fa, prefix):
    subprocess.check_call([_tool("mkindex"), fa, prefix])


def read_fastq(path):
    names, seqs, quals = [], [], []
    with open(path, "rb") as f:
        while True:
            h = f.readline()
            if not h:
                break
            s = f.readline().rstrip(b"\r\n")
            f.readline()
            q = f.readline().rstrip(b"\r\n")
            names.append(h[1:].split()[0])
            seqs.append(s)
            quals.append(q)
    return names, seqs, quals
