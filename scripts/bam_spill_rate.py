#!/usr/bin/env python3
"""What it costs to hold a device merger's runs spilled (csrc/k_bamspill.hip, csrc/spill_store.cpp), on the record set of
scripts/markdup_rate.py: N / 2 pairs of valid 304-byte BAM records on a human-like contig table, dealt to R runs.  The marked, indexed
finish (bwahip_bam_devmerger_finish_markdup with the index, output dropped), ALTERNATING in one process, warm-up first, with
  resident        every run in HBM (add_dup);
  spilled_mem     every run spilled, the record bytes in pinned host memory, window_pieces at the default (8);
  spilled_mem_q   the same at a quarter of the default (2);
  spilled_file    every run spilled to unlinked files in a temporary directory (host_budget 0), window_pieces at the default;
and, once, the only finish the records of a sample that does not fit had before: the host merger at level 1 with the BAI builder
listening and no marking (bwahip_bam_merger_finish_bai, the finish of bwahip_stream_run_bam_sorted_bai; its merge_s), output to /dev/null.
piece_blocks is the context's default (1 024), so a window is 535 MB.
    python3 scripts/bam_spill_rate.py <index prefix> [records = 4000000] [runs = 8] [repetitions = 3] [threads of the host finish = 1] > profiles/bam_spill/bam_spill_rate_4M.json
Prints one JSON object."""
import json, os, statistics, sys, tempfile, time
import numpy as np
ROOT = os.environ.get("BWAHIP_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry
bw = entry.load_bwahip()
prefix = sys.argv[1]
n = (int(sys.argv[2]) if len(sys.argv) > 2 else 4000000) & ~1
n_runs = int(sys.argv[3]) if len(sys.argv) > 3 else 8
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
host_threads = int(sys.argv[5]) if len(sys.argv) > 5 else 1
LENS = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309, 114364328, 107043718,
        101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415, 16569]
rng = np.random.default_rng(1)
rec_t = np.dtype([("block_size", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                  ("l_seq", "<i4"), ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S12"), ("cigar", "<u4"), ("seq", "u1", 75), ("qual", "u1", 150),
                  ("rest", "u1", 27)])
assert rec_t.itemsize == 304
T = n // 2
g = rng.integers(0, sum(LENS) - 1000 * len(LENS), T)                            # the pair's leftmost base on the concatenated contigs
copy = np.nonzero(rng.random(T) < 0.1)[0]
copy = copy[copy > 0]
src = rng.integers(0, copy)                                                    # an earlier pair: its place and its insert
ins = rng.integers(200, 501, T)
g[copy], ins[copy] = g[src], ins[src]
starts = np.concatenate(([0], np.cumsum([l - 1000 for l in LENS])))
ref = np.searchsorted(starts, g, side="right") - 1
pos = g - starts[ref]
recs = np.zeros((T, 2), dtype=rec_t)
recs["block_size"], recs["l_read_name"], recs["mapq"], recs["n_cigar"], recs["l_seq"] = 300, 12, 60, 1, 150
recs["ref"], recs["next_ref"] = ref[:, None], ref[:, None]
recs["pos"][:, 0], recs["pos"][:, 1] = pos, pos + ins - 150
recs["next_pos"][:, 0], recs["next_pos"][:, 1] = recs["pos"][:, 1], recs["pos"][:, 0]
recs["flag"][:, 0], recs["flag"][:, 1] = 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80
unm = rng.random(T) < 0.05                                                     # the second mate unmapped, at its mate's place
recs["flag"][unm, 0] = 0x1 | 0x8 | 0x40
recs["flag"][unm, 1] = 0x1 | 0x4 | 0x80
recs["pos"][unm, 1] = recs["pos"][unm, 0]
recs["name"], recs["cigar"] = b"read.name.x", 150 << 4
recs["seq"] = rng.integers(0, 256, (T, 2, 75), dtype=np.uint8)
recs["qual"] = rng.integers(2, 42, (T, 2, 150), dtype=np.uint8)
recs["rest"] = rng.integers(0, 4, (T, 2, 27), dtype=np.uint8) + 65
pos_bits = (max(LENS) + 1).bit_length()
key_of = lambda r: (r["ref"].astype(np.uint64) << np.uint64(pos_bits + 1)) | ((r["pos"] + 1).astype(np.uint64) << np.uint64(1)) | (r["flag"] >> 4 & 1).astype(np.uint64)
med = statistics.median
mm = lambda v, nd=3: {"median": round(med(v), nd), "min_max": [round(min(v), nd), round(max(v), nd)]}
out = {"workload": f"{n} synthetic 304-byte records in {T} pairs on a human-like contig table, {n_runs} runs", "repetitions": reps}
bounds = [T * k // n_runs for k in range(n_runs + 1)]
MODES = {"resident": None, "spilled_mem": (1 << 40, 0), "spilled_mem_q": (1 << 40, 2), "spilled_file": (0, 0)}   # (host_budget, window_pieces)
rows = {k: [] for k in MODES}
devnull = os.open(os.devnull, os.O_WRONLY)
with tempfile.TemporaryDirectory() as tmp, bw.Context(prefix, 0) as ctx:
    mergers = {k: bw.DevMerger(ctx, 0) for k in MODES}
    host = bw.BamMerger(tmp, 1 << 30)
    try:
        for k, v in MODES.items():
            if v:
                mergers[k].set_spill(v[0], tmp, v[1])
        t_add = {k: 0.0 for k in MODES}
        for k in range(n_runs):
            run = recs[bounds[k]:bounds[k + 1]].reshape(-1)                    # input order: the mates are neighbours
            keys = key_of(run)
            order = np.argsort(keys, kind="stable")
            srt, off = run[order].tobytes(), np.arange(len(run) + 1, dtype=np.int64) * 304
            desc = ctx.kat_dup_desc(run.tobytes(), off, True)
            tmpl = (order // 2).astype(np.uint32)
            for name, m in mergers.items():
                t0 = time.time()
                (m.add_spilled if MODES[name] else m.add_dup)(k, srt, keys[order], off, tmpl, desc)
                t_add[name] += time.time() - t0
            host.add(k, srt, keys[order], off)
        out["add_s"] = {k: round(v, 3) for k, v in t_add.items()}             # from host memory: upload (resident) or a copy into the store
        for r in range(reps + 1):                                              # r = 0: warm-up
            for name, m in mergers.items():
                st, bs, ms = m.finish_markdup(-1, -1, 1000, len(LENS))
                sp = m.spill_stats()
                if r:
                    rows[name].append(dict(finish_s=st.finish_s, sort_ms=st.sort_ms, gather_ms=st.gather_ms, deflate_ms=st.deflate_ms, index_ms=bs.index_ms, markdup_ms=ms.markdup_ms,
                                           upload_ms=sp.upload_ms, download_s=sp.download_s, n_windows=sp.n_windows, window_hbm_bytes=sp.window_hbm_bytes, hbm_bytes=st.hbm_bytes,
                                           host_bytes=sp.host_bytes, file_bytes=sp.file_bytes, n_marked=ms.n_marked, bgzf_bytes=st.bgzf_bytes, raw_bytes=st.raw_bytes))
        with bw.BaiBuilder(len(LENS), 1000) as bb:                             # one run only: the host merger finishes once
            t0 = time.time()
            host.finish_bai(devnull, bb, 1, host_threads)
            bb.finish(-1)
            out["host_finish_bai_level1"] = dict(merge_s=round(host.stats()["merge_s"], 3), wall_s=round(time.time() - t0, 3), threads=host_threads, runs_of_this_figure=1)
    finally:
        for m in mergers.values():
            m.close()
        host.close()
        os.close(devnull)
for name, v in rows.items():
    out[name] = {f: mm([x[f] for x in v]) for f in ("finish_s", "sort_ms", "gather_ms", "deflate_ms", "index_ms", "markdup_ms", "upload_ms")}
    out[name].update({f: v[0][f] for f in ("download_s", "n_windows", "window_hbm_bytes", "hbm_bytes", "host_bytes", "file_bytes", "n_marked", "bgzf_bytes", "raw_bytes")})
assert len({(v[0]["n_marked"], v[0]["bgzf_bytes"]) for v in rows.values()}) == 1, "the modes did not write the same file"
h = out["host_finish_bai_level1"]["merge_s"]
out["finish_s_over_host_merge_s"] = {name: round(med([x["finish_s"] for x in v]) / h, 4) for name, v in rows.items()}
out["spilled_over_resident_finish_s"] = {name: round(med([x["finish_s"] for x in v]) / med([x["finish_s"] for x in rows["resident"]]), 3) for name, v in rows.items()}
print(json.dumps(out))
