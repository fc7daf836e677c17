#!/usr/bin/env python3
"""What duplicate marking costs inside the device merger's finish (csrc/k_markdup.hip), after scripts/bai_rate.py: the same runs through
bwahip_bam_devmerger_finish_bai (unmarked) and bwahip_bam_devmerger_finish_markdup with the index, ALTERNATING in one process, output
dropped, warm-up first.  Three things are timed by HIP events: the batch's descriptor kernel (bwahip_kat_dup_desc, the kernel alone, on
every run's records in input order), the decision stage and the marking pass (decide_ms / mark_ms of bwahip_markdup_stats_t).

The runs are synthetic: N / 2 pairs of valid 304-byte BAM records (a 150M CIGAR, a 12-byte name, 150 bases with qualities 2 .. 41, 27
bytes of tags) at uniform positions on a human-like contig table, FR with inserts of 200 .. 500, a tenth of the pairs placed exactly
where an earlier pair is, a twentieth of the mates unmapped; consecutive pairs are dealt to R runs as batches would be.  Any index
serves for the context.
    python3 scripts/markdup_rate.py <index prefix> [records = 4000000] [runs = 8] [repetitions = 5] > profiles/markdup/markdup_rate_4M.json
With BWAHIP_ROOT=<another checkout of this repository that has been built> the library of that tree is loaded instead; a tree from before
marking existed (the parent commit) then gives its unmarked finish_bai on the same runs, and nothing else.  Prints one JSON object."""
import json, os, statistics, sys
import numpy as np
ROOT = os.environ.get("BWAHIP_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry
bw = entry.load_bwahip()
prefix = sys.argv[1]
n = (int(sys.argv[2]) if len(sys.argv) > 2 else 4000000) & ~1
n_runs = int(sys.argv[3]) if len(sys.argv) > 3 else 8
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
has_markdup = hasattr(bw, "stream_run_bam_sorted_dev_markdup")
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
out = {"workload": f"{n} synthetic 304-byte records in {T} pairs on a human-like contig table, {n_runs} runs", "repetitions": reps, "library": ROOT}
bounds = [T * k // n_runs for k in range(n_runs + 1)]
rows = {"finish_bai": [], "finish_markdup": []}
desc_ms = []
with bw.Context(prefix, 0) as ctx, bw.DevMerger(ctx, 0) as m_plain, bw.DevMerger(ctx, 0) as m_dup:
    for k in range(n_runs):
        run = recs[bounds[k]:bounds[k + 1]].reshape(-1)                        # input order: the mates are neighbours
        keys = key_of(run)
        order = np.argsort(keys, kind="stable")
        srt, off = run[order].tobytes(), np.arange(len(run) + 1, dtype=np.int64) * 304
        m_plain.add(k, srt, keys[order], off)
        if has_markdup:
            raw = run.tobytes()
            for r in range(reps + 1):                                          # r = 0: warm-up
                desc = ctx.kat_dup_desc(raw, off, True)
                if r:
                    desc_ms.append((k, ctx.kat_dup_desc_ms()))
            m_dup.add_dup(k, srt, keys[order], off, (order // 2).astype(np.uint32), desc)
    for r in range(reps + 1):
        for what in ("finish_bai", "finish_markdup") if has_markdup else ("finish_bai",):
            if what == "finish_bai":
                st, bs = m_plain.finish_bai(-1, -1, 1000, len(LENS))
                row = {}
            else:
                st, bs, ms = m_dup.finish_markdup(-1, -1, 1000, len(LENS))
                row = dict(markdup_ms=ms.markdup_ms, decide_ms=ms.decide_ms, mark_ms=ms.mark_ms, hbm_bytes=ms.hbm_bytes, n_marked=ms.n_marked,
                           n_templates=list(ms.n_templates), n_dup_templates=list(ms.n_dup_templates))
            row.update(finish_s=st.finish_s, sort_ms=st.sort_ms, gather_ms=st.gather_ms, deflate_ms=st.deflate_ms, index_ms=bs.index_ms, raw_bytes=st.raw_bytes, bgzf_bytes=st.bgzf_bytes)
            if r:
                rows[what].append(row)
for what, v in rows.items():
    if v:
        out[what] = {f: mm([x[f] for x in v]) for f in ("finish_s", "sort_ms", "gather_ms", "deflate_ms", "index_ms")}
        out[what].update(raw_bytes=v[0]["raw_bytes"], bgzf_bytes=v[0]["bgzf_bytes"])
if has_markdup:
    b = rows["finish_markdup"]
    out["finish_markdup"].update({f: mm([x[f] for x in b]) for f in ("markdup_ms", "decide_ms", "mark_ms")}, **{f: b[0][f] for f in ("hbm_bytes", "n_marked", "n_templates", "n_dup_templates")})
    gpu = [x["sort_ms"] + x["gather_ms"] + x["deflate_ms"] + x["index_ms"] + x["markdup_ms"] for x in b]
    out["markdup_share_of_finish_gpu_time"] = mm([x["markdup_ms"] / t for x, t in zip(b, gpu)], 4)
    out["finish_markdup_over_finish_bai_seconds"] = round(med([x["finish_s"] for x in b]) / med([x["finish_s"] for x in rows["finish_bai"]]), 4)
    per_rep = [sum(ms for k, ms in desc_ms[r::reps]) for r in range(reps)]     # all runs' kernels of one repetition
    out["dup_desc"] = {"kernel_ms_all_runs": mm(per_rep), "record_bytes": n * 304, "record_bytes_per_ms": round(n * 304 / med(per_rep)),
                       "GB_per_s": round(n * 304 / med(per_rep) / 1e6, 1)}
print(json.dumps(out))
