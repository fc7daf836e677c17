#!/usr/bin/env python3
"""What the BAI index costs inside the device merger's finish (csrc/k_bai.hip), after scripts/bam_sorted_dev_rate.py: the same runs
through bwahip_bam_devmerger_finish and bwahip_bam_devmerger_finish_bai, ALTERNATING in one process, output dropped, warm-up first.
The yardstick is finish on the same runs; reported beside it are the index stage's GPU time (index_ms) and the sort / gather / deflate
milliseconds of the finish, the chunks, windows and bytes of the index, and the HBM the stage held.

The runs are synthetic: N valid BAM records of 304 bytes (a 150M CIGAR, a name, 252 bytes of a four-letter alphabet) at uniform
positions on a human-like contig table (25 contigs, the longest 248 956 422 bases), a twentieth of them unmapped with their mate's
coordinates and a hundredth without a reference, dealt at random to R sorted runs.  Any index serves for the context.
    python3 scripts/bai_rate.py <index prefix> [records = 4000000] [runs = 8] [repetitions = 5] > profiles/bai/bai_rate.json
Prints one JSON object."""
import json, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry
bw = entry.load_bwahip()
prefix = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4000000
n_runs = int(sys.argv[3]) if len(sys.argv) > 3 else 8
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
LENS = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309, 114364328, 107043718,
        101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415, 16569]
rng = np.random.default_rng(1)
rec_t = np.dtype([("block_size", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                  ("l_seq", "<i4"), ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S12"), ("cigar", "<u4"), ("rest", "u1", 252)])
assert rec_t.itemsize == 304
g = np.sort(rng.integers(0, sum(LENS) - 150 * len(LENS), n))                   # a position on the concatenated contigs
starts = np.concatenate(([0], np.cumsum([l - 150 for l in LENS])))
ref = np.searchsorted(starts, g, side="right") - 1
pos = g - starts[ref]
no_ref = rng.random(n) < 0.01
ref[no_ref], pos[no_ref] = -1, -1
flag = np.where(rng.random(n) < 0.5, 16, 0).astype(np.uint16)
flag[rng.random(n) < 0.05] |= 4
flag[no_ref] = 4
recs = np.zeros(n, dtype=rec_t)
recs["block_size"], recs["ref"], recs["pos"], recs["l_read_name"], recs["mapq"], recs["n_cigar"], recs["flag"] = 300, ref, pos, 12, 60, 1, flag
recs["next_ref"], recs["next_pos"], recs["name"], recs["cigar"] = -1, -1, b"read.name.x", 150 << 4
recs["rest"] = rng.integers(0, 4, (n, 252), dtype=np.uint8) + 65
pos_bits = (max(LENS) + 1).bit_length()
keys = (np.where(ref < 0, len(LENS), ref).astype(np.uint64) << np.uint64(pos_bits + 1)) | ((pos + 1).astype(np.uint64) << np.uint64(1)) | (flag >> 4 & 1).astype(np.uint64)
order = np.argsort(keys, kind="stable")
recs, keys = recs[order], keys[order]
run_of = rng.integers(0, n_runs, n)
med = statistics.median
mm = lambda v, nd=3: {"median": round(med(v), nd), "min_max": [round(min(v), nd), round(max(v), nd)]}
out = {"workload": f"{n} synthetic 304-byte records on a human-like contig table, {n_runs} runs", "repetitions": reps}
rows = {"finish": [], "finish_bai": []}
with bw.Context(prefix, 0) as ctx, bw.DevMerger(ctx, 0) as m:
    for k in range(n_runs):
        sel = run_of == k
        m.add(k, recs[sel].tobytes(), keys[sel], np.arange(int(sel.sum()) + 1, dtype=np.int64) * 304)
    for r in range(reps + 1):                                                  # r = 0: warm-up
        for what in ("finish", "finish_bai"):
            if what == "finish":
                st, row = m.finish(-1), {}
            else:
                st, bs = m.finish_bai(-1, -1, 1000, len(LENS))
                row = {f: getattr(bs, f) for f in ("n_chunks", "n_windows", "n_no_coor", "bai_bytes", "hbm_bytes", "index_ms")}
            row.update(finish_s=st.finish_s, sort_ms=st.sort_ms, gather_ms=st.gather_ms, deflate_ms=st.deflate_ms, raw_bytes=st.raw_bytes, bgzf_bytes=st.bgzf_bytes)
            if r:
                rows[what].append(row)
for what, v in rows.items():
    out[what] = {f: mm([x[f] for x in v]) for f in ("finish_s", "sort_ms", "gather_ms", "deflate_ms")}
    out[what].update(raw_bytes=v[0]["raw_bytes"], bgzf_bytes=v[0]["bgzf_bytes"])
b = rows["finish_bai"]
out["finish_bai"].update(index_ms=mm([x["index_ms"] for x in b]), **{f: b[0][f] for f in ("n_chunks", "n_windows", "n_no_coor", "bai_bytes", "hbm_bytes")})
gpu = [x["sort_ms"] + x["gather_ms"] + x["deflate_ms"] + x["index_ms"] for x in b]
out["index_share_of_finish_gpu_time"] = mm([x["index_ms"] / t for x, t in zip(b, gpu)], 4)
out["finish_bai_over_finish_seconds"] = round(med([x["finish_s"] for x in b]) / med([x["finish_s"] for x in rows["finish"]]), 4)
print(json.dumps(out))
