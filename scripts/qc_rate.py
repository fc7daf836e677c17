#!/usr/bin/env python3
"""What the QC stage costs inside the device merger's finish (csrc/k_qc.hip), after scripts/bai_rate.py and scripts/markdup_rate.py: the
same runs through bwahip_bam_devmerger_finish_bai unarmed and armed (bwahip_bam_devmerger_set_qc), ALTERNATING in one process, output
dropped, warm-up first.  The stage's record_ms and scan_ms are HIP events (bwahip_qc_stats_t); what is left of qc_ms is the clearing of
the tables and of the difference array.  The contig table is the human-like one of the other rate scripts (25 contigs, 3.1 Gbp), so the
scan term -- 4 bytes per base, whatever the records -- is the one of the bench genome; a second armed merger over a 25 Mbp table (the
records beyond a contig's end are clipped) shows what it is without it.  The scan is set against a plain device-to-device copy of the
difference array's bytes (a read plus a write, torch), the record pass against the whole BAI stage on the same records (index_ms).
    python3 scripts/qc_rate.py <index prefix> [records = 4000000] [runs = 8] [repetitions = 5] > profiles/qc/qc_rate_4M.json
Any index serves for the context.  Prints one JSON object."""
import json, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry
bw = entry.load_bwahip()
prefix = sys.argv[1]
n = (int(sys.argv[2]) if len(sys.argv) > 2 else 4000000) & ~1
n_runs = int(sys.argv[3]) if len(sys.argv) > 3 else 8
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
LENS = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309, 114364328, 107043718,
        101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415, 16569]
SMALL = [min(l, 1000000) for l in LENS]
rng = np.random.default_rng(1)
rec_t = np.dtype([("block_size", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                  ("l_seq", "<i4"), ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S12"), ("cigar", "<u4"), ("seq", "u1", 75), ("qual", "u1", 150),
                  ("rest", "u1", 27)])
assert rec_t.itemsize == 304
T = n // 2
g = rng.integers(0, sum(LENS) - 1000 * len(LENS), T)
ins = rng.integers(200, 501, T)
starts = np.concatenate(([0], np.cumsum([l - 1000 for l in LENS])))
ref = np.searchsorted(starts, g, side="right") - 1
pos = g - starts[ref]
recs = np.zeros((T, 2), dtype=rec_t)
recs["block_size"], recs["l_read_name"], recs["mapq"], recs["n_cigar"], recs["l_seq"] = 300, 12, 60, 1, 150
recs["ref"], recs["next_ref"] = ref[:, None], ref[:, None]
recs["pos"][:, 0], recs["pos"][:, 1] = pos, pos + ins - 150
recs["next_pos"][:, 0], recs["next_pos"][:, 1] = recs["pos"][:, 1], recs["pos"][:, 0]
recs["tlen"][:, 0], recs["tlen"][:, 1] = ins, -ins
recs["flag"][:, 0], recs["flag"][:, 1] = 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80
recs["mapq"] = rng.choice(np.array([0, 20, 40, 60, 60, 60], dtype=np.uint8), (T, 2))
recs["name"], recs["cigar"] = b"read.name.x", 150 << 4
recs["qual"] = 30
pos_bits = (max(LENS) + 1).bit_length()
key_of = lambda r: (r["ref"].astype(np.uint64) << np.uint64(pos_bits + 1)) | ((r["pos"] + 1).astype(np.uint64) << np.uint64(1)) | (r["flag"] >> 4 & 1).astype(np.uint64)
med = statistics.median
mm = lambda v, nd=3: {"median": round(med(v), nd), "min_max": [round(min(v), nd), round(max(v), nd)]}
out = {"workload": f"{n} synthetic 304-byte records in {T} pairs on a human-like contig table, {n_runs} runs", "repetitions": reps}
# the yardstick of the scan: one read plus one write of the difference array's bytes (torch first: it does not find the device once the library holds it)
import torch
slots = sum((l + 1 + 2047) // 2048 * 2048 for l in LENS)
a = torch.zeros(slots, dtype=torch.int32, device="cuda")
b = torch.empty_like(a)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
copy_ms = []
for r in range(reps + 1):
    ev[0].record(); b.copy_(a); ev[1].record(); torch.cuda.synchronize()
    if r:
        copy_ms.append(ev[0].elapsed_time(ev[1]))
del a, b
torch.cuda.empty_cache()
bounds = [T * k // n_runs for k in range(n_runs + 1)]
rows = {"unarmed": [], "armed_3.1Gbp": [], "armed_25Mbp": []}
with bw.Context(prefix, 0) as ctx, bw.DevMerger(ctx, 0) as m_plain, bw.DevMerger(ctx, 0) as m_qc, bw.DevMerger(ctx, 0) as m_small:
    for k in range(n_runs):
        run = recs[bounds[k]:bounds[k + 1]].reshape(-1)
        keys = key_of(run)
        order = np.argsort(keys, kind="stable")
        srt, off = run[order].tobytes(), np.arange(len(run) + 1, dtype=np.int64) * 304
        for m in (m_plain, m_qc, m_small):
            m.add(k, srt, keys[order], off)
    qs = {"armed_3.1Gbp": m_qc.set_qc(LENS, -1, ()), "armed_25Mbp": m_small.set_qc(SMALL, -1, ())}
    mergers = {"unarmed": m_plain, "armed_3.1Gbp": m_qc, "armed_25Mbp": m_small}
    for r in range(reps + 1):                                                  # r = 0: warm-up
        for what, m in mergers.items():
            st, bs = m.finish_bai(-1, -1, 1000, len(LENS))
            row = dict(finish_s=st.finish_s, sort_ms=st.sort_ms, gather_ms=st.gather_ms, deflate_ms=st.deflate_ms, index_ms=bs.index_ms)
            if what in qs:
                q = qs[what]
                row.update(qc_ms=q.qc_ms, record_ms=q.record_ms, scan_ms=q.scan_ms, clear_ms=q.qc_ms - q.record_ms - q.scan_ms, hbm_bytes=q.hbm_bytes, n_windows=q.n_windows, qc_bytes=q.qc_bytes)
            if r:
                rows[what].append(row)
for what, v in rows.items():
    out[what] = {f: mm([x[f] for x in v]) for f in v[0] if f.endswith("_ms") or f == "finish_s"}
    if "qc_ms" in v[0]:
        out[what].update({f: v[0][f] for f in ("hbm_bytes", "n_windows", "qc_bytes")})
        gpu = [x["sort_ms"] + x["gather_ms"] + x["deflate_ms"] + x["index_ms"] + x["qc_ms"] for x in v]
        out[what]["qc_share_of_finish_gpu_time"] = mm([x["qc_ms"] / t for x, t in zip(v, gpu)], 4)
        out[what]["finish_over_unarmed_seconds"] = round(med([x["finish_s"] for x in v]) / med([x["finish_s"] for x in rows["unarmed"]]), 4)
scan = out["armed_3.1Gbp"]["scan_ms"]["median"]
out["difference_array_bytes"] = slots * 4
out["copy_same_bytes_ms"] = mm(copy_ms)
out["copy_TB_per_s_read_plus_write"] = round(2 * slots * 4 / med(copy_ms) / 1e9, 2)
out["scan_reads_the_array_twice_TB_per_s"] = round(2 * slots * 4 / scan / 1e9, 2)
out["scan_share_of_copy_rate"] = round((2 * slots * 4 / scan) / (2 * slots * 4 / med(copy_ms)), 3)
print(json.dumps(out))
