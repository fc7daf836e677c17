#!/usr/bin/env python3
"""What the recalibration-table stage costs inside the device merger's finish (csrc/k_recal.hip), after scripts/pileup_rate.py: the same runs
through bwahip_bam_devmerger_finish_bai unarmed, armed for the table without a mask, armed with a mask of about 1 % set bits, armed for
the pileup (k_pu_count's observe pass over the same records) and armed for the QC summary alone (k_qc_rec on the same records),
ALTERNATING in one process, output dropped, warm-up first.  The stages' times are HIP events (bwahip_recal_stats_t and its like).  The
workload is that of scripts/pileup_rate.py -- synthetic 304-byte records (150M) in FR pairs at uniform positions on a human-like table of
25 contigs, a random packed reference of the table's 3.1 Gbp, every read its reference's bases with 1 % of them changed -- with the
qualities drawn from four values (2, 12, 23, 37: a binned instrument), so that every quality has a slot in the workgroup's LDS.  The pass
is set against a plain device-to-device copy of the records' bytes (a read plus a write, torch).
    python3 scripts/recal_rate.py <index prefix> [records = 4000000] [runs = 8] [repetitions = 5] > profiles/recal/recal_rate_4M.json
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
flat = recs.reshape(-1)
for lo in range(0, n, 250000):
    flat["qual"][lo:lo + 250000] = rng.choice(np.array([2, 12, 23, 37, 37, 37], dtype=np.uint8), (len(flat[lo:lo + 250000]), 150))
# the packed reference, random, and every read's bases out of it: base i in byte i >> 2 at shift (~i & 3) << 1; 1 % of the bases changed
pac = rng.integers(0, 256, (sum(LENS) + 3) // 4, dtype=np.uint8)
ref_off = np.concatenate(([0], np.cumsum(LENS)))
gpos = ref_off[flat["ref"]] + flat["pos"]
J = np.arange(150, dtype=np.int64)
n_changed = 0
for lo in range(0, n, 250000):
    i = gpos[lo:lo + 250000, None] + J
    code = (pac[i >> 2] >> ((~i & 3) << 1).astype(np.uint8)) & 3
    change = rng.random(code.shape) < 0.01
    n_changed += int(change.sum())
    code = (code + change * rng.integers(1, 4, code.shape, dtype=np.uint8)) & 3
    nib = (1 << code).astype(np.uint8)
    flat["seq"][lo:lo + 250000] = nib[:, 0::2] << 4 | nib[:, 1::2]
del i, code, change, nib
# the mask: one bit set in 8 % of the bytes, about 1 % of the bits
n_mask = (sum(LENS) + 7) // 8
mask = np.zeros(n_mask, dtype=np.uint8)
for lo in range(0, n_mask, 1 << 25):
    m = len(mask[lo:lo + (1 << 25)])
    mask[lo:lo + m] = (rng.random(m) < 0.08) * (1 << rng.integers(0, 8, m, dtype=np.uint8))
mask_bits = int(np.count_nonzero(mask))
pos_bits = (max(LENS) + 1).bit_length()
key_of = lambda r: (r["ref"].astype(np.uint64) << np.uint64(pos_bits + 1)) | ((r["pos"] + 1).astype(np.uint64) << np.uint64(1)) | (r["flag"] >> 4 & 1).astype(np.uint64)
med = statistics.median
mm = lambda v, nd=3: {"median": round(med(v), nd), "min_max": [round(min(v), nd), round(max(v), nd)]}
out = {"workload": f"{n} synthetic 304-byte records in {T} pairs on a human-like contig table, real bases, {n_changed} of them changed, four qualities, {n_runs} runs; "
                   f"the mask has {mask_bits} of {sum(LENS)} bits set", "repetitions": reps}
# the yardstick of the pass: one read plus one write of the records' bytes (torch first: it does not find the device once the library holds it)
import torch
a = torch.zeros(n * 304, dtype=torch.uint8, device="cuda")
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
rows = {"unarmed": [], "recal": [], "recal_masked": [], "pileup": [], "qc_25Mbp": []}
pac_bytes, mask_bytes = pac.tobytes(), mask.tobytes()
with bw.Context(prefix, 0) as ctx, bw.DevMerger(ctx, 0) as m_plain, bw.DevMerger(ctx, 0) as m_rc, bw.DevMerger(ctx, 0) as m_rcm, bw.DevMerger(ctx, 0) as m_pu, \
        bw.DevMerger(ctx, 0) as m_qc:
    mergers = {"unarmed": m_plain, "recal": m_rc, "recal_masked": m_rcm, "pileup": m_pu, "qc_25Mbp": m_qc}
    for k in range(n_runs):
        run = recs[bounds[k]:bounds[k + 1]].reshape(-1)
        keys = key_of(run)
        order = np.argsort(keys, kind="stable")
        srt, off = run[order].tobytes(), np.arange(len(run) + 1, dtype=np.int64) * 304
        for m in mergers.values():
            m.add(k, srt, keys[order], off)
    rs = {"recal": m_rc.set_recal(LENS, pac_bytes, None, -1, ()), "recal_masked": m_rcm.set_recal(LENS, pac_bytes, mask_bytes, -1, ())}
    ps = m_pu.set_pileup(LENS, pac_bytes, -1, ())
    qs = m_qc.set_qc(SMALL, -1, ())
    for r in range(reps + 1):                                                  # r = 0: warm-up (and the one upload of the reference and the mask)
        for what, m in mergers.items():
            st, bs = m.finish_bai(-1, -1, 1000, len(LENS))
            row = dict(finish_s=st.finish_s, sort_ms=st.sort_ms, gather_ms=st.gather_ms, deflate_ms=st.deflate_ms, index_ms=bs.index_ms)
            if what in rs:
                x = rs[what]
                row.update(recal_ms=x.recal_ms, hbm_bytes=x.hbm_bytes, n_records=x.n_records, n_bases=x.n_bases, n_err=x.n_err, n_masked=x.n_masked, n_rows=list(x.n_rows),
                           rc_bytes=x.rc_bytes)
            if what == "pileup":
                row.update(pileup_ms=ps.pileup_ms, observe_ms=ps.observe_ms)
            if what == "qc_25Mbp":
                row.update(qc_record_ms=qs.record_ms)
            if r:
                rows[what].append(row)
for what, v in rows.items():
    out[what] = {f: mm([x[f] for x in v]) for f in v[0] if f.endswith("_ms") or f == "finish_s"}
    if "recal_ms" in v[0]:
        out[what].update({f: v[0][f] for f in ("hbm_bytes", "n_records", "n_bases", "n_err", "n_masked", "n_rows", "rc_bytes")})
        gpu = [x["sort_ms"] + x["gather_ms"] + x["deflate_ms"] + x["index_ms"] + x["recal_ms"] for x in v]
        out[what]["recal_share_of_finish_gpu_time"] = mm([x["recal_ms"] / t for x, t in zip(v, gpu)], 4)
        out[what]["finish_over_unarmed_seconds"] = round(med([x["finish_s"] for x in v]) / med([x["finish_s"] for x in rows["unarmed"]]), 4)
        out[what]["recal_over_pileup_observe"] = round(med([x["recal_ms"] for x in v]) / med([x["observe_ms"] for x in rows["pileup"]]), 2)
        out[what]["recal_over_qc_record_pass"] = round(med([x["recal_ms"] for x in v]) / med([x["qc_record_ms"] for x in rows["qc_25Mbp"]]), 2)
        out[what]["recal_over_copy"] = round(med([x["recal_ms"] for x in v]) / med(copy_ms), 2)
out["record_bytes"] = n * 304
out["copy_same_bytes_ms"] = mm(copy_ms)
out["copy_TB_per_s_read_plus_write"] = round(2 * n * 304 / med(copy_ms) / 1e9, 2)
print(json.dumps(out))
