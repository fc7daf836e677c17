#!/usr/bin/env python3
"""SAM text vs BAM records on bench.py's default workload (1 M x 150 bp PE reads per batch, the cached 3.1 Gbp index), the two formats
ALTERNATING in one process after a warm-up: (1) sizing + write pass (kernel_ms slots of the SAM stage) and bytes per read, (2) the
single-context resident rate with the download, (3) file to file to /dev/null over three contexts, SAM vs BAM at level 0 and level 1.
Uses the FASTQ files a bench.py run left (bench_r0_[12].fq in $BWAHIP_BENCH_DIR) and the index in bench.py's cache directory.
Prints one JSON object; `python3 scripts/bam_rate.py [repetitions] > profiles/bam/bam_rate.json`."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
bw = entry.load_bwahip()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
d = os.environ.get("BWAHIP_BENCH_DIR", "/dev/shm/bwahip_bench")
cache = os.environ.get("BWAHIP_BENCH_CACHE") or os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.expanduser("~/.cache"), "bwahip_bench")
prefix = os.path.join(cache, os.environ.get("BWAHIP_BENCH_INDEX", "g3100"))
fq1, fq2 = os.path.join(d, "bench_r0_1.fq"), os.path.join(d, "bench_r0_2.fq")
opt = bw.default_opt(); opt.flag |= 2; opt.n_threads = int(os.environ.get("BWAHIP_BENCH_HOST_THREADS", "16"))
K = 150000000
med = statistics.median
out = {"workload": "1 M x 150 bp PE reads per batch (bench.py default)", "repetitions": reps}
with bw.Context(prefix, 0) as c0:
    with bw.FastqReader(fq1, fq2) as rd:
        arr, n = rd.next(K)
        # one batch through the host entry point leaves reads, names and qualities resident: the device-resident pair then re-runs it
        c0.process_seqs_text_array(arr, n, opt)
        runs = {"sam": [], "bam": []}
        for r in range(reps + 1):                                  # r = 0: warm-up
            for fmt in ("sam", "bam"):
                t0 = time.time()
                ms = c0.batch_run_sam(opt) if fmt == "sam" else c0.batch_run_bam(opt)
                t1 = time.time()
                data = c0.batch_sam() if fmt == "sam" else c0.batch_bam()
                t2 = time.time()
                if r:
                    runs[fmt].append({"size_ms": ms["k_sam_size"], "write_ms": ms["k_sam_write"], "run_s": t1 - t0, "download_s": t2 - t1, "bytes": len(data)})
        for fmt, v in runs.items():
            passes = [x["size_ms"] + x["write_ms"] for x in v]
            out[fmt] = {"size_ms": [round(x["size_ms"], 3) for x in v], "write_ms": [round(x["write_ms"], 3) for x in v],
                        "passes_ms_median": round(med(passes), 3), "passes_ms_min_max": [round(min(passes), 3), round(max(passes), 3)],
                        "bytes_per_read": round(v[0]["bytes"] / n, 1),
                        "resident_reads_per_s_with_download": round(n / med([x["run_s"] + x["download_s"] for x in v])),
                        "resident_reads_per_s": round(n / med([x["run_s"] for x in v]))}
    ctxs = [c0, c0.clone(), c0.clone()]
    fd = os.open("/dev/null", os.O_WRONLY)
    stream = {"sam": [], "bam_level0": [], "bam_level1": []}
    for r in range(reps + 1):
        for what in stream:
            t0 = time.time()
            if what == "sam":
                st = bw.stream_run(ctxs, fq1, fq2, fd, opt, chunk_bases=K, reader_threads=8)
            else:
                st = bw.stream_run_bam(ctxs, fq1, fq2, fd, None, int(what[-1]), opt, chunk_bases=K, reader_threads=8)
            if r:
                stream[what].append(st.n_reads / (time.time() - t0))
    os.close(fd)
    for c in ctxs[1:]:
        c.close()
    out["file_to_file_reads_per_s"] = {k: {"median": round(med(v)), "min_max": [round(min(v)), round(max(v))]} for k, v in stream.items()}
print(json.dumps(out))
