#!/usr/bin/env python3
"""Coordinate-sorted BAM on bench.py's default workload (1 M x 150 bp PE reads per batch, the cached 3.1 Gbp index), after
scripts/bam_rate.py: same workload, same warm-up, sorted and unsorted ALTERNATING in one process.  (1) The sort stage on the GPU --
record table, radix sort, gather, as HIP events -- next to the two BAM passes (sizing + write) of the same runs, the radix passes that
ran, and the gather's bytes moved / time; (2) file to file to /dev/null over three contexts at level 0 and level 1: the unsorted
bwahip_stream_run_bam against bwahip_stream_run_bam_sorted with a budget that holds everything and with mem_budget = 0.
(3) the resource usage of the kernels of csrc/k_bamsort.hip, as hipcc reports it when it compiles the file the way the Makefile does.
Uses the FASTQ files a bench.py run left (bench_r0_[12].fq in $BWAHIP_BENCH_DIR) and the index in bench.py's cache directory.
Prints one JSON object; `python3 scripts/bam_sorted_rate.py [repetitions] > profiles/bam_sorted/bam_sorted_rate.json`."""
import json, os, re, statistics, subprocess, sys, tempfile, time
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
mm = lambda v, nd=3: {"median": round(med(v), nd), "min_max": [round(min(v), nd), round(max(v), nd)]}
out = {"workload": "1 M x 150 bp PE reads per batch (bench.py default)", "repetitions": reps}


def kernel_resource_usage():
    """kernel -> registers, scratch, occupancy and LDS from -Rpass-analysis=kernel-resource-usage (device code only, nothing is kept)"""
    csrc = os.path.join(ROOT, "bwa-mem-gpu_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--offload-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "k_bamsort.hip"), "-o", os.devnull], capture_output=True, text=True)
    if r.returncode:
        return {"error": r.stderr[-500:]}
    names = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
             "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes_per_block"}
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z][^:]*): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            k = re.search(r"\d(k_[a-z_]+)E", m.group(1))
            cur = usage.setdefault(k.group(1) if k else m.group(1), {})
        elif cur is not None and m.group(2).strip() in names:
            cur[names[m.group(2).strip()]] = int(m.group(3))
    return usage


out["kernel_resource_usage"] = kernel_resource_usage()
with bw.Context(prefix, 0) as c0:
    out["key_bits"] = bw.bam_sort_key_bits(c0)
    with bw.FastqReader(fq1, fq2) as rd:
        arr, n = rd.next(K)
        c0.process_seqs_text_array(arr, n, opt)                    # leaves reads, names and qualities resident
        runs = {"bam": [], "sorted": []}
        for r in range(reps + 1):                                  # r = 0: warm-up
            for fmt in runs:
                ms = c0.batch_run_bam(opt) if fmt == "bam" else c0.batch_run_bam_sorted(opt)
                if fmt == "sorted":
                    rec, keys, off = c0.batch_bam_sorted()
                    ms["bytes"], ms["n_rec"] = len(rec), len(keys)
                if r:
                    runs[fmt].append(ms)
        srt = runs["sorted"]
        stage = [x["sort_table"] + x["sort_radix"] + x["sort_gather"] for x in srt]
        nb, nr = srt[0]["bytes"], srt[0]["n_rec"]
        out["per_batch"] = {"reads": n, "records": nr, "record_bytes": nb}
        out["bam_passes_ms"] = {"unsorted_runs": mm([x["k_sam_size"] + x["k_sam_write"] for x in runs["bam"]]),
                                "sorted_runs": mm([x["k_sam_size"] + x["k_sam_write"] for x in srt])}
        out["sort_stage_ms"] = {"total": mm(stage), "record_table": mm([x["sort_table"] for x in srt]), "radix_sort": mm([x["sort_radix"] for x in srt]),
                                "gather": mm([x["sort_gather"] for x in srt]), "radix_passes": srt[0]["sort_passes"]}
        g = med([x["sort_gather"] for x in srt])
        # the gather reads and writes every record byte once, and per record 4 (ordinal) + 8 (offset) + 4 (length) + 2 x 8 (output offsets) + 4 + 4 (sorted lengths) bytes
        moved = 2 * nb + 40 * nr
        out["gather"] = {"bytes_moved": moved, "GB_per_s": round(moved / (g * 1e-3) / 1e9, 1), "fraction_of_8TBps_peak": round(moved / (g * 1e-3) / 8e12, 3)}
    ctxs = [c0, c0.clone(), c0.clone()]
    fd = os.open("/dev/null", os.O_WRONLY)
    tmp = tempfile.mkdtemp(prefix="bwahip_sorted_", dir=os.environ.get("BWAHIP_SORT_TMP", d))
    kinds = ["bam_level0", "sorted_level0_in_memory", "sorted_level0_budget0", "bam_level1", "sorted_level1_in_memory", "sorted_level1_budget0"]
    stream = {k: [] for k in kinds}
    for r in range(reps + 1):
        for what in kinds:
            level = int(what.split("level")[1][0])
            t0 = time.time()
            if what.startswith("bam"):
                st = bw.stream_run_bam(ctxs, fq1, fq2, fd, None, level, opt, chunk_bases=K, reader_threads=8)
                row = {"reads_per_s": st.n_reads / (time.time() - t0)}
            else:
                st, so = bw.stream_run_bam_sorted(ctxs, fq1, fq2, fd, None, level, opt, chunk_bases=K, reader_threads=8, tmp_dir=tmp,
                                                  mem_budget=0 if what.endswith("budget0") else 1 << 40)
                row = {"reads_per_s": st.n_reads / (time.time() - t0), "merge_s": so.merge_s, "spilled_bytes": so.spilled_bytes, "sort_ms": so.sort_ms,
                       "n_runs": so.n_runs, "n_records": so.n_records, "seconds": st.seconds}
            if r:
                stream[what].append(row)
    os.close(fd)
    os.rmdir(tmp)
    for c in ctxs[1:]:
        c.close()
    f2f = {}
    for k, v in stream.items():
        f2f[k] = {"reads_per_s": mm([x["reads_per_s"] for x in v], 0)}
        if "merge_s" in v[0]:
            f2f[k].update(merge_s=mm([x["merge_s"] for x in v]), seconds=mm([x["seconds"] for x in v]), spilled_bytes=v[0]["spilled_bytes"],
                          n_runs=v[0]["n_runs"], n_records=v[0]["n_records"], gpu_sort_ms_all_batches=mm([x["sort_ms"] for x in v], 2))
    out["file_to_file"] = f2f
print(json.dumps(out))
