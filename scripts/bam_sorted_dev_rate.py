#!/usr/bin/env python3
"""Coordinate-sorted BAM with the merge and the deflate on the GPU, on bench.py's default workload (1 M x 150 bp PE reads per batch, the
cached 3.1 Gbp index), after scripts/bam_sorted_rate.py: same workload, same warm-up, three contexts, output to /dev/null, the kinds
ALTERNATING in one process.  Kinds: bam_dev (unsorted, blocks made on the GPU: bwahip_stream_run_bam_dev), sorted_level1_in_memory (the
host merge in front of host zlib: bwahip_stream_run_bam_sorted with a budget that holds everything), and sorted_dev at piece_blocks 256,
1024 and 4096 (bwahip_stream_run_bam_sorted_dev with a budget that holds everything).  Per kind the median and min-max of reads/s; for the
device kinds also finish_s, the sort / gather / deflate milliseconds of the finish and hbm_bytes; and the resource usage of the kernels of
csrc/k_bammerge.hip, as hipcc reports it when it compiles the file the way the Makefile does.
Uses the FASTQ files a bench.py run left (bench_r0_[12].fq in $BWAHIP_BENCH_DIR) and the index in bench.py's cache directory.
Prints one JSON object; `python3 scripts/bam_sorted_dev_rate.py [repetitions] > profiles/bam_sorted_dev/bam_sorted_dev_rate.json`."""
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
out = {"workload": "1 M x 150 bp PE reads per batch (bench.py default)", "repetitions": reps, "contexts": 3}


def kernel_resource_usage():
    """kernel -> registers, scratch, occupancy and LDS from -Rpass-analysis=kernel-resource-usage (device code only, nothing is kept)"""
    csrc = os.path.join(ROOT, "bwa-mem-gpu_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--offload-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "k_bammerge.hip"), "-o", os.devnull], capture_output=True, text=True)
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
    ctxs = [c0, c0.clone(), c0.clone()]
    fd = os.open("/dev/null", os.O_WRONLY)
    tmp = tempfile.mkdtemp(prefix="bwahip_sorted_dev_", dir=os.environ.get("BWAHIP_SORT_TMP", d))
    kinds = ["bam_dev", "sorted_level1_in_memory", "sorted_dev_pb256", "sorted_dev_pb1024", "sorted_dev_pb4096"]
    stream = {k: [] for k in kinds}
    for r in range(reps + 1):                                      # r = 0: warm-up
        for what in kinds:
            t0 = time.time()
            if what == "bam_dev":
                st, bs = bw.stream_run_bam_dev(ctxs, fq1, fq2, fd, None, opt, chunk_bases=K, reader_threads=8)
                row = {"reads_per_s": st.n_reads / (time.time() - t0)}
            elif what == "sorted_level1_in_memory":
                st, so = bw.stream_run_bam_sorted(ctxs, fq1, fq2, fd, None, 1, opt, chunk_bases=K, reader_threads=8, tmp_dir=tmp, mem_budget=1 << 40)
                row = {"reads_per_s": st.n_reads / (time.time() - t0), "finish_s": so.merge_s, "n_runs": so.n_runs, "n_records": so.n_records}
            else:
                st, sd = bw.stream_run_bam_sorted_dev(ctxs, fq1, fq2, fd, None, opt, chunk_bases=K, reader_threads=8, hbm_budget=1 << 40,
                                                      piece_blocks=int(what.split("pb")[1]), tmp_dir=tmp)
                row = {"reads_per_s": st.n_reads / (time.time() - t0), "finish_s": sd.dev.finish_s, "n_runs": sd.n_runs, "n_records": sd.n_records,
                       "fell_back": sd.fell_back, "sort_ms": sd.dev.sort_ms, "gather_ms": sd.dev.gather_ms, "deflate_ms": sd.dev.deflate_ms,
                       "hbm_bytes": sd.dev.hbm_bytes, "raw_bytes": sd.dev.raw_bytes, "bgzf_bytes": sd.dev.bgzf_bytes, "n_blocks": sd.dev.n_blocks,
                       "n_stored": sd.dev.n_stored, "batch_sort_ms": sd.sort_ms}
            row["n_reads"] = st.n_reads
            if r:
                stream[what].append(row)
    os.close(fd)
    os.rmdir(tmp)
    for c in ctxs[1:]:
        c.close()
    f2f = {}
    for k, v in stream.items():
        f2f[k] = {"reads_per_s": mm([x["reads_per_s"] for x in v], 0), "n_reads": v[0]["n_reads"]}
        if "finish_s" in v[0]:
            f2f[k].update(finish_s=mm([x["finish_s"] for x in v]), n_runs=v[0]["n_runs"], n_records=v[0]["n_records"])
        if "hbm_bytes" in v[0]:
            f2f[k].update(sort_ms=mm([x["sort_ms"] for x in v], 2), gather_ms=mm([x["gather_ms"] for x in v], 2), deflate_ms=mm([x["deflate_ms"] for x in v], 2),
                          hbm_bytes=mm([x["hbm_bytes"] for x in v], 0), fell_back=max(x["fell_back"] for x in v), raw_bytes=v[0]["raw_bytes"],
                          bgzf_bytes=v[0]["bgzf_bytes"], n_blocks=v[0]["n_blocks"], n_stored=v[0]["n_stored"],
                          batch_sort_ms_all_batches=mm([x["batch_sort_ms"] for x in v], 2))
    out["file_to_file"] = f2f
    lo = min(f2f[k]["reads_per_s"]["min_max"][0] for k in kinds if k.startswith("sorted_dev"))
    out["sorted_dev_ranges_wholly_above_host_merge"] = {k: f2f[k]["reads_per_s"]["min_max"][0] > f2f["sorted_level1_in_memory"]["reads_per_s"]["min_max"][1]
                                                        for k in kinds if k.startswith("sorted_dev")}
    out["lowest_sorted_dev_reads_per_s"] = lo
print(json.dumps(out))
