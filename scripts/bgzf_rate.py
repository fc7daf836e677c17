#!/usr/bin/env python3
"""BGZF blocks made on the GPU (csrc/k_bgzf.hip) on bench.py's default workload (1 M x 150 bp PE reads per batch, the cached 3.1 Gbp
index), in one process after a warm-up, the modes ALTERNATING: (1) the deflate stage by HIP events per batch and its share of the
batch's time on the GPU, (2) compressed bytes per read against zlib levels 1 and 6 on the same blocks (the first 1 000 blocks of the
batch), (3) the single-context resident rate with the records / the members left in HBM, (4) file to file to /dev/null over three
contexts: SAM, bwahip_stream_run_bam at levels 0 and 1, bwahip_stream_run_bam_dev.
Uses the FASTQ files a bench.py run left (bench_r0_[12].fq in $BWAHIP_BENCH_DIR) and the index in bench.py's cache directory.
Prints one JSON object; `python3 scripts/bgzf_rate.py [repetitions] > profiles/bgzf/bgzf_rate.json`."""
import json, os, statistics, sys, time, zlib
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
B = 65280
med = statistics.median


def member_sizes(buf):
    out, pos = [], 0
    while pos < len(buf):
        size = int.from_bytes(buf[pos + 16:pos + 18], "little") + 1
        out.append(size)
        pos += size
    return out


def zlen(block, level):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return len(z.compress(block) + z.flush())


out = {"workload": "1 M x 150 bp PE reads per batch (bench.py default)", "repetitions": reps}
with bw.Context(prefix, 0) as c0:
    with bw.FastqReader(fq1, fq2) as rd:
        arr, n = rd.next(K)
        # one batch through the host entry point leaves reads, names and qualities resident: the device-resident pairs then re-run it
        c0.process_seqs_text_array(arr, n, opt)
        runs = {"bam": [], "bgzf": []}
        for r in range(reps + 1):                                  # r = 0: warm-up
            for fmt in runs:
                t0 = time.time()
                ms = c0.batch_run_bam(opt) if fmt == "bam" else c0.batch_run_bgzf(opt)
                t1 = time.time()
                if r:
                    runs[fmt].append({"run_s": t1 - t0, "deflate_ms": ms.get("deflate", 0.0), "passes_ms": ms["k_sam_size"] + ms["k_sam_write"]})
        members, raw_len, n_blocks, n_stored = c0.batch_bgzf()    # the last run was bgzf
        c0.batch_run_bam(opt)
        rec = c0.batch_bam()
        assert raw_len == len(rec) and n_blocks == (len(rec) + B - 1) // B
        sizes = member_sizes(members)
        assert len(sizes) == n_blocks and sum(sizes) == len(members)
        pos = 0
        for i in range(min(50, n_blocks)):                         # a sample inflated here; the test suite judges the format
            z = zlib.decompressobj(wbits=-15)
            data = z.decompress(members[pos + 18:pos + sizes[i] - 8])
            assert z.eof and data == rec[i * B:(i + 1) * B] and int.from_bytes(members[pos + sizes[i] - 8:pos + sizes[i] - 4], "little") == zlib.crc32(data)
            pos += sizes[i]
        S = min(1000, n_blocks)
        blocks = [rec[i * B:(i + 1) * B] for i in range(S)]
        raw_s = sum(len(b) for b in blocks)
        reads_s = n * raw_s / len(rec)                              # reads the sampled blocks stand for
        gpu_s = sum(sizes[:S]) - 26 * S
        l1 = sum(zlen(b, 1) for b in blocks)
        l6 = sum(zlen(b, 6) for b in blocks)
        dm = [x["deflate_ms"] for x in runs["bgzf"]]
        share = [x["deflate_ms"] / (x["run_s"] * 1e3) for x in runs["bgzf"]]
        out["deflate_stage"] = {"ms_per_batch": [round(x, 3) for x in dm], "ms_median": round(med(dm), 3), "ms_min_max": [round(min(dm), 3), round(max(dm), 3)],
                                "share_of_batch_time_median": round(med(share), 4), "bam_passes_ms_median": round(med([x["passes_ms"] for x in runs["bgzf"]]), 3),
                                "blocks": n_blocks, "stored_blocks": n_stored, "raw_bytes": raw_len, "bgzf_bytes": len(members)}
        out["bytes_per_read"] = {"records": round(len(rec) / n, 1), "gpu_members_whole_batch": round(len(members) / n, 1),
                                 "sample_blocks": S, "gpu_deflate_payload": round(gpu_s / reads_s, 1), "zlib_level1": round(l1 / reads_s, 1), "zlib_level6": round(l6 / reads_s, 1),
                                 "gpu_over_level1": round(gpu_s / l1, 4), "gpu_over_level6": round(gpu_s / l6, 4), "gpu_over_raw": round(gpu_s / raw_s, 4)}
        out["resident_reads_per_s"] = {fmt: {"median": round(n / med([x["run_s"] for x in v])), "min_max": [round(n / max(x["run_s"] for x in v)), round(n / min(x["run_s"] for x in v))]}
                                       for fmt, v in runs.items()}
    ctxs = [c0, c0.clone(), c0.clone()]
    fd = os.open("/dev/null", os.O_WRONLY)
    stream = {"sam": [], "bam_level0": [], "bam_level1": [], "bam_dev": []}
    dev_stats = []
    for r in range(reps + 1):
        for what in stream:
            t0 = time.time()
            if what == "sam":
                st = bw.stream_run(ctxs, fq1, fq2, fd, opt, chunk_bases=K, reader_threads=8)
            elif what == "bam_dev":
                st, bs = bw.stream_run_bam_dev(ctxs, fq1, fq2, fd, None, opt, chunk_bases=K, reader_threads=8)
                if r:
                    dev_stats.append({"deflate_ms_per_batch": round(bs.deflate_ms / st.n_batches, 3), "gpu_busy_s": round(st.gpu_busy_s, 3), "write_s": round(st.write_s, 3),
                                      "bgzf_over_raw": round(bs.bgzf_bytes / bs.raw_bytes, 4), "stored": bs.n_stored})
            else:
                st = bw.stream_run_bam(ctxs, fq1, fq2, fd, None, int(what[-1]), opt, chunk_bases=K, reader_threads=8)
            if r:
                stream[what].append(st.n_reads / (time.time() - t0))
    os.close(fd)
    for c in ctxs[1:]:
        c.close()
    out["file_to_file_reads_per_s"] = {k: {"median": round(med(v)), "min_max": [round(min(v)), round(max(v))]} for k, v in stream.items()}
    out["bam_dev_stream"] = dev_stats
print(json.dumps(out))
