#!/usr/bin/env python3
"""What the table jump of k_smem is predicted to save, counted on the CPU: tests/smem_skip_model.c over reads of the benchmark
workload against the benchmark index (bench.py's cache; built when missing), the calls passes 1 and 2 of mem_collect_intv make.
Prints one JSON line: plain turns per read, skip turns per read and the fallback rate by min_intv for every depth asked for.

    python3 scripts/smem_skip_predict.py [--reads 2000] [--depths 12,13,14] [--genome-profile default] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-gpu_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--depths", default="12,13,14")
    ap.add_argument("--genome-mbp", type=int, default=None)
    ap.add_argument("--genome-profile", default="default", choices=["default", "human-like"])
    ap.add_argument("--sub-ppm", type=int, default=10000)
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    import bench
    import tools_py as tp
    import test_smem_skip_model as tm
    from common import bw
    mbp = args.genome_mbp or bench.DEFAULT_MBP
    t0 = time.time()
    bench.ensure_index(bw, tp, mbp, args.genome_profile)
    prefix = bench.index_prefix(mbp, args.genome_profile)
    lens = tp.contig_lengths(mbp * 1000000)
    genome = tp.read_fasta_bases(prefix + ".fa", lens)
    reads = tp.make_reads(genome, lens, args.reads, 150, sub_ppm=args.sub_ppm, seed=103, paired=True)
    del genome
    codes = np.ascontiguousarray(bw.NT4[reads.reshape(-1)])
    off = np.arange(args.reads + 1, dtype=np.int64) * reads.shape[1]
    with tempfile.TemporaryDirectory() as d:
        model = tm.Model(d, prefix)
        bench.log(f"index and {args.reads} reads ready: {time.time() - t0:.1f}s")
        res = {"reads": args.reads, "genome_mbp": mbp, "genome_profile": args.genome_profile, "sub_ppm": args.sub_ppm, "depths": {}}
        for depth in [int(x) for x in args.depths.split(",")]:
            s1, s2, by = model.collect((codes, off), depth)
            assert s1["diff"] == 0 and s2["diff"] == 0, (depth, s1, s2)
            plain, skip = s1["plain_turns"] + s2["plain_turns"], s1["skip_turns"] + s2["skip_turns"]
            res["plain_turns_per_read"] = round(plain / args.reads, 2)
            res["depths"][str(depth)] = {
                "skip_turns_per_read": round(skip / args.reads, 2), "ratio": round(skip / plain, 4),
                "lookups_per_read": round((s1["lookups"] + s2["lookups"]) / args.reads, 2),
                "calls_per_read": [round(s1["calls"] / args.reads, 3), round(s2["calls"] / args.reads, 3)],
                "fallbacks_per_read": [round(s1["fallbacks"] / args.reads, 4), round(s2["fallbacks"] / args.reads, 4)],
                "abandoned_turns_per_read": round((s1["abandoned_turns"] + s2["abandoned_turns"]) / args.reads, 2),
                "fallback_rate_by_min_intv": {str(m): [c, f] for m, (c, f) in enumerate(by) if c}}
            bench.log(f"J = {depth}: {res['depths'][str(depth)]}")
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
