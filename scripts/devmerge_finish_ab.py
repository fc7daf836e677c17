#!/usr/bin/env python3
"""The device merger's marked, indexed finish of two or more builds of this repository against each other at full precision: the
libraries of the given trees are loaded into ONE process (each has its own context and its own mergers on the same device), every merger
holds the record set of scripts/bam_spill_rate.py (N synthetic 304-byte records in N / 2 pairs, 8 runs) resident and spilled to pinned
memory, and bwahip_bam_devmerger_finish_markdup with the index (output dropped) ALTERNATES between them, the order reversed every other
repetition, one warm-up first.  scripts/bam_spill_rate.py and scripts/markdup_rate.py round seconds to a millisecond; this does not.
The contexts are created in the order the trees are given: give them in both orders to see what that order costs.
    python3 scripts/devmerge_finish_ab.py <index prefix> <records> <repetitions> name=<tree> name=<tree> ... > profiles/devmerge_finish/ab_<names>.json
A tree is a checkout that has been built (bwa-mem-gpu_amd/bwahip.py and libbwahip.so).  Prints one JSON object: per tree and mode the
median, minimum and maximum of finish_s and of the stages' event times."""
import importlib.util, json, os, statistics, sys
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
prefix, n_arg, reps = sys.argv[1], sys.argv[2], int(sys.argv[3])
trees = [a.split("=", 1) for a in sys.argv[4:]]
head = open(os.path.join(HERE, "scripts", "bam_spill_rate.py")).read().split("\nout = {")[0]     # the record set, as that script makes it
sys.argv = ["bam_spill_rate.py", prefix, n_arg]
g = {"__name__": "bam_spill_rate_head", "__file__": os.path.join(HERE, "scripts", "bam_spill_rate.py")}
exec(compile(head, "bam_spill_rate_head", "exec"), g)
recs, key_of, T, n_runs, LENS = g["recs"], g["key_of"], g["T"], g["n_runs"], g["LENS"]
libs = {}
for name, tree in trees:
    spec = importlib.util.spec_from_file_location("bwahip_" + name, os.path.join(tree, "bwa-mem-gpu_amd", "bwahip.py"))
    libs[name] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(libs[name])
assert len({bw.lib()._name for bw in libs.values()}) == len(libs), "two names for one library"
ctxs = {name: bw.Context(prefix, 0) for name, bw in libs.items()}
mergers = {}
for name, bw in libs.items():
    for mode in ("resident", "spilled_mem"):
        mergers[(name, mode)] = m = bw.DevMerger(ctxs[name], 0)
        if mode != "resident":
            m.set_spill(1 << 40, None, 0)
bounds = [T * k // n_runs for k in range(n_runs + 1)]
for k in range(n_runs):
    run = recs[bounds[k]:bounds[k + 1]].reshape(-1)
    keys = key_of(run)
    order = np.argsort(keys, kind="stable")
    srt, off = run[order].tobytes(), np.arange(len(run) + 1, dtype=np.int64) * 304
    desc = ctxs[trees[0][0]].kat_dup_desc(run.tobytes(), off, True)
    for (name, mode), m in mergers.items():
        (m.add_dup if mode == "resident" else m.add_spilled)(k, srt, keys[order], off, (order // 2).astype(np.uint32), desc)
FIELDS = ("finish_s", "sort_ms", "gather_ms", "deflate_ms", "index_ms", "markdup_ms", "decide_ms", "mark_ms")
rows = {k: [] for k in mergers}
for r in range(reps + 1):                                                          # r = 0: warm-up
    for key in (list(mergers) if r % 2 else list(mergers)[::-1]):
        st, bs, ms = mergers[key].finish_markdup(-1, -1, 1000, len(LENS))
        if r:
            rows[key].append(dict(finish_s=st.finish_s, sort_ms=st.sort_ms, gather_ms=st.gather_ms, deflate_ms=st.deflate_ms, index_ms=bs.index_ms, markdup_ms=ms.markdup_ms,
                                  decide_ms=ms.decide_ms, mark_ms=ms.mark_ms, written=(st.bgzf_bytes, ms.n_marked)))
assert len({x["written"] for v in rows.values() for x in v}) == 1, "the builds did not write the same file"
out = {"workload": f"{2 * T} synthetic 304-byte records, {n_runs} runs", "repetitions": reps, "contexts_created_in_this_order": [n for n, _ in trees]}
for (name, mode), v in rows.items():
    out[f"{name}_{mode}"] = {f: {"median": round(statistics.median(x[f] for x in v), 6), "min_max": [round(min(x[f] for x in v), 6), round(max(x[f] for x in v), 6)]} for f in FIELDS}
    out[f"{name}_{mode}"]["gpu_stages_ms"] = round(statistics.median(sum(x[f] for f in FIELDS[1:6]) for x in v), 3)
for m in mergers.values():
    m.close()
for c in ctxs.values():
    c.close()
print(json.dumps(out))
