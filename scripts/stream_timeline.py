#!/usr/bin/env python3
"""Where a bwahip_stream_run pass spends its time.

   BWAHIP_STREAM_LOG=1 python3 scripts/stream_only.py 3 3 2> stream.log
   python3 scripts/stream_timeline.py stream.log [kernel_trace.csv] [resident_kernel_seconds]

stream.log: the driver's `[bwahip] span <stage> batch <k> ctx <w> <begin ms> <end ms>` lines (times from the call), one group per pass,
each closed by the `[bwahip] stream: ... reallocations` line.  Stages: take (batch from the reader), stage (host gather into pinned
memory), h2d, hot (hot path), final (finalisation, up to the end of the write pass), d2h, write.  The LAST pass is evaluated.

kernel_trace.csv (rocprofv3 --kernel-trace of the same command): the kernels are split into passes at the longest idle gaps, and the
last pass gives the time some kernel was running and the idle time between its first and last kernel.  With resident_kernel_seconds
(the resident pipeline's time for the same reads, bench.py's gpu_pipeline) the excess of kernel-active time is printed too."""
import csv
import re
import sys

SPAN = re.compile(r"\[bwahip\] span (\w+) batch (\d+) ctx (\d+) ([-\d.]+) ([-\d.]+)")
END = re.compile(r"\[bwahip\] stream: (\d+) batches on (\d+) contexts, (\d+) buffer reallocations")
ORDER = ["take", "stage", "h2d", "hot", "final", "d2h", "write"]


def passes_of(path):
    out, cur = [], []
    for line in open(path, errors="replace"):
        m = SPAN.search(line)
        if m:
            cur.append((m.group(1), int(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5))))
            continue
        m = END.search(line)
        if m:
            out.append({"spans": cur, "batches": int(m.group(1)), "contexts": int(m.group(2)), "reallocations": int(m.group(3))})
            cur = []
    return out


def report_spans(p):
    sp = p["spans"]
    end = max(s[4] for s in sp)
    print(f"pass: {p['batches']} batches on {p['contexts']} contexts, call -> last byte written {end:.1f} ms, buffer reallocations {p['reallocations']}")
    print("stage      summed ms   mean ms   longest ms")
    for st in ORDER:
        d = [s[4] - s[3] for s in sp if s[0] == st]
        if d:
            print(f"{st:8s} {sum(d):11.1f} {sum(d) / len(d):9.1f} {max(d):12.1f}")
    hot0 = min(s[3] for s in sp if s[0] == "hot")
    finals = sorted(s[4] for s in sp if s[0] == "final")
    alone = finals[-2] if len(finals) > 1 else hot0
    print(f"start-up (call -> first hot path queued)             {hot0:8.1f} ms")
    print(f"drain (last batch alone: second-last finalisation ended -> last byte written) {end - alone:8.1f} ms")
    # time during which no context had a compute stage (hot or final) under way, between the first and the last
    ev = sorted([(s[3], 1) for s in sp if s[0] in ("hot", "final")] + [(s[4], -1) for s in sp if s[0] in ("hot", "final")])
    depth, t_prev, none_ms = 0, None, 0.0
    for t, dlt in ev:
        if depth == 0 and t_prev is not None:
            none_ms += t - t_prev
        depth += dlt
        t_prev = t
    print(f"no compute stage under way between first and last      {none_ms:8.1f} ms")
    print("batch ctx " + " ".join(f"{st:>15s}" for st in ORDER))
    for b in sorted({s[1] for s in sp}):
        row = {s[0]: s for s in sp if s[1] == b}
        ctx = next(iter(row.values()))[2]
        print(f"{b:5d} {ctx:3d} " + " ".join(f"{row[st][3]:7.1f}-{row[st][4]:7.1f}" if st in row else " " * 15 for st in ORDER))
    return end


def report_trace(path, n_passes, resident_s):
    iv = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path)))
    merged = []
    for a, b in iv:
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    gaps = sorted(((merged[i + 1][0] - merged[i][1], i) for i in range(len(merged) - 1)), reverse=True)
    cut = max(i for _, i in gaps[:max(1, n_passes)]) + 1 if n_passes > 1 else 0   # the last pass starts behind the last of the longest gaps
    last = merged[cut:]
    wall = (last[-1][1] - last[0][0]) / 1e9
    busy = sum(b - a for a, b in last) / 1e9
    print(f"kernel trace, last pass: first -> last kernel {wall:.3f} s, some kernel running {busy:.3f} s = {busy / wall:.3f}, idle in between {wall - busy:.3f} s"
          f" ({sum(1 for i in range(len(last) - 1) if last[i + 1][0] - last[i][1] > 1e6)} gaps over 1 ms)")
    if resident_s:
        print(f"kernel-active time above the resident pipeline's {resident_s:.3f} s: {busy - resident_s:+.3f} s")
    return wall


def main():
    ps = passes_of(sys.argv[1])
    end = report_spans(ps[-1]) if ps and ps[-1]["spans"] else None
    if len(sys.argv) > 2:
        n_passes = len(ps) if ps else int(sum(1 for line in open(sys.argv[1], errors="replace") if "[bwahip] stream:" in line))
        wall = report_trace(sys.argv[2], n_passes, float(sys.argv[3]) if len(sys.argv) > 3 else 0.0)
        if end is not None:
            print(f"outside first -> last kernel (start-up before the first kernel + after the last) {end / 1e3 - wall:.3f} s")


if __name__ == "__main__":
    main()
