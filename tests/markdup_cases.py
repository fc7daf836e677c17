"""The synthetic data of the duplicate-marking tests (tests/test_markdup_cpu.py, tests/test_gpu_markdup.py): BAM records in the style of
tests/bai_cases.py::rec but with sequence and quality bytes, grouped into reads and templates in input order, and descriptor sets for the
decision alone.  assert_families checks on the judge's own output (tests/markdup_ref.py) that every family the tests are about is in the
set, so that the set cannot quietly lose one."""
import random
import struct

import numpy as np

import markdup_ref as ref

M, I, D, N, S, H, P, EQ, X = range(9)
N_SEQS, LONGEST = 5, 2 ** 31 - 1                   # the synthetic index the records' sort keys are packed for (tests/bam_sort_ref.py::packed_key)
DESC_DTYPE = np.dtype([("end", np.uint64, (2,)), ("score", np.uint32), ("kind", np.uint32)])   # bwahip_dup_desc_t


def rec(name, ref_id, pos, cigar=(), flag=0, quals=b"", tags=b""):
    """One record: l_seq = len(quals) bases (all 'A'), these quality bytes, these CIGAR operations [(length, op)]."""
    name = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), 60, 0, len(cigar), flag, len(quals), -1, -1, 0) + name
    body += b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar)
    body += b"\x11" * ((len(quals) + 1) // 2) + bytes(quals) + tags
    return struct.pack("<i", len(body)) + body


def _q(rng, n, kind):
    if kind == "none":
        return b"\xff" * n
    if kind == "edge":                           # around the threshold: 14 does not count, 15 does
        return bytes(rng.choice((13, 14, 15, 16)) for _ in range(n))
    if kind == "low":
        return bytes(rng.randrange(0, 15) for _ in range(n))
    return bytes(rng.randrange(2, 42) for _ in range(n))


# alignments the templates draw from, so that equal unclipped ends come up by different routes: (ref, pos, cigar, reverse)
SHAPES = [
    (0, 1000, [(50, M)], False), (0, 1005, [(5, S), (45, M)], False), (0, 1007, [(3, H), (4, S), (43, M)], False),      # u5 = 1000 three ways
    (0, 951, [(50, M)], True), (0, 961, [(40, M), (10, S)], True), (0, 966, [(35, M), (6, S), (9, H)], True),           # u5 = 1000, reverse, three ways
    (0, 1000, [(50, M)], True),                                                                                       # pos 1000 but u5 = 1049
    (0, 3, [(10, S), (40, M)], False), (0, 2, [(9, H), (41, M)], False),                                               # u5 = -7
    (1, 500, [(20, M), (5, D), (10, M), (7, N), (13, EQ), (7, X)], False), (1, 500, [(20, M), (5, D), (10, M), (7, N), (13, EQ), (7, X)], True),   # rlen 62
    (1, 561, [(30, S), (20, I)], True), (1, 561, [(50, S)], True), (1, 591, [(30, S), (20, I)], False),                 # rlen = 0: reverse u5 = 561 (+ 50 when all is clipped), forward 561
    (2, 77, [(25, M), (3, I), (22, M)], False), (2, 77, [(25, M), (3, I), (22, M)], True),
    (2, 300, [(4, H), (40, M), (6, S)], False), (2, 300, [(40, M), (6, H)], False), (2, 261, [(5, S), (40, M)], True), (2, 261, [(3, H), (40, M), (5, S)], True),   # clips at the 3' end: they do not count
    (4, 10, [(50, M)], False), (3, 2 ** 31 - 60, [(50, M)], True),                                                    # the highest contig; u5 close to 2^31
]

FRAG_ONLY = [(1, 90000, [(2, S), (48, M)], False), (1, 90000, [(50, M)], True)]


def _reads(rng, paired, n_tmpl):
    """n_tmpl templates in input order: a list of (name, reads), reads = the record lists of its one or two reads."""
    out = []
    for t in range(n_tmpl):
        name = b"t%d" % t + b"x" * (t % 5)                           # names of varying length: records begin at every alignment
        reads = []
        for k in range(2 if paired else 1):
            mate = (0x1 | (0x40 if k == 0 else 0x80)) if paired else 0
            ref_id, pos, cigar, rev = SHAPES[rng.randrange(len(SHAPES))] if t % 7 else SHAPES[(t // 7 + k) % len(SHAPES)]
            lone = paired and t % 11 == 5                            # a fragment where no pair has an end: the mate unmapped, a place of its own
            if lone:
                ref_id, pos, cigar, rev = FRAG_ONLY[t // 11 % len(FRAG_ONLY)]
            n = sum(x for x, op in cigar if op in (M, I, S, EQ, X))
            quals = _q(rng, n, rng.choice(("none", "edge", "edge", "low", "any", "any", "any")))
            style = rng.randrange(12)
            if lone:
                style = 0 if k else 11
            if style == 0:                                           # unmapped, with a CIGAR and a position that must not count
                recs = [rec(name, ref_id, pos, cigar, mate | 0x4, quals)]
            elif style == 1:                                         # no primary record at all
                recs = [rec(name, ref_id, pos, cigar, mate | 0x800 | (0x10 if rev else 0), quals), rec(name, 0, 5, [(n, M)], mate | 0x100, quals)]
            elif style == 2:                                         # a supplementary before and a secondary after the primary
                recs = [rec(name, 4, 9, [(10, M), (n - 10, H)], mate | 0x800, quals[:10], tags=b"SAZx\0"),
                        rec(name, ref_id, pos, cigar, mate | (0x10 if rev else 0), quals),
                        rec(name, 0, 1000, [(n, M)], mate | 0x100, b"\xff" * n)]
            elif style == 3:                                         # two primaries: the first counts, in the batch and (it sorts first) in the file; an unmapped secondary is never marked
                recs = [rec(name, ref_id, pos, cigar, mate | (0x10 if rev else 0), quals), rec(name, ref_id, pos + 5, [(n, M)], mate, quals),
                        rec(name, -1, -1, [], mate | 0x100 | 0x4, quals)]
            else:
                recs = [rec(name, ref_id, pos, cigar, mate | (0x10 if rev else 0), quals, tags=b"X" * rng.randrange(0, 4))]
            reads.append(recs)
        out.append((name, reads))
    return out


def record_set(paired, n_tmpl=420, seed=5):
    """dict(templates, names, reads = all reads in input order, buf / off = their records concatenated with the reads' offsets)."""
    rng = random.Random(seed + paired)
    tm = _reads(rng, paired, n_tmpl)
    reads = [r for _, rr in tm for r in rr]
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([sum(map(len, r)) for r in reads])
    return dict(templates=tm, names=[n for n, _ in tm], reads=reads, buf=b"".join(x for r in reads for x in r), off=off, paired=paired)


def judge_descs(case):
    return [ref.describe_reads(rr) for _, rr in case["templates"]]


def as_desc_array(descs):
    a = np.zeros(len(descs), dtype=DESC_DTYPE)
    for i, (e0, e1, sc, kind) in enumerate(descs):
        a[i] = ((e0, e1), sc, kind)
    return a


def assert_record_families(case):
    """On the judge's output for a record set: every family is there."""
    parsed = [[ref.parse(x) for x in r] for r in case["reads"]]
    prim = [next((p for p in rr if not p["flag"] & 0x900), None) for rr in parsed]
    mapped = [p for p in prim if p and not p["flag"] & 0x4]
    clip = lambda p, end, op: p["cigar"] and p["cigar"][end][1] == op
    for rev in (0, 0x10):
        for end in (0, -1):
            for op in (S, H):
                assert any(p["flag"] & 0x10 == rev and clip(p, end, op) for p in mapped), (rev, end, op)
    assert any(ref.u5_of(p) < 0 for p in mapped)
    assert any(not any(op in ref.REF_OPS for _, op in p["cigar"]) for p in mapped if p["flag"] & 0x10) and any(not any(op in ref.REF_OPS for _, op in p["cigar"]) for p in mapped if not p["flag"] & 0x10)
    assert any(p["qual"][:1] == b"\xff" for p in mapped) and any(14 in p["qual"] and 15 in p["qual"] for p in mapped)
    assert any(sum(1 for p in rr if p["flag"] & 0x800) and sum(1 for p in rr if p["flag"] & 0x100) and pr for rr, pr in zip(parsed, prim))
    assert any(pr is None for pr in prim) and any(pr and pr["flag"] & 0x4 for pr in prim)
    assert any(sum(1 for p in rr if not p["flag"] & 0x900) > 1 for rr in parsed)
    starts = set()
    o = 0
    for r in case["reads"]:
        for x in r:
            starts.add(o % 4)
            o += len(x)
    assert starts == {0, 1, 2, 3}                                    # records at odd addresses
    descs = judge_descs(case)
    assert {d[3] for d in descs} == ({0, 1, 2} if case["paired"] else {0, 1})
    dup, cls = ref.decide(descs)
    want = ("pair", "frag_pair", "frag_frag", "kept_pair", "kept_frag") if case["paired"] else ("frag_frag", "kept_frag")
    for k in want:
        assert k in cls, k
    if case["paired"]:                                               # a pair that shadows a fragment
        ends = {e for d in descs if d[3] == 2 for e in d[:2]}
        assert any(d[3] == 1 and d[0] in ends for d in descs)


# ---------------------------------------------------------------------------------------------------------------- descriptor sets
def _pair(a, b, score):
    return (min(a, b), max(a, b), score, 2)


def desc_sets():
    """name -> list of (end0, end1, score, kind) in input order."""
    w = ref.end_word
    rng = random.Random(77)
    sets = {"n0": [], "n1_pair": [_pair(w(0, 5, 0), w(0, 300, 1), 9)], "n1_frag": [(w(1, 5, 0), 0, 3, 1)], "n1_none": [(0, 0, 0, 0)],
            "n2_same": [_pair(w(0, 5, 0), w(0, 300, 1), 9)] * 2, "n2_frag_pair": [(w(0, 300, 1), 0, 900, 1), _pair(w(0, 5, 0), w(0, 300, 1), 1)]}
    a, b, c = w(0, 100, 0), w(0, 400, 1), w(0, 401, 1)
    hi = [w(r, 100, 0) for r in (1, 2, 3, 1 << 20)]                   # differ only above bit 32
    assert len({x & 0x1ffffffff for x in hi}) == 1
    sets["small"] = [
        _pair(a, b, 10), _pair(a, b, 10), _pair(a, b, 11), _pair(a, b, 11), (0, 0, 0, 0),       # ties decided by order: the third is kept
        _pair(a, c, 10), _pair(a, c, 9),                                                       # equal end[0], another end[1]: a cluster of its own
        (b, 0, 1000, 1), (c, 0, 5, 1), (a, 0, 7, 1),                                            # fragments at a pair's second and first end
        (w(0, 999, 0), 0, 5, 1), (w(0, 999, 0), 0, 5, 1), (w(0, 999, 0), 0, 6, 1), (w(0, 999, 1), 0, 1, 1),   # fragments with no pair at their end
        _pair(hi[0], hi[1], 3), _pair(hi[0], hi[2], 3), _pair(hi[3], hi[1], 3), _pair(hi[0], hi[1], 3), (hi[2], 0, 1, 1), (w(4, 100, 0), 0, 1, 1), (w(4, 100, 0), 0, 1, 1),
        (0, 0, 0, 0), _pair(0, 0, 1), _pair(0, 0, 2), (0, 0, 4, 1),                             # the end word 0 (refID 0, u5 = -2^31, forward) is an end word like any other
    ]
    big = [_pair(a, b, rng.choice((5, 5, 6))) for _ in range(4500)] + [(w(2, 1, 1), 0, rng.choice((1, 2)), 1) for _ in range(4200)]   # more than one tile of the radix sort each
    rng.shuffle(big)
    sets["big_cluster"] = big
    ends = [w(rng.randrange(3), rng.randrange(0, 600), rng.randrange(2)) for _ in range(1500)]
    rnd = []
    for _ in range(10000):
        k = rng.choice((0, 1, 1, 2, 2, 2))
        rnd.append((0, 0, 0, 0) if k == 0 else (rng.choice(ends), 0, rng.randrange(0, 4), 1) if k == 1 else _pair(rng.choice(ends[:200]), rng.choice(ends[:200]), rng.randrange(0, 4)))
    sets["random"] = rnd
    return sets


def assert_desc_families(sets):
    assert {len(sets[k]) for k in ("n0", "n1_pair", "n2_same")} == {0, 1, 2}
    for name in ("small", "big_cluster", "random"):
        dup, cls = ref.decide(sets[name])
        if name != "big_cluster":
            assert {d[3] for d in sets[name]} == {0, 1, 2}
            for k in ("pair", "frag_pair", "frag_frag", "kept_pair", "kept_frag"):
                assert k in cls, (name, k)
    dup, cls = ref.decide(sets["small"])
    assert dup[:4] == [1, 1, 0, 1] and dup[5:7] == [0, 1] and dup[7:10] == [1, 1, 1] and dup[10:14] == [1, 1, 0, 0]
    sigs = {}
    for d in sets["big_cluster"]:
        sigs[d[:2]] = sigs.get(d[:2], 0) + 1
    assert max(sigs.values()) > 4096 and min(sigs.values()) > 4096
    dup, _ = ref.decide(sets["big_cluster"])
    assert len(dup) - sum(dup) == 2
    rnd = {}
    for d in sets["random"]:
        if d[3]:
            rnd[d[:2]] = rnd.get(d[:2], 0) + 1
    assert len(sets["random"]) >= 10000 and sum(1 for v in rnd.values() if v > 1) > 500
