"""The synthetic records of the pileup tests (tests/test_pileup_cpu.py, tests/test_gpu_pileup.py): minimal BAM records with real SEQ and QUAL,
built by hand over small random references whose lengths sit at 1, around the 2-bit packing (3, 4, 5), the wavefront (64) and the workgroup
(256), and one of several thousand bases; their order puts a contig's first base at every phase of a .pac byte.  assert_families checks on
the judge's own reading (tests/pileup_ref.py) that everything the tests are about is in the set, so that it cannot quietly lose one."""
import random
import struct

import numpy as np

import pileup_ref as ref
from pileup_ref import D, EQ, H, I, M, N, P, S, X

REF_LEN = [1, 5, 65, 3, 257, 4, 63, 64, 255, 256, 5000, 400, 3000]
BIG, STACK_REF, QUIET = 10, 11, 12                                   # the random reads end at BIG; the other two hold what is planted alone
STACK_POS = 200
L_SEQS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 700)
MAPQS = (0, 19, 20, 29, 30, 60, 255)
MIN_BASEQ, MIN_MAPQ = 20, 30                                         # what the option sets of the tests use beside 0
QUALS = (MIN_BASEQ - 1, MIN_BASEQ, 2, 30, 41, 93)
CODE = (1, 2, 4, 8)


def reference(seed=7):
    rng = random.Random(seed)
    return [[rng.randrange(4) for _ in range(n)] for n in REF_LEN]


def rec(name, ref_id, pos, cigar=(), seq=(), qual=None, flag=0, mapq=60, tail=b"", l_seq=None):
    """One record: 36 bytes, the name, the CIGAR operations [(length, op)], the bases (BAM codes) packed two a byte, the qualities, `tail`.
    l_seq: what the record says, when that is not len(seq)."""
    name = name + b"\0"
    seq = list(seq)
    qual = bytes([30] * len(seq)) if qual is None else bytes(qual)
    assert len(qual) == len(seq)
    packed = bytes((seq[k] << 4) | (seq[k + 1] if k + 1 < len(seq) else 0) for k in range(0, len(seq), 2))
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), mapq, 0, len(cigar), flag, len(seq) if l_seq is None else l_seq, -1, -1, 0) + name
    body += b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar) + packed + qual + tail
    return struct.pack("<i", len(body)) + body


def read_over(refs, r, pos, cigar, rng=None, rate=0.0, edits=None):
    """The bases of a read that follows contig r from pos through the CIGAR: the reference's own bases under M = X (beyond the contig:
    A), random ones for I and S; every base mutated with probability `rate`; edits: {query index: BAM code} on top."""
    seq, p = [], pos
    for n, op in cigar:
        if op in (M, EQ, X):
            for j in range(n):
                b = refs[r][p + j] if 0 <= p + j < len(refs[r]) else 0
                if rng and rng.random() < rate:
                    b = (b + rng.randrange(1, 4)) % 4
                seq.append(CODE[b])
            p += n
        elif op in (I, S):
            seq += [CODE[rng.randrange(4)] if rng else 1 for _ in range(n)]
        elif op in (D, N):
            p += n
    for q, code in (edits or {}).items():
        seq[q] = code
    return seq


def _cigar(rng, l_seq):
    """A CIGAR of query length l_seq."""
    k = rng.randrange(8) if l_seq >= 12 else 0
    if k == 0:
        return [(l_seq, M)]
    a = (l_seq - 6) // 2
    b = l_seq - 6 - a
    if k == 1:
        return [(2, S), (a, M), (4, I), (b, M)]
    if k == 2:
        return [(a + 2, M), (rng.randrange(1, 7), D), (b + 2, EQ), (2, X)]
    if k == 3:
        return [(rng.randrange(1, 9), H), (a + 3, M), (rng.randrange(1, 60), N), (b, M), (3, S)]
    if k == 4:
        return [(a + 4, EQ), (rng.randrange(1, 3), P), (b, X), (2, S), (rng.randrange(1, 5), H)]
    if k == 5:
        return [(a, M), (2, N), (3, D), (1, I), (b + 5, M)]
    if k == 6:
        return [(l_seq - 3, S), (3, I)]                                                  # nothing on the reference
    return [(3, I), (l_seq - 6, M), (3, S)]                                              # an insertion in front of the first reference base


def _flag(rng):
    f = 0x10 if rng.random() < 0.5 else 0
    for bit, p in ((0x1, 0.5), (0x4, 0.04), (0x100, 0.04), (0x800, 0.05), (0x400, 0.08), (0x200, 0.06)):
        if rng.random() < p:
            f |= bit
    return f


def _quals(rng, n):
    if rng.random() < 0.1:
        return [0xff] * n                                                                  # no qualities: every base passes
    return [rng.choice(QUALS) for _ in range(n)]


def record_set(seed=3, n_random=2400):
    rng = random.Random(seed)
    refs = reference()
    out = []
    for k in range(n_random):
        r = rng.randrange(BIG) if rng.random() < 0.5 else BIG
        L = REF_LEN[r]
        l_seq = rng.choice(L_SEQS) if r == BIG or rng.random() < 0.3 else rng.choice((1, 15, 16, 17))
        pos = rng.randrange(0, L)
        cig = _cigar(rng, l_seq)
        seq = read_over(refs, r, pos, cig, rng, 0.04)
        if rng.random() < 0.2:
            seq[rng.randrange(l_seq)] = rng.choice((15, 0, 3))                             # N and other codes that are no evidence
        out.append(rec(b"q%d" % k + b"x" * (k % 4), r, pos, cig, seq, _quals(rng, l_seq), _flag(rng), rng.choice(MAPQS), tail=bytes(rng.randrange(0, 4))))
    for r, L in enumerate(REF_LEN[:BIG + 1]):
        # three reads that disagree with the first and with the last base of every contig: sites at both ends, neighbours across the boundary
        for end, p in (("first", 0), ("last", L - 1)):
            alt = CODE[(refs[r][p] + 1) % 4]
            for k in range(3):
                n = min(L - p, 20) if end == "first" else 1
                out.append(rec(b"%s%d_%d" % (end.encode(), r, k), r, p, [(n, M)], read_over(refs, r, p, [(n, M)], edits={0: alt}), flag=0x10 * (k & 1)))
        # beyond the end; an insertion in front of the end's base, and one at the end itself, which is dropped
        p = max(0, L - 4)
        out.append(rec(b"beyond%d" % r, r, p, [(12, M)], read_over(refs, r, p, [(12, M)], edits={1: CODE[(refs[r][min(p + 1, L - 1)] + 2) % 4]})))
        out.append(rec(b"d_beyond%d" % r, r, p, [(2, M), (9, D), (4, M)], read_over(refs, r, p, [(2, M), (9, D), (4, M)])))
        for k in range(2):
            out.append(rec(b"ins_end%d_%d" % (r, k), r, p, [(L - p, M), (3, I), (2, S)], read_over(refs, r, p, [(L - p, M)]) + [1, 2, 4, 8, 8]))
            if L > 1:
                out.append(rec(b"ins_last%d_%d" % (r, k), r, p, [(L - p - 1, M), (2, I), (1, M)], read_over(refs, r, p, [(L - p - 1, M)]) + [2, 2, CODE[refs[r][L - 1]]]))
    # ---- every length of the list on the big contig, forward and reverse, with one planted mismatch at the read's last base
    for n in L_SEQS:
        for k in range(2):
            p = 1000 + 7 * n % 900
            out.append(rec(b"len%d_%d" % (n, k), BIG, p, [(n, M)], read_over(refs, BIG, p, [(n, M)], edits={n - 1: CODE[(refs[BIG][p + n - 1] + 1) % 4]}), flag=0x10 * k))
    out.append(rec(b"noseq", BIG, 50, [(30, M)], []))                                        # l_seq 0: takes no part
    out.append(rec(b"cigar_short", QUIET, 60, [(20, M)], read_over(refs, QUIET, 60, [(30, M)], edits={3: CODE[(refs[QUIET][63] + 1) % 4]})))   # query length 20, l_seq 30
    # ---- qualities either side of MIN_BASEQ, and 0xff in front; N at a mismatching position; N inside an insertion
    p = 2000
    alt = CODE[(refs[QUIET][p + 5] + 1) % 4]
    for k, q5 in enumerate((MIN_BASEQ - 1, MIN_BASEQ - 1, MIN_BASEQ, MIN_BASEQ)):
        out.append(rec(b"bq%d" % k, QUIET, p, [(10, M)], read_over(refs, QUIET, p, [(10, M)], edits={5: alt}), [40] * 5 + [q5] + [40] * 4))
    for k in range(2):
        out.append(rec(b"noqual%d" % k, QUIET, p, [(10, M)], read_over(refs, QUIET, p, [(10, M)], edits={6: CODE[(refs[QUIET][p + 6] + 2) % 4]}), [0xff] + [0] * 9))
        out.append(rec(b"n_mism%d" % k, QUIET, p, [(10, M)], read_over(refs, QUIET, p, [(10, M)], edits={7: 15})))
        out.append(rec(b"n_ins%d" % k, QUIET, p, [(4, M), (3, I), (3, M)], read_over(refs, QUIET, p, [(4, M)]) + [1, 15, 2] + read_over(refs, QUIET, p + 4, [(3, M)])))
        out.append(rec(b"acgt_ins%d" % k, QUIET, p, [(4, M), (3, I), (3, M)], read_over(refs, QUIET, p, [(4, M)]) + [1, 8, 2] + read_over(refs, QUIET, p + 4, [(3, M)])))
    # ---- a site under a deletion: three mismatching reads, two that delete the base
    p = 2100
    for k in range(3):
        out.append(rec(b"under%d" % k, QUIET, p - 3, [(10, M)], read_over(refs, QUIET, p - 3, [(10, M)], edits={3: CODE[(refs[QUIET][p] + 1) % 4]}), flag=0x10 * (k & 1)))
    for k in range(2):
        out.append(rec(b"over%d" % k, QUIET, p - 5, [(3, M), (6, D), (4, M)], read_over(refs, QUIET, p - 5, [(3, M), (6, D), (4, M)])))
    # ---- excluded by exactly one bit of 1796; mapq either side of MIN_MAPQ: each pair alone on its site
    for k, (bit, mapq) in enumerate(((0x4, 60), (0x100, 60), (0x200, 60), (0x400, 60), (0, MIN_MAPQ - 1), (0, MIN_MAPQ))):
        p = 2200 + 20 * k
        for j in range(2):
            out.append(rec(b"only%x_%d_%d" % (bit, mapq, j), QUIET, p, [(10, M)], read_over(refs, QUIET, p, [(10, M)], edits={4: CODE[(refs[QUIET][p + 4] + 1) % 4]}), flag=bit, mapq=mapq))
    # ---- alleles seen once, twice and three times, each alone on its site
    for cnt in (1, 2, 3):
        p = 2400 + 20 * cnt
        for j in range(cnt):
            out.append(rec(b"cnt%d_%d" % (cnt, j), QUIET, p, [(10, M)], read_over(refs, QUIET, p, [(10, M)], edits={2: CODE[(refs[QUIET][p + 2] + 3) % 4]}), flag=0x10 * (j & 1)))
    # ---- insertions of 8, 9, 31 and 32 bases with the same first eight; beyond them they differ
    p = 2600
    first8 = [1, 2, 4, 8, 8, 4, 2, 1]
    for n, rest in ((8, []), (8, []), (9, [1]), (9, [4]), (31, [2] * 23), (32, [8] * 24), (32, [1] * 24)):
        cig = [(5, M), (n, I), (5, M)]
        out.append(rec(b"ins%d_%d" % (n, len(out)), QUIET, p, cig, read_over(refs, QUIET, p, [(5, M)]) + first8 + rest + read_over(refs, QUIET, p + 5, [(5, M)])))
    # ---- more than 300 reads on one site of a contig nothing else touches, more than 20 alleles there
    b = refs[STACK_REF][STACK_POS]
    for k in range(330):
        kind = k % 30
        pos = STACK_POS - 10
        if kind < 9:                                                                        # three SNV alleles and the reference
            cig = [(30, M)]
            seq = read_over(refs, STACK_REF, pos, cig, edits={10: CODE[(b + kind % 4) % 4]})
        elif kind < 20:                                                                     # deletions of 1 .. 11 bases that begin at the site
            cig = [(10, M), (kind - 8, D), (10, M)]
            seq = read_over(refs, STACK_REF, pos, cig)
        else:                                                                               # insertions in front of the site: ten alleles
            cig = [(10, M), (2, I), (10, M)]
            seq = read_over(refs, STACK_REF, pos, [(10, M)]) + [CODE[(kind - 20) % 4], CODE[(kind - 20) // 4]] + read_over(refs, STACK_REF, STACK_POS, [(10, M)])
        out.append(rec(b"st%d" % k, STACK_REF, pos, cig, seq, flag=0x10 * (k // 30 & 1)))
    rng.shuffle(out)
    return make_case(out, refs)


def make_case(records, refs=None, shift=0):
    """shift: bytes in front of the first record (the offsets do not start at 0)."""
    refs = reference() if refs is None else refs
    off = np.zeros(len(records) + 1, dtype=np.int64)
    if records:
        off[1:] = np.cumsum([len(r) for r in records])
    return dict(records=records, refs=refs, ref_len=[len(s) for s in refs], pac=ref.pack_reference(refs), buf=b"\x5a" * shift + b"".join(records), off=off + shift)


def ordinary(n_bytes, seed=1):
    """At least n_bytes of ordinary records on the big contig (long tails, so that few of them are many bytes)."""
    rng, refs, out, got = random.Random(seed), reference(), [], 0
    while got < n_bytes:
        p, n = rng.randrange(0, 4800), rng.randrange(30, 151)
        out.append(rec(b"o%d" % len(out), BIG, p, [(n, M)], read_over(refs, BIG, p, [(n, M)], rng, 0.02), flag=16 * rng.randrange(2), tail=bytes(rng.randrange(150, 260))))
        got += len(out[-1])
    return out


def bad_records(n_ref=len(REF_LEN)):
    """name -> (record, the rule refuses it): the table of tests/qc_cases.py, where the three records whose l_seq does not fit are now
    refused, and a record whose bases fit but whose qualities do not."""
    good = rec(b"bad", BIG, 0, [(10, M)], [1] * 10)
    patched = lambda src, at, fmt, v: (lambda b: (struct.pack_into(fmt, b, at, v), bytes(b))[1])(bytearray(src))
    raw = lambda n: struct.pack("<iiiBBHHH", n - 4, 0, 0, 1, 0, 0, 0, 0) + bytes(n - 20)
    cut = good[:-3]
    return {"block_size below 32": (raw(20), True), "a read of 35 bytes": (raw(35), True), "block_size one too large": (patched(good, 0, "<i", len(good) - 3), True),
            "block_size one too small": (patched(good, 0, "<i", len(good) - 5), True), "bytes after the last record": (good + b"\0" * 10, True),
            "n_cigar_op beyond the record": (patched(good, 16, "<H", 60000), True), "l_read_name beyond the record": (patched(good, 12, "<B", 255), True),
            "l_seq beyond the record": (patched(good, 20, "<i", 1 << 30), True), "l_seq negative": (patched(good, 20, "<i", -1), True),
            "l_seq one too large": (patched(good, 20, "<i", 11), True), "l_seq = 2^31 - 1": (patched(good, 20, "<i", 0x7fffffff), True),
            "the last three qualities missing": (struct.pack("<i", len(cut) - 4) + cut[4:], True),
            "refID = n_ref": (rec(b"bad", n_ref, 0, [(1, M)], [1]), True), "refID = 2^31 - 1": (rec(b"bad", 0x7fffffff, 0), True),
            "pos < 0 on a reference": (rec(b"bad", 0, -1, [(1, M)], [1]), True), "pos < 0 without a reference": (rec(b"bad", -1, -5), False)}


def assert_families(case):
    recs, lens, refs, pac = case["records"], case["ref_len"], case["refs"], case["pac"]
    assert 2000 <= len(recs) <= 6000
    starts = [sum(lens[:r]) for r in range(len(lens))]
    assert {1, 3, 4, 5, 63, 64, 65, 255, 256, 257} <= set(lens) and max(lens) >= 3000 and {s % 4 for s in starts} == {0, 1, 2, 3}
    f = [ref.fields(r, len(lens)) for r in recs]
    opt1, opt2 = ref.resolve(0, 0, -1, 1), ref.resolve()
    part = [x for x in f if ref.takes_part(x, opt1)]
    p1, p2 = ref.pileup(recs, lens, pac, (0, 0, -1, 1)), ref.pileup(recs, lens, pac)
    at2 = {(s["ref"], s["pos"]): s for s in p2["sites"]}
    at1 = {(s["ref"], s["pos"]): s for s in p1["sites"]}
    for r, L in enumerate(lens[:BIG + 1]):                            # both ends of every contig; the boundary keeps its two sites apart
        assert (r, 0) in at2 and (r, L - 1) in at2, r
    assert min(p2["n_obs"]) > 50, p2["n_obs"]
    # clipped at the end; the insertion at the end is dropped, the one in front of the last base is not
    ref_end = lambda x: x["pos"] + sum(n for n, op in x["cigar"] if op in (M, D, N, EQ, X))
    assert sum(1 for x in part if ref_end(x) > lens[x["ref"]]) > 20
    dropped = [x for x in part if any(op == I for _, op in x["cigar"]) and not any(k == ref.INS for _, k, _, _ in ref.observe(x, lens[x["ref"]], starts[x["ref"]], pac, opt1)[2])
               and all(c in ref.CODE2 for c in x["seq"])]
    assert len(dropped) >= 10
    assert any(a["kind"] == ref.INS for r in range(BIG + 1) if lens[r] > 1 for a in at2[(r, lens[r] - 1)]["alleles"])
    assert {x["l_seq"] for x in f} >= {0, *L_SEQS} and {x["l_seq"] for x in part} >= set(L_SEQS)
    seen, o = set(), 0
    for r in recs:
        seen.add(o % 4)
        o += len(r)
    assert seen == {0, 1, 2, 3}                                      # records at every alignment
    quals = {q for x in part for q in x["qual"]}
    assert {MIN_BASEQ - 1, MIN_BASEQ} <= quals and sum(1 for x in part if x["qual"][0] == 0xff and min(x["qual"]) < MIN_BASEQ) >= 2
    pq = ref.pileup(recs, lens, pac, (0, MIN_BASEQ, -1, 2))
    bq = lambda p: {(s["ref"], s["pos"]): s for s in p["sites"]}
    site = (QUIET, 2005)
    assert sum(a["fwd"] + a["rev"] for a in at2[site]["alleles"] if a["kind"] == ref.SNV) == sum(a["fwd"] + a["rev"] for a in bq(pq)[site]["alleles"] if a["kind"] == ref.SNV) + 2
    assert (QUIET, 2006) in bq(pq)                                     # 0xff in front: quality 0 passes
    assert any(15 in x["seq"] for x in part) and (QUIET, 2007) not in at1          # N where the others agree with the reference: no site at all
    ins = [a for a in at1[(QUIET, 2004)]["alleles"] if a["kind"] == ref.INS]     # A N C is no evidence, A T C is
    assert len(ins) == 1 and (ins[0]["len"], ins[0]["bases"], ins[0]["fwd"]) == (3, 0 | 3 << 2 | 1 << 4, 2), ins
    assert {op for x in f for _, op in x["cigar"]} == set(range(9))
    s = at2[(QUIET, 2100)]                                             # three mismatches, two deletions over them
    assert s["n_cov"] >= 5 and sum(a["fwd"] + a["rev"] for a in s["alleles"]) + sum(s["n_ref"]) <= s["n_cov"] - 2
    assert any(sum(n for n, op in x["cigar"] if op in ref.QUERY_OPS) != x["l_seq"] and x["l_seq"] > 0 for x in f) and (QUIET, 63) not in at1
    for k, bit in enumerate((0x4, 0x100, 0x200, 0x400)):
        assert (QUIET, 2204 + 20 * k) not in at2 and (QUIET, 2204 + 20 * k) in bq(ref.pileup(recs, lens, pac, (0, 0, 1796 & ~bit, 2))), hex(bit)
    pm = bq(ref.pileup(recs, lens, pac, (MIN_MAPQ, 0, -1, 2)))
    assert (QUIET, 2284) in at2 and (QUIET, 2284) not in pm and (QUIET, 2304) in pm
    for cnt in (1, 2, 3):                                            # kept exactly from min_alt = its count downwards
        site = (QUIET, 2402 + 20 * cnt)
        for min_alt in (1, 2, 3):
            assert (site in bq(ref.pileup(recs, lens, pac, (0, 0, -1, min_alt)))) == (cnt >= min_alt), (cnt, min_alt)
    assert any(a["fwd"] and a["rev"] for s in p2["sites"] for a in s["alleles"])
    ins = {(a["len"], a["bases"]): a["fwd"] + a["rev"] for a in at2[(QUIET, 2605)]["alleles"] if a["kind"] == ref.INS}
    assert {k[0]: v for k, v in ins.items()} == {8: 2, 9: 2, 31: 3} and len({k[1] for k in ins}) == 1, ins
    s = at2[(STACK_REF, STACK_POS)]
    assert s["n_cov"] > 300 and len(s["alleles"]) > 20 and {a["kind"] for a in s["alleles"]} == {0, 1, 2}, (s["n_cov"], len(s["alleles"]))
    return p2
