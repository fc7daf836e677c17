"""The judge of duplicate marking (include/bwahip.h, "Duplicate marking"): plain Python over BAM record bytes.  It groups records into
templates by read name (the tests use unique names; the two reads of a pair by 0x40 / 0x80), computes kinds, end words and scores from the
bytes, applies the rule, and returns the marked records and the per-class counts.  Nothing here calls the library under test."""
import struct

M64 = (1 << 64) - 1
REF_OPS = (0, 2, 3, 7, 8)                        # M D N = X
CLIPS = (4, 5)                                   # S H


def parse(rec):
    ref, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    o = 36
    name = rec[o:o + l_name]
    o += l_name
    cigar = [(v >> 4, v & 15) for v in struct.unpack_from(f"<{n_cig}I", rec, o)]
    o += 4 * n_cig + (l_seq + 1) // 2
    return dict(ref=ref, pos=pos, flag=flag, name=name.split(b"\0")[0], cigar=cigar, qual=rec[o:o + l_seq])


def wrap32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


def end_word(ref, u5, rev):
    return ((ref & M64) << 33 | (u5 + (1 << 31)) << 1 | int(bool(rev))) & M64


def u5_of(p):
    """The unclipped 5' position of a parsed, mapped record (as int32)."""
    ops = p["cigar"]
    lead = trail = 0
    for n, op in ops:
        if op not in CLIPS:
            break
        lead += n
    for n, op in reversed(ops):
        if op not in CLIPS:
            break
        trail += n
    rlen = sum(n for n, op in ops if op in REF_OPS)
    return wrap32(p["pos"] + max(rlen, 1) - 1 + trail if p["flag"] & 0x10 else p["pos"] - lead)


def score_of(p):
    q = p["qual"]
    if q and q[0] == 0xff:
        return 0
    return sum(b for b in q if b >= 15)


def describe_reads(reads):
    """reads: the record lists of a template's one or two reads -> (end0, end1, score, kind)."""
    ends, score = [], 0
    for recs in reads:
        prim = [p for p in map(parse, recs) if not p["flag"] & 0x900]
        if prim and not prim[0]["flag"] & 0x4:
            p = prim[0]
            ends.append(end_word(p["ref"], u5_of(p), p["flag"] & 0x10))
            score += score_of(p)
    if not ends:
        return (0, 0, 0, 0)
    ends.sort()
    return (ends[0], ends[1] if len(ends) == 2 else 0, score & 0xffffffff, len(ends))


def decide(descs):
    """descs in input order -> (dup, cls): dup[i] 0 / 1; cls[i] None for a template that is alone with its signature, else one of
    'pair' / 'frag_pair' / 'frag_frag' for duplicates and 'kept_pair' / 'kept_frag' for the survivor of a cluster with duplicates."""
    n = len(descs)
    dup, cls = [0] * n, [None] * n
    best = lambda ii: min(ii, key=lambda i: (-descs[i][2], i))
    pairs, frags, pair_ends = {}, {}, set()
    for i, (e0, e1, _, kind) in enumerate(descs):
        if kind == 2:
            pairs.setdefault((e0, e1), []).append(i)
            pair_ends.update((e0, e1))
    for i, (e0, _, _, kind) in enumerate(descs):
        if kind == 1:
            if e0 in pair_ends:
                dup[i], cls[i] = 1, "frag_pair"
            else:
                frags.setdefault(e0, []).append(i)
    for groups, d, k in ((pairs, "pair", "kept_pair"), (frags, "frag_frag", "kept_frag")):
        for ii in groups.values():
            b = best(ii)
            for i in ii:
                if i != b:
                    dup[i], cls[i] = 1, d
                elif len(ii) > 1:
                    cls[i] = k
    return dup, cls


def templates_of(records, names, paired):
    """records in any order, names = the templates' names in input order -> per template the record lists of its reads."""
    idx = {n: i for i, n in enumerate(names)}
    assert len(idx) == len(names), "template names must be unique"
    out = [([], []) if paired else ([],) for _ in names]
    for r in records:
        p = parse(r)
        out[idx[p["name"]]][1 if paired and p["flag"] & 0x80 else 0].append(r)
    return out


def set_dup(rec):
    flag, = struct.unpack_from("<H", rec, 18)
    return rec if flag & 0x4 else rec[:18] + struct.pack("<H", flag | 0x400) + rec[20:]


def mark(records, names, paired):
    """records: any order (the order is kept); names: the templates' names in input order.  Returns dict(records = the marked records,
    descs, dup, cls, stats = (templates per kind, duplicate templates per kind, records marked), classes = templates per class)."""
    tm = templates_of(records, names, paired)
    descs = [describe_reads(t) for t in tm]
    dup, cls = decide(descs)
    idx = {n: i for i, n in enumerate(names)}
    out, n_marked = [], 0
    for r in records:
        m = set_dup(r) if dup[idx[parse(r)["name"]]] else r
        n_marked += m != r
        out.append(m)
    n_kind = [sum(1 for d in descs if d[3] == k) for k in range(3)]
    n_dup = [sum(1 for d, x in zip(descs, dup) if d[3] == k and x) for k in range(3)]
    classes = {k: sum(1 for c in cls if c == k) for k in ("pair", "frag_pair", "frag_frag", "kept_pair", "kept_frag")}
    return dict(records=out, descs=descs, dup=dup, cls=cls, stats=(n_kind, n_dup, n_marked), classes=classes)
