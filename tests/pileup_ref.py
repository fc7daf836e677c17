"""The judge of the pileup (BPU\\1): plain Python over the records' bytes, the contig lengths and the packed reference, written from the rule in
include/bwahip.h ("Pileup of candidate variant sites") and not from the C++.  build() gives the canonical bytes, parse() reads a file back
into a dict, fields() what the rule reads of one record, observe() what one record contributes."""
import struct
from collections import Counter

M, I, D, N, S, H, P, EQ, X = range(9)
MATCH_OPS, QUERY_OPS = (M, EQ, X), (M, I, S, EQ, X)
DEFAULT_EXCLUDE = 0x4 | 0x100 | 0x200 | 0x400
SNV, DEL, INS = 0, 1, 2
CODE2 = {1: 0, 2: 1, 4: 2, 8: 3}                                    # the BAM codes of A C G T
DEL_CAP = 2 ** 21 - 1


class BadRecord(ValueError):
    pass


def resolve(min_mapq=0, min_baseq=0, exclude_flags=-1, min_alt=0):
    if not 0 <= min_mapq <= 255 or not 0 <= min_baseq <= 93 or exclude_flags > 0xffff or not 0 <= min_alt <= 0xffff:
        raise ValueError("options out of range")
    return (min_mapq, min_baseq, DEFAULT_EXCLUDE if exclude_flags < 0 else exclude_flags, min_alt or 2)


def pack_reference(seqs):
    """The contigs' bases (lists of 0..3) one after the other in .pac's layout: base i in byte i >> 2 at shift (~i & 3) << 1."""
    flat = [b for s in seqs for b in s]
    out = bytearray((len(flat) + 3) // 4)
    for i, b in enumerate(flat):
        out[i >> 2] |= b << ((~i & 3) << 1)
    return bytes(out)


def ref_base(pac, g):
    return pac[g >> 2] >> ((~g & 3) << 1) & 3


def fields(rec, n_ref):
    """dict of what the rule reads of one record; BadRecord for what it refuses."""
    if len(rec) < 36:
        raise BadRecord("shorter than 36 bytes")
    block_size, ref, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiiBBHHHi", rec, 0)
    if block_size + 4 != len(rec):
        raise BadRecord("block_size")
    if 36 + l_name + 4 * n_cigar > len(rec):
        raise BadRecord("name and CIGAR beyond the record")
    if ref >= n_ref or (ref >= 0 and pos < 0):
        raise BadRecord("refID or pos")
    if l_seq < 0:
        raise BadRecord("l_seq < 0")
    at = 36 + l_name + 4 * n_cigar
    if at + (l_seq + 1) // 2 + l_seq > len(rec):
        raise BadRecord("bases and qualities beyond the record")
    cigar = [(w >> 4, w & 15) for w in struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_name)]
    packed = rec[at:at + (l_seq + 1) // 2]
    seq = [packed[q >> 1] >> 4 if q % 2 == 0 else packed[q >> 1] & 15 for q in range(l_seq)]
    qual = rec[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq]
    return dict(ref=ref, pos=pos, mapq=mapq, flag=flag, l_seq=l_seq, cigar=cigar, seq=seq, qual=qual)


def takes_part(f, opt):
    return (f["ref"] >= 0 and not f["flag"] & opt[2] and f["mapq"] >= opt[0] and f["l_seq"] > 0 and
            sum(n for n, op in f["cigar"] if op in QUERY_OPS) == f["l_seq"])


def observe(f, length, g0, pac, opt):
    """What a record that takes part contributes on its contig of `length` bases that begins at base g0 of the packed reference:
    (covered positions, positions whose base passes and equals the reference, observations as (p, kind, len, bases))."""
    cover, match, obs = [], [], []
    all_pass = f["qual"][0] == 0xff
    p, q = f["pos"], 0
    for n, op in f["cigar"]:
        if op in MATCH_OPS:
            for j in range(n):
                if not 0 <= p + j < length:
                    continue
                cover.append(p + j)
                code = f["seq"][q + j]
                if code in CODE2 and (all_pass or f["qual"][q + j] >= opt[1]):
                    if CODE2[code] == ref_base(pac, g0 + p + j):
                        match.append(p + j)
                    else:
                        obs.append((p + j, SNV, 1, CODE2[code]))
            p += n
            q += n
        elif op == D:
            if n and 0 <= p < length:
                obs.append((p, DEL, min(n, DEL_CAP), 0))
            cover += [x for x in range(p, p + n) if 0 <= x < length]
            p += n
        elif op == I:
            ins = f["seq"][q:q + n]
            if n and 0 <= p < length and all(c in CODE2 for c in ins):
                obs.append((p, INS, min(n, 31), sum(CODE2[c] << (2 * k) for k, c in enumerate(ins[:8]))))
            q += n
        elif op == N:
            p += n
        elif op == S:
            q += n
    return cover, match, obs


def pileup(records, ref_len, pac, opt=()):
    opt = resolve(*opt)
    n_ref = len(ref_len)
    if sum(ref_len) >= 2 ** 40:
        raise ValueError("the contigs are too long")
    off = [sum(ref_len[:r]) for r in range(n_ref)]
    cov, hit, alleles, n_obs = Counter(), Counter(), {}, [0, 0, 0]
    for rec in records:
        f = fields(rec, n_ref)
        if not takes_part(f, opt):
            continue
        r, strand = f["ref"], 1 if f["flag"] & 0x10 else 0
        cover, match, obs = observe(f, ref_len[r], off[r], pac, opt)
        for p in cover:
            cov[(r, p)] += 1
        for p in match:
            hit[(r, p, strand)] += 1
        for p, kind, ln, bases in obs:
            n_obs[kind] += 1
            alleles.setdefault((r, p, kind, ln, bases), [0, 0])[strand] += 1
    kept = sorted(k for k, (fwd, rev) in alleles.items() if fwd + rev >= opt[3])
    sites = []
    for k in kept:
        r, p = k[:2]
        if not sites or (sites[-1]["ref"], sites[-1]["pos"]) != (r, p):
            sites.append(dict(ref=r, pos=p, ref_base=ref_base(pac, off[r] + p), n_cov=cov[(r, p)], n_ref=(hit[(r, p, 0)], hit[(r, p, 1)]), alleles=[]))
        sites[-1]["alleles"].append(dict(kind=k[2], len=k[3], bases=k[4], fwd=alleles[k][0], rev=alleles[k][1]))
    return dict(n_ref=n_ref, opt=opt, n_obs=n_obs, sites=sites)


def serialise(s):
    al = [a for x in s["sites"] for a in x["alleles"]]
    out = [b"BPU\1", struct.pack("<iiiii", s["n_ref"], *s["opt"]), struct.pack("<QQ3Q", len(s["sites"]), len(al), *s["n_obs"])]
    out += [struct.pack("<iiIIIII", x["ref"], x["pos"], x["ref_base"], len(x["alleles"]), x["n_cov"], *x["n_ref"]) for x in s["sites"]]
    out += [struct.pack("<IIIII", a["kind"], a["len"], a["bases"], a["fwd"], a["rev"]) for a in al]
    return b"".join(out)


def build(records, ref_len, pac, opt=()):
    """The canonical bytes for these records (any order), contig lengths and packed reference."""
    return serialise(pileup(records, ref_len, pac, opt))


def parse(data):
    """A BPU\\1 file as the dict pileup() makes; ValueError when it is not one or its length does not fit."""
    if data[:4] != b"BPU\1" or len(data) < 64:
        raise ValueError("not a BPU file")
    n_ref, *opt = struct.unpack_from("<iiiii", data, 4)
    n_sites, n_alleles, *n_obs = struct.unpack_from("<QQ3Q", data, 24)
    if len(data) != 64 + 28 * n_sites + 20 * n_alleles:
        raise ValueError("length")
    sites, at = [], 64 + 28 * n_sites
    for k in range(n_sites):
        r, p, rb, na, n_cov, nf, nr = struct.unpack_from("<iiIIIII", data, 64 + 28 * k)
        al = [dict(zip(("kind", "len", "bases", "fwd", "rev"), struct.unpack_from("<IIIII", data, at + 20 * j))) for j in range(na)]
        at += 20 * na
        sites.append(dict(ref=r, pos=p, ref_base=rb, n_cov=n_cov, n_ref=(nf, nr), alleles=al))
    if at != len(data):
        raise ValueError("the sites' allele counts")
    return dict(n_ref=n_ref, opt=tuple(opt), n_obs=n_obs, sites=sites)


def first_difference(got, want):
    """A few words on where two files part, for assertion messages."""
    if got == want:
        return "equal"
    try:
        a, b = parse(got), parse(want)
    except (ValueError, struct.error) as e:
        return f"unparsable ({e}); lengths {len(got)} / {len(want)}"
    for k in ("n_ref", "opt", "n_obs"):
        if a[k] != b[k]:
            return f"{k}: {a[k]} != {b[k]}"
    for x, y in zip(a["sites"], b["sites"]):
        if x != y:
            return f"site {x} != {y}"
    return f"{len(a['sites'])} sites != {len(b['sites'])}"
