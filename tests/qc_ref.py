"""The judge of the QC summary (BQC\\1): plain Python over the records' bytes and the contig lengths, written from the rule in
include/bwahip.h ("Alignment QC summary and depth of coverage") and not from the C++.  build() gives the canonical bytes, parse() reads a
summary back into a dict, fields() what one record counts for."""
import struct

M, I, D, N, S, H, P, EQ, X = range(9)
COVER_OPS, REF_OPS = (M, D, EQ, X), (M, D, N, EQ, X)
DEFAULT_EXCLUDE = 0x4 | 0x100 | 0x200 | 0x400
N_CAT = 16


class BadRecord(ValueError):
    pass


def resolve(window_shift=0, exclude_flags=-1, min_mapq=0):
    if (window_shift != 0 and not 4 <= window_shift <= 29) or exclude_flags > 0xffff or not 0 <= min_mapq <= 255:
        raise ValueError("options out of range")
    return (window_shift or 14, DEFAULT_EXCLUDE if exclude_flags < 0 else exclude_flags, min_mapq)


def fields(rec, n_ref):
    """dict of what the rule reads of one record; BadRecord for what it refuses."""
    if len(rec) < 36:
        raise BadRecord("shorter than 36 bytes")
    block_size, ref, pos, l_name, mapq, _bin, n_cigar, flag, _l_seq, next_ref, _next_pos, tlen = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    if block_size + 4 != len(rec):
        raise BadRecord("block_size")
    if 36 + l_name + 4 * n_cigar > len(rec):
        raise BadRecord("name and CIGAR beyond the record")
    if ref >= n_ref or (ref >= 0 and pos < 0):
        raise BadRecord("refID or pos")
    cigar = [(w >> 4, w & 15) for w in struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_name)]
    return dict(ref=ref, pos=pos, mapq=mapq, flag=flag, next_ref=next_ref, tlen=tlen, cigar=cigar)


def categories(f):
    """The indices k of count[q][k] the record adds one to."""
    flag = f["flag"]
    prim, mapped = not flag & 0x900, not flag & 0x4
    out = [0]
    if prim:
        out.append(1)
    if flag & 0x100:
        out.append(2)
    if flag & 0x800 and not flag & 0x100:
        out.append(3)
    if flag & 0x400:
        out.append(4)
        if prim:
            out.append(5)
    if mapped:
        out.append(6)
        if prim:
            out.append(7)
    if prim and flag & 0x1:
        out.append(8)
        if flag & 0x40:
            out.append(9)
        if flag & 0x80:
            out.append(10)
        if flag & 0x2 and mapped:
            out.append(11)
        if mapped and not flag & 0x8:
            out.append(12)
            if f["next_ref"] != f["ref"]:
                out.append(14)
                if f["mapq"] >= 5:
                    out.append(15)
        if mapped and flag & 0x8:
            out.append(13)
    return out


def intervals(f, length):
    """The record's covering operations as [a, b) clipped to the contig, one per operation."""
    out, p = [], f["pos"]
    for n, op in f["cigar"]:
        if op in COVER_OPS:
            a, b = max(p, 0), min(p + n, length)
            if a < b:
                out.append((a, b))
        if op in REF_OPS:
            p += n
    return out


def takes_part(f, opt):
    return f["ref"] >= 0 and not f["flag"] & opt[1] and f["mapq"] >= opt[2]


def depths(records, ref_len, opt=()):
    """Per reference the list of depths, base by base."""
    opt = resolve(*opt)
    diff = [[0] * (n + 1) for n in ref_len]
    for rec in records:
        f = fields(rec, len(ref_len))
        if takes_part(f, opt):
            for a, b in intervals(f, ref_len[f["ref"]]):
                diff[f["ref"]][a] += 1
                diff[f["ref"]][b] -= 1
    out = []
    for d in diff:
        run, dep = 0, []
        for x in d[:-1]:
            run += x
            dep.append(run)
        out.append(dep)
    return out


def summary(records, ref_len, opt=()):
    ws, excl, min_mapq = o = resolve(*opt)
    n_ref = len(ref_len)
    s = dict(n_ref=n_ref, opt=o, n_no_coor=0, count=[[0] * N_CAT for _ in range(2)], mapq_hist=[0] * 256, isize_hist=[0] * 1025, depth_hist=[0] * 256,
             refs=[dict(len=n, mapped=0, placed_unmapped=0) for n in ref_len])
    for rec in records:
        f = fields(rec, n_ref)
        flag = f["flag"]
        for k in categories(f):
            s["count"][1 if flag & 0x200 else 0][k] += 1
        if f["ref"] < 0:
            s["n_no_coor"] += 1
        else:
            s["refs"][f["ref"]]["placed_unmapped" if flag & 0x4 else "mapped"] += 1
        if not flag & 0x900 and not flag & 0x4:
            s["mapq_hist"][f["mapq"]] += 1
        if not flag & 0x900 and flag & 0x1 and flag & 0x2 and not flag & 0x4 and not flag & 0x8 and f["tlen"] > 0:
            s["isize_hist"][min(f["tlen"], 1024)] += 1
    for r, dep in zip(s["refs"], depths(records, ref_len, opt)):
        r["covered"] = sum(1 for d in dep if d >= 1)
        r["depth_sum"] = sum(dep)
        r["windows"] = [sum(dep[w:w + (1 << ws)]) for w in range(0, len(dep), 1 << ws)]
        for d in dep:
            s["depth_hist"][min(d, 255)] += 1
    return s


def serialise(s):
    out = [b"BQC\1", struct.pack("<iiii", s["n_ref"], *s["opt"]), struct.pack("<Q", s["n_no_coor"])]
    out += [struct.pack("<16Q", *row) for row in s["count"]]
    out += [struct.pack("<256Q", *s["mapq_hist"]), struct.pack("<1025Q", *s["isize_hist"]), struct.pack("<256Q", *s["depth_hist"])]
    out += [struct.pack("<6Q", r["len"], r["mapped"], r["placed_unmapped"], r["covered"], r["depth_sum"], len(r["windows"])) for r in s["refs"]]
    out += [struct.pack("<%dQ" % len(r["windows"]), *r["windows"]) for r in s["refs"]]
    return b"".join(out)


def build(records, ref_len, opt=()):
    """The canonical bytes for these records (any order) and contig lengths."""
    return serialise(summary(records, ref_len, opt))


def parse(data):
    """A BQC\\1 file as the dict summary() makes; ValueError when it is not one or its length does not fit."""
    if data[:4] != b"BQC\1" or len(data) < 28:
        raise ValueError("not a BQC file")
    n_ref, ws, excl, min_mapq = struct.unpack_from("<iiii", data, 4)
    at = 20

    def take(n):
        nonlocal at
        v = list(struct.unpack_from("<%dQ" % n, data, at))
        at += 8 * n
        return v
    s = dict(n_ref=n_ref, opt=(ws, excl, min_mapq), n_no_coor=take(1)[0], count=[take(N_CAT), take(N_CAT)], mapq_hist=take(256), isize_hist=take(1025), depth_hist=take(256), refs=[])
    n_windows = []
    for _ in range(n_ref):
        ln, mapped, unm, covered, depth_sum, nw = take(6)
        s["refs"].append(dict(len=ln, mapped=mapped, placed_unmapped=unm, covered=covered, depth_sum=depth_sum))
        n_windows.append(nw)
    for r, nw in zip(s["refs"], n_windows):
        if nw != (r["len"] + (1 << ws) - 1) >> ws:
            raise ValueError("window count")
        r["windows"] = take(nw)
    if at != len(data):
        raise ValueError("length")
    return s


def first_difference(got, want):
    """A few words on where two summaries part, for assertion messages."""
    if got == want:
        return "equal"
    try:
        a, b = parse(got), parse(want)
    except (ValueError, struct.error) as e:
        return f"unparsable ({e}); lengths {len(got)} / {len(want)}"
    for k in ("n_ref", "opt", "n_no_coor", "count"):
        if a[k] != b[k]:
            return f"{k}: {a[k]} != {b[k]}"
    for k in ("mapq_hist", "isize_hist", "depth_hist"):
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            if x != y:
                return f"{k}[{i}]: {x} != {y}"
    for r, (x, y) in enumerate(zip(a["refs"], b["refs"])):
        for k in ("len", "mapped", "placed_unmapped", "covered", "depth_sum"):
            if x[k] != y[k]:
                return f"reference {r} {k}: {x[k]} != {y[k]}"
        for w, (p, q) in enumerate(zip(x["windows"], y["windows"])):
            if p != q:
                return f"reference {r} window {w}: {p} != {q}"
    return "differ"
