"""The BAI index (SAM specification 5.2, reg2bin / reg2bins of 5.3) in the canonical form of include/bwahip.h, written from the
specification and that definition -- the judge of the index tests.  Pure Python; nothing here calls the library under test.

(a) build(records, member_offsets, n_ref): the canonical bytes; from_file(bam_bytes): the same from a finished file.
(b) parse(bai) and query(bai, ref, beg, end): a reader -- the chunks a region needs, by reg2bins and the linear index.  check_semantics
    judges any index of a set of records, whatever its canonical form: every record that overlaps a region lies inside a returned chunk,
    every chunk begins and ends on a record boundary of the file."""
import struct

import numpy as np

import bam_ref
import bgzf_ref

BLOCK = 65280
META_BIN = 37450
MAX_END = 1 << 29
LEVEL_FIRST = (0, 1, 9, 73, 585, 4681)          # the first bin of each of the six levels


class Refused(ValueError):
    """build() refuses what the library must refuse; args[0] is 'EINVAL' or 'ECAPACITY'."""


def level_of(b):
    return max(l for l, first in enumerate(LEVEL_FIRST) if b >= first)


def reg2bins(beg, end):
    """Section 5.3: every bin that may hold a record overlapping [beg, end)."""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def fields(rec, n_ref):
    """(refID, pos, e, bin, unmapped) of one record, every read bounded by the record's length."""
    if len(rec) < 36 or struct.unpack_from("<i", rec, 0)[0] + 4 != len(rec):
        raise Refused("EINVAL")
    ref, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    if 36 + l_name + 4 * n_cig > len(rec) or ref >= n_ref or (ref >= 0 and pos < 0):
        raise Refused("EINVAL")
    if ref < 0:
        return ref, pos, 0, 0, bool(flag & 4)
    rlen = sum(w >> 4 for w in struct.unpack_from(f"<{n_cig}I", rec, 36 + l_name) if w & 15 in (0, 2, 3, 7, 8))
    e = pos + rlen if rlen > 0 and not flag & 4 else pos + 1
    return ref, pos, e, bam_ref.reg2bin(pos, e), bool(flag & 4)


def voffsets(records, member_offsets):
    """V(u_0) .. V(u_n): the virtual offsets of the records' boundaries."""
    u, total = [0], sum(map(len, records))
    for r in records:
        u.append(u[-1] + len(r))
    n_blocks = (total + BLOCK - 1) // BLOCK
    assert len(member_offsets) == n_blocks + 1, f"{len(member_offsets)} member offsets for {n_blocks} blocks"
    return [member_offsets[x // BLOCK] << 16 | x % BLOCK if x < total else member_offsets[n_blocks] << 16 for x in u]


def build(records, member_offsets, n_ref):
    """records in file order; member_offsets: the file offsets c_0 .. c_B of the members of the record stream (c_B: where the EOF block goes)."""
    v = voffsets(records, member_offsets)
    prev = None
    f = []
    for rec in records:                                       # the first offending record decides: malformed, then out of order, then too far
        x = fields(rec, n_ref)
        key = (x[0] & 0xffffffff, x[1] if x[0] >= 0 else 0)
        if prev is not None and key < prev:
            raise Refused("EINVAL")
        if x[2] > MAX_END:
            raise Refused("ECAPACITY")
        prev = key
        f.append(x)
    refs = [dict(bins={}, lin={}, first=None, last=None, mapped=0, unmapped=0) for _ in range(n_ref)]
    n_no_coor, run = 0, None                                  # run: [ref, bin, begin, end] of the chunk that is open
    runs = []
    for i, (ref, pos, e, b, unm) in enumerate(f):
        if ref < 0:
            n_no_coor += 1
            run = None
            continue
        if run is not None and run[0] == ref and run[1] == b:
            run[3] = v[i + 1]
        else:
            run = [ref, b, v[i], v[i + 1]]
            runs.append(run)
        R = refs[ref]
        if R["first"] is None:
            R["first"] = v[i]
        R["last"] = v[i + 1]
        R["unmapped" if unm else "mapped"] += 1
        for w in range(pos >> 14, ((e - 1) >> 14) + 1):
            R["lin"][w] = min(R["lin"].get(w, v[i]), v[i])
    for ref, b, beg, end in runs:                              # file order within a bin; joined when it begins in the member the predecessor ends in
        chunks = refs[ref]["bins"].setdefault(b, [])
        if chunks and beg >> 16 <= chunks[-1][1] >> 16:
            chunks[-1][1] = end
        else:
            chunks.append([beg, end])
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for R in refs:
        if R["first"] is None:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(R["bins"]) + 1))
        for b in sorted(R["bins"]):
            out.append(struct.pack("<Ii", b, len(R["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in R["bins"][b]))
        out.append(struct.pack("<IiQQQQ", META_BIN, 2, R["first"], R["last"], R["mapped"], R["unmapped"]))
        n_intv = max(R["lin"]) + 1
        lin, right = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            right = R["lin"].get(w, right)
            lin[w] = right
        out.append(struct.pack(f"<i{n_intv}Q", n_intv, *lin))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def split_file(bam_bytes):
    """(n_ref, records, member_offsets, header length in the file) of a BAM file: header in members of its own, records, EOF block."""
    members = bgzf_ref.parse(bam_bytes)
    assert members and members[-1]["data"] == b"" and bam_bytes.endswith(bgzf_ref.EOF_BLOCK), "no end-of-file block"
    data = b"".join(m["data"] for m in members)
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        o += 4 + l_name + 4
    at = fo = k = 0
    while at < o:                                              # the header's members
        at += len(members[k]["data"])
        fo += members[k]["size"]
        k += 1
    assert at == o, "the header does not end with a member"
    offs = [fo]
    for m in members[k:-1]:
        assert len(m["data"]) == BLOCK or m is members[-2], "a member of the records that is not 65 280 bytes of input"
        offs.append(offs[-1] + m["size"])
    assert offs[-1] == len(bam_bytes) - len(bgzf_ref.EOF_BLOCK)
    return n_ref, bam_ref.split_records(data[o:]), offs, fo


def from_file(bam_bytes):
    n_ref, records, offs, _ = split_file(bam_bytes)
    return build(records, offs, n_ref)


# ---------------------------------------------------------------------------------------------------------------- (b) a reader
def parse(bai):
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", bai, 4)
    o, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, o)
        o += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", bai, o + 16 * k) for k in range(n_chunk)]
            o += 16 * n_chunk
            assert b not in bins and n_chunk > 0
            if b == META_BIN:
                assert n_chunk == 2 and meta is None
                meta = chunks
            else:
                assert b < META_BIN - 1 and all(x < y for x, y in chunks)
                bins[b] = chunks
        n_intv, = struct.unpack_from("<i", bai, o)
        o += 4
        lin = list(struct.unpack_from(f"<{n_intv}Q", bai, o))
        o += 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, lin=lin))
    n_no_coor = None
    if o < len(bai):
        n_no_coor, = struct.unpack_from("<Q", bai, o)
        o += 8
    assert o == len(bai), "bytes behind the index"
    return dict(refs=refs, n_no_coor=n_no_coor)


def query(bai, ref, beg, end):
    """The chunks a reader has to scan for records of `ref` that overlap [beg, end): those of the bins of reg2bins that end behind the
    linear index's offset of the window of beg."""
    idx = bai if isinstance(bai, dict) else parse(bai)
    R = idx["refs"][ref]
    if beg >> 14 >= len(R["lin"]):
        return []                                              # no record reaches that window
    min_off = R["lin"][beg >> 14]
    out = []
    for b, chunks in R["bins"].items():                        # b in reg2bins(beg, end), without listing the up to 37 449 of them
        shift = 29 - 3 * level_of(b)
        if LEVEL_FIRST[level_of(b)] + (beg >> shift) <= b <= LEVEL_FIRST[level_of(b)] + ((end - 1) >> shift):
            out.extend(c for c in chunks if c[1] > min_off)
    return sorted(out)


def regions_of(records, n_ref, ref_len=MAX_END):
    """The fixed list of regions of the semantic test: every window boundary a record touches +-1, whole references (an empty one among
    them), single bases."""
    out = []
    for ref in range(n_ref):
        out.append((ref, 0, ref_len))
        edges = set()
        for rec in records:
            r, pos, e, _, _ = fields(rec, n_ref)
            if r == ref:
                for x in (pos, e - 1):
                    edges.update(((x >> 14) << 14, ((x >> 14) + 1) << 14, x))
        for x in sorted(edges):
            for y in (x - 1, x, x + 1):
                if 0 <= y < ref_len:
                    out.append((ref, y, y + 1))
                    out.append((ref, y, min(ref_len, y + 16384)))
            if 1 <= x < ref_len:
                out.append((ref, 0, x))
                out.append((ref, x, ref_len))
    return out


def check_semantics(bai, records, member_offsets, n_ref, regions=None):
    """Judge (b): holds for any valid index of these records, canonical or not.  Returns the number of (region, record) overlaps checked."""
    idx = parse(bai)
    assert len(idx["refs"]) == n_ref
    v = voffsets(records, member_offsets)
    f = [fields(r, n_ref) for r in records]
    bounds = set(v)
    for R in idx["refs"]:
        for chunks in R["bins"].values():
            for c in chunks:
                assert c[0] in bounds and c[1] in bounds, f"chunk {c} does not begin and end on a record boundary"
    assert idx["n_no_coor"] == sum(1 for x in f if x[0] < 0)
    by_ref = {}
    for i, x in enumerate(f):
        if x[0] >= 0:
            by_ref.setdefault(x[0], []).append(i)
    arrays = {}
    for ref, ii in by_ref.items():                             # numpy only to make the many regions quick: the comparisons are the ones above
        arrays[ref] = (np.array(ii), np.array([f[i][1] for i in ii], dtype=np.int64), np.array([f[i][2] for i in ii], dtype=np.int64),
                       np.array([v[i] for i in ii], dtype=np.uint64), np.array([v[i + 1] for i in ii], dtype=np.uint64))
    checked = 0
    for ref, beg, end in regions if regions is not None else regions_of(records, n_ref):
        got = query(idx, ref, beg, end)
        if ref not in arrays:
            continue
        ii, pos, e, vb, ve = arrays[ref]
        hit = np.nonzero((pos < end) & (e > beg))[0]
        if not len(hit):
            continue
        cb = np.array([c[0] for c in got], dtype=np.uint64)
        ce = np.array([c[1] for c in got], dtype=np.uint64)
        inside = ((cb[None, :] <= vb[hit, None]) & (ve[hit, None] <= ce[None, :])).any(axis=1) if len(got) else np.zeros(len(hit), dtype=bool)
        assert inside.all(), f"record {ii[hit[~inside][0]]} overlaps {ref}:{beg}-{end} and lies in no returned chunk"
        checked += len(hit)
    return checked
