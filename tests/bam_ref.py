"""SAM text <-> BAM records, written from the SAM specification (sections 1.4, 4.2, 4.2.1, 4.2.4, 5.3) -- the independent
reference the BAM tests compare against: the expected records are sam_to_bam_records() of SAM text that the REFERENCE side
produced.  Pure Python; nothing here calls the library under test."""
import struct
import numpy as np

CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"


def reg2bin(beg, end):
    """Section 5.3; Python's >> on negative integers is arithmetic, as the C code's on signed values."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def _int_tag(v):
    """The smallest type that holds the value: negative c s i, else C S I."""
    if v < 0:
        if v >= -128:
            return b"c" + struct.pack("<b", v)
        if v >= -32768:
            return b"s" + struct.pack("<h", v)
        assert v >= -2 ** 31
        return b"i" + struct.pack("<i", v)
    if v <= 255:
        return b"C" + struct.pack("<B", v)
    if v <= 65535:
        return b"S" + struct.pack("<H", v)
    assert v < 2 ** 32
    return b"I" + struct.pack("<I", v)


def _parse_cigar(s):
    ops, num = [], ""
    for ch in s:
        if ch.isdigit():
            num += ch
        else:
            ops.append((int(num), CIGAR_OPS.index(ch)))
            num = ""
    assert num == ""
    return ops


def sam_line_to_bam(line, contig_ids):
    f = line.split("\t")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    flag, pos, mapq, pnext, tlen = int(flag), int(pos) - 1, int(mapq), int(pnext) - 1, int(tlen)
    rid = -1 if rname == "*" else contig_ids[rname]
    nrid = -1 if rnext == "*" else rid if rnext == "=" else contig_ids[rnext]
    ops = [] if cigar == "*" else _parse_cigar(cigar)
    rlen = sum(n for n, op in ops if op in (0, 2, 3, 7, 8))
    end = pos + rlen if not (flag & 4) and ops and rlen else pos + 1
    name = qname.encode() + b"\0"
    assert len(name) <= 255
    l_seq = 0 if seq == "*" else len(seq)
    out = struct.pack("<iiBBHHHiiii", rid, pos, len(name), mapq, reg2bin(pos, end) & 0xffff, len(ops), flag, l_seq, nrid, pnext, tlen)
    out += name
    out += b"".join(struct.pack("<I", n << 4 | op) for n, op in ops)
    if l_seq:
        codes = [SEQ_CODES.index(c) for c in seq.upper()] + [0]
        out += bytes(codes[2 * i] << 4 | codes[2 * i + 1] for i in range((l_seq + 1) // 2))
        out += b"\xff" * l_seq if qual == "*" else bytes(c - 33 for c in qual.encode())
    for t in f[11:]:
        tag, ty, val = t[:2], t[3], t[5:]
        assert t[2] == ":" and t[4] == ":", t
        out += tag.encode()
        if ty == "i":
            out += _int_tag(int(val))
        elif ty == "Z":
            out += b"Z" + val.encode() + b"\0"
        elif ty == "A":
            assert len(val) == 1
            out += b"A" + val.encode()
        elif ty == "f":
            out += b"f" + np.float32(float(val)).tobytes()
        else:
            raise ValueError(f"tag type {ty} is not produced by bwa mem")
    return struct.pack("<i", len(out)) + out


def sam_to_bam_records(sam_text, contig_names):
    """SAM body (bytes or str; header lines are skipped) -> the concatenated BAM records."""
    if isinstance(sam_text, bytes):
        sam_text = sam_text.decode()
    ids = {n: i for i, n in enumerate(contig_names)}
    return b"".join(sam_line_to_bam(l, ids) for l in sam_text.split("\n") if l and not l.startswith("@"))


def split_records(buf):
    out, o = [], 0
    while o < len(buf):
        (bs,) = struct.unpack_from("<i", buf, o)
        assert bs >= 32 and o + 4 + bs <= len(buf), f"record at {o}: block_size {bs} does not fit {len(buf)} bytes"
        out.append(buf[o:o + 4 + bs])
        o += 4 + bs
    return out


def bam_record_to_sam(rec, contig_names, float_fmt="%.3f"):
    """One record -> its SAM line.  `f` tags print with float_fmt (bwa mem prints pa with three decimals)."""
    bs, rid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nrid, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    assert bs == len(rec) - 4
    o = 36
    name = rec[o:o + l_name - 1].decode()
    assert rec[o + l_name - 1] == 0
    o += l_name
    cig = "".join(f"{w >> 4}{CIGAR_OPS[w & 15]}" for w in struct.unpack_from(f"<{n_cig}I", rec, o)) or "*"
    o += 4 * n_cig
    if l_seq:
        sq = rec[o:o + (l_seq + 1) // 2]
        seq = "".join(SEQ_CODES[sq[i >> 1] >> 4 if i % 2 == 0 else sq[i >> 1] & 15] for i in range(l_seq))
        o += (l_seq + 1) // 2
        q = rec[o:o + l_seq]
        qual = "*" if q == b"\xff" * l_seq else bytes(c + 33 for c in q).decode()
        o += l_seq
    else:
        seq = qual = "*"
    f = [name, str(flag), "*" if rid < 0 else contig_names[rid], str(pos + 1), str(mapq), cig,
         "*" if nrid < 0 else "=" if nrid == rid else contig_names[nrid], str(npos + 1), str(tlen), seq, qual]
    while o < len(rec):
        tag, ty = rec[o:o + 2].decode(), chr(rec[o + 2])
        o += 3
        if ty in "cCsSiI":
            fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty]
            f.append(f"{tag}:i:{struct.unpack_from(fmt, rec, o)[0]}")
            o += struct.calcsize(fmt)
        elif ty == "Z":
            e = rec.index(b"\0", o)
            f.append(f"{tag}:Z:{rec[o:e].decode()}")
            o = e + 1
        elif ty == "A":
            f.append(f"{tag}:A:{chr(rec[o])}")
            o += 1
        elif ty == "f":
            f.append(f"{tag}:f:" + float_fmt % struct.unpack_from("<f", rec, o)[0])
            o += 4
        else:
            raise ValueError(f"tag type {ty}")
    return "\t".join(f)


def bam_records_to_sam(buf, contig_names):
    return "".join(bam_record_to_sam(r, contig_names) + "\n" for r in split_records(buf))


def contig_names_of(prefix):
    """Names from <prefix>.ann (bns_dump's layout, bntseq.c: first line l_pac n_seqs seed; then two lines per contig)."""
    lines = open(prefix + ".ann").read().split("\n")
    n = int(lines[0].split()[1])
    return [lines[1 + 2 * i].split(" ")[1] for i in range(n)]
