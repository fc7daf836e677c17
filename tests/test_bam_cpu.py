"""BAM output, the parts that need no GPU: the independent SAM <-> BAM reference the GPU tests rely on (tests/bam_ref.py, checked
against itself on the reference-made golden SAM and on hand-written records), bwahip_bam_header and the BGZF writer."""
import ctypes as C
import gzip
import os
import struct
import zlib

import pytest

import bam_ref
import common
from common import bw

GOLDEN_CONTIGS = ["ctg1", "ctg2", "ctg3"]
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _golden_sams():
    return sorted(f for f in os.listdir(common.GOLDEN) if f.endswith(".sam.gz"))


@pytest.mark.parametrize("name", _golden_sams())
def test_bam_ref_round_trip_on_golden_sam(name):
    text = gzip.open(os.path.join(common.GOLDEN, name)).read().decode()
    body = "".join(l + "\n" for l in text.split("\n") if l and not l.startswith("@"))
    rec = bam_ref.sam_to_bam_records(body, GOLDEN_CONTIGS)
    assert len(bam_ref.split_records(rec)) == body.count("\n")
    assert bam_ref.bam_records_to_sam(rec, GOLDEN_CONTIGS) == body


def test_golden_sam_covers_the_record_kinds():
    """What the round trip above is said to cover is really in the files."""
    se = gzip.open(os.path.join(common.GOLDEN, "se.sam.gz")).read().decode().split("\n")
    al = gzip.open(os.path.join(common.GOLDEN, "se_all.sam.gz")).read().decode().split("\n")
    pe = gzip.open(os.path.join(common.GOLDEN, "pe.sam.gz")).read().decode()
    assert sum(1 for l in se if l and int(l.split("\t")[1]) & 4) == 34
    assert sum(1 for l in al if l and int(l.split("\t")[1]) & 0x100 and l.split("\t")[9] == "*") == 866
    assert any("H" in l.split("\t")[5] and int(l.split("\t")[1]) & 0x800 for l in se if l)
    assert "SA:Z:" in "\n".join(se) and "XA:Z:" in "\n".join(se) and "pa:f:" in "\n".join(se) and "MC:Z:" in pe
    assert any(l and int(l.split("\t")[1]) & 8 and not int(l.split("\t")[1]) & 4 for l in pe.split("\n"))


def _tags(rec):
    """[(tag, type, raw value bytes)] of one record."""
    l_name, n_cig, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    o = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    out = []
    while o < len(rec):
        tag, ty = rec[o:o + 2].decode(), chr(rec[o + 2])
        o += 3
        n = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "A": 1}.get(ty) or rec.index(b"\0", o) + 1 - o
        out.append((tag, ty, rec[o:o + n]))
        o += n
    return out


def test_bam_ref_hand_written_records():
    # integer tags at the type boundaries
    line = "r1\t0\tctg1\t100\t60\t5M\t*\t0\t0\tACGTN\tIIII#\t" + "\t".join(
        f"X{c}:i:{v}" for c, v in zip("abcdefghijk", (255, 256, 65535, 65536, -1, -128, -129, -32768, -32769, 0, 4294967295)))
    rec = bam_ref.sam_to_bam_records(line + "\n", GOLDEN_CONTIGS)
    assert [t[1] for t in _tags(rec)] == list("CSSIccssiCI")
    assert bam_ref.bam_records_to_sam(rec, GOLDEN_CONTIGS) == line + "\n"
    # fixed part of a mapped record: refID 0, pos 99, l_read_name 3, mapq 60, bin of [99, 104), one CIGAR op, l_seq 5 (odd)
    bs, rid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nrid, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    assert (bs, rid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nrid, npos, tlen) == (len(rec) - 4, 0, 99, 3, 60, 4681, 1, 0, 5, -1, -1, 0)
    assert rec[36:39] == b"r1\0" and struct.unpack_from("<I", rec, 39)[0] == 5 << 4
    assert rec[43:46] == bytes([0x12, 0x48, 0xf0]) and rec[46:51] == bytes([40, 40, 40, 40, 2])     # A C | G T | N, pad 0
    # unmapped, no qualities: refID = pos = -1 -> bin 4680, QUAL 0xFF
    line = "u\t4\t*\t0\t0\t*\t*\t0\t0\tACG\t*\tAS:i:0\tXS:i:0"
    rec = bam_ref.sam_to_bam_records(line, GOLDEN_CONTIGS)
    assert struct.unpack_from("<iiBBH", rec, 4) == (-1, -1, 2, 0, 4680)
    assert rec[38:40] == bytes([0x12, 0x40]) and rec[40:43] == b"\xff\xff\xff"
    assert bam_ref.bam_records_to_sam(rec, GOLDEN_CONTIGS) == line + "\n"
    # clips use BAM's codes (S = 4, H = 5); mate on another contig; pa:f is the single nearest to the printed text
    line = "p\t2145\tctg2\t7\t3\t10H4M1I3M2S\tctg3\t1\t0\tACGTACGTAC\tABCDEFGHIJ\tNM:i:1\tMD:Z:7\tpa:f:0.913\tZA:A:x"
    rec = bam_ref.sam_to_bam_records(line, GOLDEN_CONTIGS)
    assert [w & 15 for w in struct.unpack_from("<5I", rec, 36 + 2)] == [5, 0, 1, 0, 4]
    assert struct.unpack_from("<i", rec, 24)[0] == 2                                            # next_refID
    import numpy as np
    assert dict((t[0], t[2]) for t in _tags(rec))["pa"] == np.float32(0.913).tobytes()
    assert bam_ref.bam_records_to_sam(rec, GOLDEN_CONTIGS) == line + "\n"


# ------------------------------------------------------------------------------------------------------------------- header
@pytest.fixture(scope="module")
def golden_index(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("g60k")
    fa = str(d / "g60k.fa")
    open(fa, "wb").write(gzip.open(os.path.join(common.GOLDEN, "g60k.fa.gz")).read())
    bw.make_index(fa, str(d / "g60k"))
    return str(d / "g60k")


def _bns_from_files(prefix):
    """bw.Bns filled from <prefix>.ann and the golden .alt list, as bns_restore does; returns (bns, [(name, len, is_alt)], keep-alive)."""
    lines = open(prefix + ".ann").read().split("\n")
    l_pac, n, seed = (int(x) for x in lines[0].split())
    alt = set(open(os.path.join(common.GOLDEN, "g60k.alt")).read().split())
    anns = (bw.Ann * n)()
    table = []
    for i in range(n):
        gi, name, anno = lines[1 + 2 * i].split(" ", 2)
        off, ln, n_ambs = (int(x) for x in lines[2 + 2 * i].split())
        anns[i].offset, anns[i].len, anns[i].n_ambs, anns[i].gi, anns[i].is_alt = off, ln, n_ambs, int(gi), int(name in alt)
        anns[i].name, anns[i].anno = name.encode(), anno.encode()
        table.append((name, ln, name in alt))
    bns = bw.Bns()
    bns.l_pac, bns.n_seqs, bns.seed, bns.anns = l_pac, n, seed, anns
    bns.n_holes = int(open(prefix + ".amb").read().split("\n")[0].split()[2])
    return bns, table, anns


def _parse_header(h):
    assert h[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", h, 4)
    text = h[8:8 + l_text]
    o = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", h, o)
    o += 4
    refs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", h, o)
        name = h[o + 4:o + 4 + l_name]
        assert name[-1] == 0
        (l_ref,) = struct.unpack_from("<i", h, o + 4 + l_name)
        refs.append((name[:-1].decode(), l_name, l_ref))
        o += 8 + l_name
    assert o == len(h)
    return text.decode(), refs


def test_bam_header(golden_index):
    bns, table, _keep = _bns_from_files(golden_index)
    assert [t[0] for t in table] == GOLDEN_CONTIGS and [t[2] for t in table] == [False, False, True]
    sq = "".join(f"@SQ\tSN:{n}\tLN:{ln}" + ("\tAH:*\n" if alt else "\n") for n, ln, alt in table)       # bwa.c:531-535
    want_refs = [(n, len(n) + 1, ln) for n, ln, _ in table]
    text, refs = _parse_header(bw.bam_header(bns))
    assert text == sq and refs == want_refs
    rg = "@RG\tID:grp7\tSM:sample"
    text, refs = _parse_header(bw.bam_header(bns, rg))
    assert text == sq + rg + "\n" and refs == want_refs                                                  # bwa.c:539
    own = "@HD\tVN:1.6\n@SQ\tSN:ctg1\tLN:40000\tM5:x\n@SQ\tSN:ctg2\tLN:16000\n@SQ\tSN:ctg3\tLN:4000\n@PG\tID:bwa"
    text, refs = _parse_header(bw.bam_header(bns, own))
    assert text == own + "\n" and refs == want_refs                                                      # bwa.c:524-530: none generated


# ------------------------------------------------------------------------------------------------------------------- BGZF
def _parse_bgzf(buf):
    """[(block length, ISIZE)]; every block is checked: gzip magic, the BC subfield, BSIZE, the raw deflate stream, CRC32, ISIZE."""
    out, o, data = [], 0, b""
    while o < len(buf):
        assert buf[o:o + 4] == b"\x1f\x8b\x08\x04" and struct.unpack_from("<H", buf, o + 10)[0] == 6
        assert buf[o + 12:o + 14] == b"BC" and struct.unpack_from("<H", buf, o + 14)[0] == 2
        bsize = struct.unpack_from("<H", buf, o + 16)[0] + 1
        assert bsize <= 65536 and o + bsize <= len(buf)
        z = zlib.decompressobj(-15)
        raw = z.decompress(buf[o + 18:o + bsize - 8]) + z.flush()
        crc, isize = struct.unpack_from("<II", buf, o + bsize - 8)
        assert isize == len(raw) and isize <= 65280 and crc == zlib.crc32(raw)
        out.append((bsize, isize))
        data += raw
        o += bsize
    return out, data


def _bgzf(tmp_path, data, level, threads):
    path = str(tmp_path / "x.bgzf")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        bw.bgzf_write(fd, data, level, threads, eof=True)
    finally:
        os.close(fd)
    return open(path, "rb").read()


def test_bgzf_writer(built, tmp_path):
    sam = b"".join(gzip.open(os.path.join(common.GOLDEN, f)).read() for f in _golden_sams())
    big = (sam * (1 + (3 << 20) // len(sam)))[:(3 << 20) + 12345]
    sizes = [b"", b"x", big[:65280], big[:65281], big]
    for level in (0, 1, 6):
        for data in sizes:
            one = _bgzf(tmp_path, data, level, 1)
            four = _bgzf(tmp_path, data, level, 4)
            assert one == four, f"level {level}, {len(data)} bytes: the file depends on the number of threads"
            assert one.endswith(BGZF_EOF)
            assert gzip.decompress(one) == data
            blocks, back = _parse_bgzf(one)
            assert back == data and blocks[-1] == (28, 0)
            assert [b[1] for b in blocks[:-1]] == [min(65280, len(data) - k) for k in range(0, len(data), 65280)]
            if level == 0 and data:
                assert len(one) == len(data) + 31 * (len(blocks) - 1) + 28
    assert len(_bgzf(tmp_path, big, 1, 4)) < len(big) // 2 < len(_bgzf(tmp_path, big, 0, 4))         # level 1 deflates, level 0 stores


def test_bgzf_rejects_bad_arguments(built):
    assert bw.lib().bwahip_bgzf_write(-1, None, 5, 1, 1) == -1
    assert bw.lib().bwahip_bgzf_write(-1, b"abc", 3, 10, 1) == -1
    assert bw.lib().bwahip_bgzf_write(-1, b"abc", 3, 1, 1) == 0          # fd < 0: produced and dropped
