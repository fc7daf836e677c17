"""BAM records encoded on the GPU (k_bam.hip) and the BAM file of the stream driver.  The expected bytes never come from the code under
test: they are tests/bam_ref.py (written from the SAM specification) applied to SAM text the REFERENCE side produced -- the committed
golden files and oracle/bwa_oracle output, exactly as the SAM tests obtain their expectation.  Byte for byte, no tolerance."""
import gzip
import os
import random
import re
import subprocess

import pytest

import bam_ref
import common
from common import bw

pytestmark = pytest.mark.gpu

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden(built, tmp_path_factory):
    """The 60 kb golden genome (ALT contig with an annotation) and the golden reads."""
    G, d = common.GOLDEN, tmp_path_factory.mktemp("g60k")
    fa = str(d / "g60k.fa")
    open(fa, "wb").write(gzip.open(os.path.join(G, "g60k.fa.gz")).read())
    bw.make_index(fa, str(d / "g60k"))
    open(str(d / "g60k.alt"), "wb").write(open(os.path.join(G, "g60k.alt"), "rb").read())
    for n in ("se.fq", "pe_1.fq", "pe_2.fq", "long.fq"):
        open(str(d / n), "wb").write(gzip.open(os.path.join(G, n + ".gz")).read())
    return {"dir": str(d), "prefix": str(d / "g60k")}


def _oracle_sam(prefix, fqs, extra=()):
    out = subprocess.run([common.ORACLE, "mem", "-t", "8", *extra, prefix, *fqs], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    return b"".join(l + b"\n" for l in out.split(b"\n") if l and not l.startswith(b"@"))


def _interleave(a, b):
    return [x for p in zip(a, b) for x in p]


def _pe_reads(fq1, fq2):
    n1, s1, q1 = bw.read_fastq(fq1)
    n2, s2, q2 = bw.read_fastq(fq2)
    return _interleave(n1, n2), _interleave(s1, s2), _interleave(q1, q2)


def _assert_records(got, want_sam, contigs, what):
    want = bam_ref.sam_to_bam_records(want_sam, contigs)
    if got == want:
        return
    g, w = bam_ref.split_records(got), bam_ref.split_records(want)
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            raise AssertionError(f"{what}: record {i} of {len(w)} differs\n got  {bam_ref.bam_record_to_sam(a, contigs)}\n      {a.hex()}\n want {bam_ref.bam_record_to_sam(b, contigs)}\n      {b.hex()}")
    raise AssertionError(f"{what}: {len(g)} records vs {len(w)}")


def test_golden_reference_sam_as_bam(golden):
    """SE (ALT contig, chimeras, N's, reads shorter than a seed), SE -a (secondary records without SEQ), PE, and the option sets of the
    golden sweep (incl. the 600-base reads) vs SAM the reference itself produced."""
    G, d = common.GOLDEN, golden["dir"]
    contigs = bam_ref.contig_names_of(golden["prefix"])
    se = bw.read_fastq(os.path.join(d, "se.fq"))
    lg = bw.read_fastq(os.path.join(d, "long.fq"))
    pe = _pe_reads(os.path.join(d, "pe_1.fq"), os.path.join(d, "pe_2.fq"))
    with bw.Context(golden["prefix"]) as c:
        opt = bw.default_opt()
        opt.n_threads = 4
        _assert_records(c.process_seqs_bam(*se, opt), gzip.open(os.path.join(G, "se.sam.gz")).read(), contigs, "se")
        opt.flag |= 0x8                                                   # -a
        _assert_records(c.process_seqs_bam(*se, opt), gzip.open(os.path.join(G, "se_all.sam.gz")).read(), contigs, "se -a")
        opt = bw.default_opt()
        opt.n_threads = 4
        opt.flag |= 0x2
        _assert_records(c.process_seqs_bam(*pe, opt), gzip.open(os.path.join(G, "pe.sam.gz")).read(), contigs, "pe")
        for name in common.GOLDEN_OPTION_SETS:
            opt, pes0 = common.opt_from_cli(common.option_flags(name))
            opt.n_threads = 4
            reads = pe if name in common.PE_OPTION_SETS else lg if name in common.LONG_OPTION_SETS else se
            if name in common.PE_OPTION_SETS:
                opt.flag |= 0x2
            _assert_records(c.process_seqs_bam(*reads, opt, pes0=pes0), gzip.open(os.path.join(G, f"opt_{name}.sam.gz")).read(), contigs, name)


@pytest.mark.parametrize("name,flags,pe,length,needs", [
    ("M_Y_5", ["-M", "-Y", "-5"], False, 150, rb"SA:Z:"),
    ("M_Y_5_pe", ["-M", "-Y", "-5"], True, 150, rb"MC:Z:"),
    ("default", [], False, 150, rb"\t\d+H\d+M|M\d+H\t"),     # supplementary lines with hard clips
    ("default_pe", [], True, 150, rb"MC:Z:"),
    ("u", ["-u"], False, 150, rb"XB:Z:"),
    ("A2_long", ["-A", "2"], False, 600, None),
])
def test_bam_vs_oracle_on_generated_reads(ctx, small_index, tmp_path, name, flags, pe, length, needs):
    """Generated reads with indels, N's and chimeras under options that change what a record holds."""
    fq1, fq2 = str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq")
    n = 600 if length > 200 else 3000
    bw.make_reads(small_index["fa"], fq1, fq2 if pe else None, n, length, 20000, 3000, 1000, 311, 30000)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = _oracle_sam(small_index["prefix"], [fq1, fq2] if pe else [fq1], flags)
    if needs:
        assert re.search(needs, want), f"{name}: the expectation does not exercise {needs}"
    if name == "A2_long":                                         # AS above 255 -> type S: the case cannot pass vacuously
        big = [int(f[5:]) for l in want.decode().split("\n") for f in l.split("\t")[11:] if f.startswith("AS:i:")]
        assert any(v > 255 for v in big) and any(v <= 255 for v in big)
    opt, pes0 = common.opt_from_cli(flags)
    opt.n_threads = 8
    if pe:
        opt.flag |= 0x2
    reads = _pe_reads(fq1, fq2) if pe else bw.read_fastq(fq1)
    _assert_records(ctx.process_seqs_bam(*reads, opt, pes0=pes0), want, contigs, name)


def test_read_group_and_reference_annotation(golden):
    """-R (RG:Z: on every record) and -V (XR:Z: from the contig's annotation; the golden ALT contig has one)."""
    contigs = bam_ref.contig_names_of(golden["prefix"])
    fq = os.path.join(golden["dir"], "se.fq")
    want = _oracle_sam(golden["prefix"], [fq], ["-V", "-R", "@RG\\tID:grp7\\tSM:sample"])
    assert b"RG:Z:grp7" in want and b"XR:Z:" in want
    opt, _ = common.opt_from_cli(["-V"])
    opt.n_threads = 4
    with bw.Context(golden["prefix"]) as c:
        c.set_rg_id("grp7")
        _assert_records(c.process_seqs_bam(*bw.read_fastq(fq), opt), want, contigs, "-V -R")


def test_fasta_reads_have_no_qualities(ctx, small_index, tmp_path):
    fq, fa = str(tmp_path / "q.fq"), str(tmp_path / "q.fa")
    bw.make_reads(small_index["fa"], fq, None, 1000, 151, 10000, 2000, 500, 313, 20000)     # odd length: the last SEQ nibble is padding
    names, seqs, _ = bw.read_fastq(fq)
    open(fa, "wb").write(b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    want = _oracle_sam(small_index["prefix"], [fa])
    assert all(l.split(b"\t")[10] == b"*" for l in want.split(b"\n") if l)
    opt = bw.default_opt()
    opt.n_threads = 4
    _assert_records(ctx.process_seqs_bam(names, seqs, None, opt), want, bam_ref.contig_names_of(small_index["prefix"]), "fasta")


def test_unmapped_reads_and_half_mapped_pairs(ctx, small_index, tmp_path):
    """Random reads do not map: refID = pos = -1, bin 4680; a pair with one random end takes the mapped mate's position (bwamem.c:842-845)."""
    rnd = random.Random(7)
    fq1, fq2, g1, g2 = (str(tmp_path / x) for x in ("u_1.fq", "u_2.fq", "g_1.fq", "g_2.fq"))
    bw.make_reads(small_index["fa"], g1, g2, 1600, 150, 10000, 1000, 300, 317)     # 800 pairs: 200 of each kind below
    n1, s1, q1 = bw.read_fastq(g1)
    n2, s2, q2 = bw.read_fastq(g2)
    for k in range(len(s1)):
        r = bytes(rnd.choice(b"ACGT") for _ in range(150))
        if k % 4 == 1:
            s1[k] = r
        elif k % 4 == 2:
            s2[k] = r
        elif k % 4 == 3:
            s1[k], s2[k] = r, bytes(rnd.choice(b"ACGT") for _ in range(150))
    for path, (nn, ss, qq) in ((fq1, (n1, s1, q1)), (fq2, (n2, s2, q2))):
        open(path, "wb").write(b"".join(b"@" + a + b"\n" + b + b"\n+\n" + c + b"\n" for a, b, c in zip(nn, ss, qq)))
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    opt = bw.default_opt()
    opt.n_threads = 4
    want = _oracle_sam(small_index["prefix"], [fq1])
    assert sum(1 for l in want.split(b"\n") if l and int(l.split(b"\t")[1]) & 4) >= 400              # the 400 random first reads
    _assert_records(ctx.process_seqs_bam(n1, s1, q1, opt), want, contigs, "unmapped se")
    want = _oracle_sam(small_index["prefix"], [fq1, fq2])
    fl = [int(l.split(b"\t")[1]) for l in want.split(b"\n") if l]
    assert sum(1 for f in fl if f & 8 and not f & 4) >= 300 and sum(1 for f in fl if f & 4 and not f & 8) >= 300 and sum(1 for f in fl if f & 4 and f & 8) >= 400
    opt.flag |= 0x2
    _assert_records(ctx.process_seqs_bam(_interleave(n1, n2), _interleave(s1, s2), _interleave(q1, q2), opt), want, contigs, "half-mapped pe")


def _with_comments(fq, make):
    lines = open(fq).read().split("\n")
    comments = []
    for i in range(0, len(lines) - 3, 4):
        c = make(i // 4)
        comments.append(c.encode() if c else None)
        if c:
            lines[i] += " " + c
    open(fq, "w").write("\n".join(lines))
    return comments


def test_comments_become_tags(ctx, small_index, tmp_path):
    """-C: each tab-separated field of the FASTQ comment is stored as the tag it spells (Z, i by the smallest-type rule, A)."""
    fq = str(tmp_path / "c.fq")
    bw.make_reads(small_index["fa"], fq, None, 900, 150, 10000, 2000, 500, 319, 20000)
    cm = _with_comments(fq, lambda k: None if k % 3 == 0 else f"BC:Z:{'ACGT'[k % 4] * 6}\tXY:i:-7\tZA:A:x" if k % 3 == 1 else f"XZ:i:{k * 97}\tBC:Z:a b")
    names, seqs, quals = bw.read_fastq(fq)
    want = _oracle_sam(small_index["prefix"], [fq], ["-C"])
    assert b"XY:i:-7\tZA:A:x" in want and b"BC:Z:a b" in want and b"XZ:i:" + str(800 * 97).encode() in want
    opt = bw.default_opt()
    opt.n_threads = 4
    _assert_records(ctx.process_seqs_bam(names, seqs, quals, opt, comments=cm), want, bam_ref.contig_names_of(small_index["prefix"]), "-C")


def test_offsets_cut_at_record_boundaries(ctx, small_index, tmp_path):
    fq = str(tmp_path / "o.fq")
    bw.make_reads(small_index["fa"], fq, None, 1500, 150, 10000, 2000, 500, 323, 40000)
    names, seqs, quals = bw.read_fastq(fq)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = _oracle_sam(small_index["prefix"], [fq]).decode().split("\n")[:-1]
    per_read = {}
    for l in want:
        per_read.setdefault(l.split("\t")[0], []).append(l)
    assert any(len(v) > 1 for v in per_read.values())
    opt = bw.default_opt()
    opt.n_threads = 4
    rec, off = ctx.process_seqs_bam(names, seqs, quals, opt, want_offsets=True)
    assert off[0] == 0 and off[-1] == len(rec) and len(off) == len(names) + 1
    for i, nm in enumerate(names):
        lines = bam_ref.bam_records_to_sam(rec[off[i]:off[i + 1]], contigs).split("\n")[:-1]       # split_records asserts the cut is clean
        assert lines == per_read[nm.decode()], f"read {i}"


def test_device_resident_pair_gives_the_same_bytes(ctx, small_index, tmp_path):
    """bwahip_batch_run_bam / bwahip_batch_bam over a batch that is resident in HBM == bwahip_process_seqs_bam.  The batch is made
    resident by a SAM call on a second context (reads, names and qualities stay in its device buffers), then finalised as BAM there."""
    fq1, fq2 = str(tmp_path / "d_1.fq"), str(tmp_path / "d_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 2000, 150, 10000, 1000, 300, 329, 20000)
    reads = _pe_reads(fq1, fq2)
    opt = bw.default_opt()
    opt.n_threads = 4
    opt.flag |= 0x2
    want = ctx.process_seqs_bam(*reads, opt)
    _assert_records(want, _oracle_sam(small_index["prefix"], [fq1, fq2]), bam_ref.contig_names_of(small_index["prefix"]), "pe")
    with bw.Context(small_index["prefix"]) as c:
        arr, keep = bw.seq_array(*reads)
        sam = c.process_seqs_text_array(arr, len(reads[0]), opt)
        ms = c.batch_run_bam(opt)
        assert ms["k_sam_size"] > 0 and ms["k_sam_write"] > 0
        assert c.batch_bam() == want
        c.batch_run_sam(opt)                                      # and back: the text of the same resident batch
        assert c.batch_sam() == sam


@pytest.mark.parametrize("n_ctx", [1, 2, 3])
def test_stream_driver_files_to_bam(small_index, tmp_path, n_ctx):
    """bwahip_stream_run_bam: the inflated file is the header followed by the records of the whole input in order; it ends with the
    EOF block; several batches and several BGZF blocks per batch."""
    fq1, fq2 = str(tmp_path / "s_1.fq"), str(tmp_path / "s_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 4300, 150, 10000, 2000, 500, 171, 20000)
    K = 600 * 150
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    hdr = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            opt = bw.default_opt()
            opt.n_threads = 4
            for a, b in ((fq1, fq2), (fq1, None)):
                want = bw.bam_header(c0, hdr) + bam_ref.sam_to_bam_records(_oracle_sam(small_index["prefix"], [a, b] if b else [a], ["-K", str(K)]), contigs)
                for level in (0, 1):
                    out = str(tmp_path / "out.bam")
                    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                    try:
                        st = bw.stream_run_bam(ctxs, a, b, fd, hdr, level, opt, chunk_bases=K, reader_threads=2)
                    finally:
                        os.close(fd)
                    got = open(out, "rb").read()
                    assert got.endswith(BGZF_EOF)
                    assert gzip.decompress(got) == want, f"n_ctx {n_ctx}, level {level}, {'pe' if b else 'se'}"
                    assert st.n_batches == (8 if b else 4) and st.n_reads == (4300 if b else 2150)
                    assert st.sam_bytes == len(want) - len(bw.bam_header(c0, hdr))
                    assert len(got) > 3 * 65536 if level == 0 else len(got) < len(want) // 2
            st = bw.stream_run_bam(ctxs, fq1, fq2, -1, None, 1, opt, chunk_bases=K, max_reads=1000)        # produced and dropped
            assert st.n_reads == 1200 and st.n_batches == 2
        finally:
            for c in ctxs[1:]:
                c.close()


def test_what_bam_cannot_hold_is_refused_and_the_context_stays_usable(ctx, small_index, tmp_path):
    fq = str(tmp_path / "e.fq")
    bw.make_reads(small_index["fa"], fq, None, 200, 150, 10000, 2000, 500, 331)
    names, seqs, quals = bw.read_fastq(fq)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = _oracle_sam(small_index["prefix"], [fq])
    opt = bw.default_opt()
    opt.n_threads = 4
    casava = [None] * 200
    casava[17] = b"1:N:0:ACGT"
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        ctx.process_seqs_bam(names, seqs, quals, opt, comments=casava)
    _assert_records(ctx.process_seqs_bam(names, seqs, quals, opt), want, contigs, "after the refused comment")
    for bad in (b"XY:i:4294967296", b"XY:i:-2147483649", b"XY:Z:a\x01b", b"X:Z:a", b"XY:A:ab", b"XY:f:1.5"):
        casava[17] = bad
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.process_seqs_bam(names, seqs, quals, opt, comments=casava)
    long_names = list(names)
    long_names[5] = b"n" * 255
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        ctx.process_seqs_bam(long_names, seqs, quals, opt)
    _assert_records(ctx.process_seqs_bam(names, seqs, quals, opt), want, contigs, "after the refused name")
    long_names[5] = b"n" * 254                                    # the longest name a record holds
    got = bam_ref.split_records(ctx.process_seqs_bam(long_names, seqs, quals, opt))
    assert any(r[12] == 255 and r[36:36 + 255] == b"n" * 254 + b"\0" for r in got)


def test_the_format_does_not_leak(ctx, small_index, tmp_path):
    """SAM after BAM on one context is byte-identical to a fresh context's SAM (SE and PE)."""
    fq1, fq2 = str(tmp_path / "l_1.fq"), str(tmp_path / "l_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 1500, 150, 10000, 2000, 500, 337, 20000)
    reads = _pe_reads(fq1, fq2)
    for pe in (False, True):
        opt = bw.default_opt()
        opt.n_threads = 4
        if pe:
            opt.flag |= 0x2
        rd = reads if pe else bw.read_fastq(fq1)
        ctx.process_seqs_bam(*rd, opt)
        arr, keep = bw.seq_array(*rd)
        got = ctx.process_seqs_text_array(arr, len(rd[0]), opt)
        with bw.Context(small_index["prefix"]) as fresh:
            arr2, keep2 = bw.seq_array(*rd)
            want = fresh.process_seqs_text_array(arr2, len(rd[0]), opt)
        assert got == want and got == _oracle_sam(small_index["prefix"], [fq1, fq2] if pe else [fq1])
