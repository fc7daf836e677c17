"""Coordinate-sorted BAM: the radix sort alone against numpy's stable argsort, a batch's sorted records, keys and offsets, ties, the
device-resident pair, and the stream driver with its merger.  Expected bytes never come from the code under test: they are
tests/bam_ref.py applied to oracle or golden SAM (as in test_gpu_bam.py), reordered by Python's stable sorted() on a key read from the
record's own bytes (tests/bam_sort_ref.py).  Byte for byte, no tolerance."""
import collections
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import bam_ref
import bam_sort_ref as sref
import common
from common import bw

pytestmark = pytest.mark.gpu

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


def _oracle_sam(prefix, fqs, extra=()):
    out = subprocess.run([common.ORACLE, "mem", "-t", "8", *extra, prefix, *fqs], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    return b"".join(l + b"\n" for l in out.split(b"\n") if l and not l.startswith(b"@"))


def _interleave(a, b):
    return [x for p in zip(a, b) for x in p]


def _pe_reads(fq1, fq2):
    n1, s1, q1 = bw.read_fastq(fq1)
    n2, s2, q2 = bw.read_fastq(fq2)
    return _interleave(n1, n2), _interleave(s1, s2), _interleave(q1, q2)


def _write_fastq(path, names, seqs, quals):
    open(path, "wb").write(b"".join(b"@" + a + b"\n" + b + b"\n+\n" + c + b"\n" for a, b, c in zip(names, seqs, quals)))


# ------------------------------------------------------------------------------------------------------------ 1. the sort alone
def _patterns(n, rng):
    """name -> (keys, key_bits)"""
    ar = np.arange(n, dtype=np.uint64)
    p = {
        "all equal": (np.full(n, 0x0123456789abcdef, dtype=np.uint64), 64),
        "two values": (np.where(ar % 2 == 0, np.uint64(7 << 40), np.uint64(3)), 64),
        "sorted": (ar * np.uint64(1000003), 64),
        "reversed": ((np.uint64(n) - ar) * np.uint64(1000003), 64),
        "bits 40-47 only": (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(40), 64),       # the lower passes must keep the order
    }
    for bits in (1, 8, 9, 34, 64):
        p[f"random {bits} bits"] = (rng.integers(0, 1 << bits, n, dtype=np.uint64, endpoint=False) if bits < 64 else rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False), bits)
    return p


def test_radix_sort_known_answers(ctx):
    _, T = ctx.kat_radix_sort(np.zeros(0, dtype=np.uint64))
    assert T >= 256 and T % 64 == 0
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17, 300_000):
        for name, (keys, bits) in _patterns(n, rng).items():
            keys = keys.astype(np.uint64)
            want = np.argsort(keys, kind="stable").astype(np.uint32)
            got, t2 = ctx.kat_radix_sort(keys, bits)
            assert t2 == T
            assert np.array_equal(got, want), f"n {n}, {name}: first difference at {int(np.argmax(got != want))}"
            again, _ = ctx.kat_radix_sort(keys, bits)
            assert np.array_equal(again, got), f"n {n}, {name}: two runs differ"


# ------------------------------------------------------------------------------------------------------------ 2. a batch vs the oracle
def _props(records):
    f = [sref.fields(r) for r in records]
    flags = [int.from_bytes(r[18:20], "little") for r in records]
    return dict(contigs=len({x[0] for x in f if x[0] >= 0}), supp=sum(1 for x in flags if x & 0x800), no_ref=sum(1 for x in f if x[0] < 0),
                strands=len({x[2] for x in f}), no_seq=sum(1 for r, x in zip(records, flags) if x & 0x100 and int.from_bytes(r[20:24], "little") == 0))


def _assert_sorted_batch(c, got, want_sam, contigs, what):
    rec, keys, off = got
    want_recs = sref.stable_sort(bam_ref.split_records(bam_ref.sam_to_bam_records(want_sam, contigs)))
    want = b"".join(want_recs)
    assert len(keys) == len(want_recs) and len(off) == len(keys) + 1, what
    if rec != want:
        for i, (a, b) in enumerate(zip(bam_ref.split_records(rec), want_recs)):
            assert a == b, f"{what}: record {i} of {len(want_recs)} differs\n got  {bam_ref.bam_record_to_sam(a, contigs)}\n want {bam_ref.bam_record_to_sam(b, contigs)}"
        raise AssertionError(f"{what}: {len(rec)} bytes vs {len(want)}")
    assert off[0] == 0 and off[-1] == len(rec)
    assert [int(x) for x in np.diff(off)] == [len(r) for r in want_recs], f"{what}: rec_off does not cut at the records"
    assert np.all(keys[1:] >= keys[:-1]), f"{what}: keys decrease"
    assert [int(k) for k in keys] == [bw.bam_sort_key(c, *sref.fields(r)) for r in want_recs], f"{what}: keys are not bwahip_bam_sort_key of their records"
    return want_recs


def test_sorted_batch_generated_reads_with_chimeras(ctx, small_index, tmp_path):
    """3000 paired reads of 150 bases and their single-end half.  The read generator applies chim_ppm to single-end sets only
    (tools/simgen.c: `!is_pe && chim_ppm`; a paired call with chim_ppm = 20000 gives the same files as one without), and the expectation
    must hold supplementary records: so every eighth first mate is replaced, under its own name, by a read of a single-end set generated
    with chimeras."""
    fq1, fq2, fqc = str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq"), str(tmp_path / "c.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 3000, 150, 10000, 2000, 500, 411, chim_ppm=20000)
    bw.make_reads(small_index["fa"], fqc, None, 1500, 150, 10000, 2000, 500, 413, chim_ppm=200000)
    n1, s1, q1 = bw.read_fastq(fq1)
    _, sc, qc = bw.read_fastq(fqc)
    assert len(n1) == len(sc) == 1500
    for k in range(0, 1500, 8):
        s1[k], q1[k] = sc[k], qc[k]
    _write_fastq(fq1, n1, s1, q1)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    opt = bw.default_opt()
    opt.n_threads = 8
    want = _oracle_sam(small_index["prefix"], [fq1])
    p = _props(bam_ref.split_records(bam_ref.sam_to_bam_records(want, contigs)))
    assert p["contigs"] >= 2 and p["supp"] >= 1 and p["strands"] == 2, p
    _assert_sorted_batch(ctx, ctx.process_seqs_bam_sorted(*bw.read_fastq(fq1), opt), want, contigs, "se")
    want = _oracle_sam(small_index["prefix"], [fq1, fq2])
    p = _props(bam_ref.split_records(bam_ref.sam_to_bam_records(want, contigs)))
    assert p["contigs"] >= 2 and p["supp"] >= 1 and p["strands"] == 2, p
    opt.flag |= 0x2
    _assert_sorted_batch(ctx, ctx.process_seqs_bam_sorted(*_pe_reads(fq1, fq2), opt), want, contigs, "pe")


def test_sorted_batch_golden_all_alignments(built, tmp_path):
    """The 60 kb golden genome (ALT contig), single-end with -a: secondary records without SEQ among the sorted ones."""
    G, d = common.GOLDEN, tmp_path
    fa = str(d / "g60k.fa")
    open(fa, "wb").write(gzip.open(os.path.join(G, "g60k.fa.gz")).read())
    bw.make_index(fa, str(d / "g60k"))
    open(str(d / "g60k.alt"), "wb").write(open(os.path.join(G, "g60k.alt"), "rb").read())
    open(str(d / "se.fq"), "wb").write(gzip.open(os.path.join(G, "se.fq.gz")).read())
    contigs = bam_ref.contig_names_of(str(d / "g60k"))
    want = gzip.open(os.path.join(G, "se_all.sam.gz")).read()
    p = _props(bam_ref.split_records(bam_ref.sam_to_bam_records(want, contigs)))
    assert p["no_seq"] >= 100 and p["contigs"] >= 2 and p["strands"] == 2 and p["supp"] >= 1, p
    opt = bw.default_opt()
    opt.n_threads = 4
    opt.flag |= 0x8                                                   # -a
    with bw.Context(str(d / "g60k")) as c:
        _assert_sorted_batch(c, c.process_seqs_bam_sorted(*bw.read_fastq(str(d / "se.fq")), opt), want, contigs, "se -a")


def test_sorted_batch_unmapped_and_half_mapped(ctx, small_index, tmp_path):
    """The mixed set of test_unmapped_reads_and_half_mapped_pairs: records without a reference go last, an unmapped read with a mapped
    mate sorts at the mate's position."""
    rnd = random.Random(7)
    fq1, fq2, g1, g2 = (str(tmp_path / x) for x in ("u_1.fq", "u_2.fq", "g_1.fq", "g_2.fq"))
    bw.make_reads(small_index["fa"], g1, g2, 1600, 150, 10000, 1000, 300, 317)
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
    _write_fastq(fq1, n1, s1, q1)
    _write_fastq(fq2, n2, s2, q2)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    opt = bw.default_opt()
    opt.n_threads = 4
    want = _oracle_sam(small_index["prefix"], [fq1])
    p = _props(bam_ref.split_records(bam_ref.sam_to_bam_records(want, contigs)))
    assert p["no_ref"] >= 100 and p["contigs"] >= 2 and p["strands"] == 2, p
    _assert_sorted_batch(ctx, ctx.process_seqs_bam_sorted(n1, s1, q1, opt), want, contigs, "unmapped se")
    want = _oracle_sam(small_index["prefix"], [fq1, fq2])
    recs = bam_ref.split_records(bam_ref.sam_to_bam_records(want, contigs))
    p = _props(recs)
    fl = [int.from_bytes(r[18:20], "little") for r in recs]
    assert p["no_ref"] >= 100 and p["contigs"] >= 2 and p["strands"] == 2, p
    assert sum(1 for r, f in zip(recs, fl) if f & 4 and not f & 8 and sref.fields(r)[0] >= 0) >= 300     # unmapped, placed at the mate
    opt.flag |= 0x2
    _assert_sorted_batch(ctx, ctx.process_seqs_bam_sorted(_interleave(n1, n2), _interleave(s1, s2), _interleave(q1, q2), opt), want, contigs, "half-mapped pe")


# ------------------------------------------------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("pe", [False, True])
def test_ties_come_out_in_input_order(ctx, small_index, tmp_path, pe):
    """One read (pair) 300 times under different names among 600 ordinary reads (pairs): all copies share (refID, pos, strand)."""
    g1, g2, fq1, fq2 = (str(tmp_path / x) for x in ("g_1.fq", "g_2.fq", "t_1.fq", "t_2.fq"))
    bw.make_reads(small_index["fa"], g1, g2, 1200, 150, 5000, 500, 0, 419)
    src = [bw.read_fastq(g1), bw.read_fastq(g2)]
    assert len(src[0][0]) == 600
    # the read (pair) to repeat must have one placement: among equally good ones bwa mem picks by a hash of the read's number
    plain = [l.split(b"\t") for l in _oracle_sam(small_index["prefix"], [g1, g2] if pe else [g1]).split(b"\n") if l]
    per_name = collections.defaultdict(list)
    for f in plain:
        per_name[f[0]].append(f)
    unique = [k for k, nm in enumerate(src[0][0]) if len(per_name[nm]) == (2 if pe else 1) and
              all(int(f[4]) == 60 and not int(f[1]) & 4 and not any(t.startswith((b"XA:", b"SA:")) for t in f[11:]) for f in per_name[nm])]
    assert unique, "no uniquely placed read to repeat"
    rep = unique[0]
    out = [([], [], []), ([], [], [])]
    for k in range(600):
        for e in range(2):
            for j in range(3):
                out[e][j].append(src[e][j][k])
            if k % 2 == 0:                                           # a copy of the chosen read (pair) after every other read
                out[e][0].append(b"dup%d" % (k // 2))
                out[e][1].append(src[e][1][rep])
                out[e][2].append(src[e][2][rep])
    _write_fastq(fq1, *out[0])
    _write_fastq(fq2, *out[1])
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = _oracle_sam(small_index["prefix"], [fq1, fq2] if pe else [fq1])
    groups = collections.Counter(sref.fields(r) for r in bam_ref.split_records(bam_ref.sam_to_bam_records(want, contigs)))
    assert max(groups.values()) >= 300, "the expectation holds no tie group of 300"
    opt = bw.default_opt()
    opt.n_threads = 4
    if pe:
        opt.flag |= 0x2
    reads = _pe_reads(fq1, fq2) if pe else bw.read_fastq(fq1)
    recs = _assert_sorted_batch(ctx, ctx.process_seqs_bam_sorted(*reads, opt), want, contigs, "ties")
    top = max(groups, key=groups.get)
    names = [r[36:36 + r[12] - 1] for r in recs if sref.fields(r) == top and r[36:39] == b"dup"]
    assert len(names) >= 300 and names == sorted(names, key=lambda s: int(s[3:])), "the copies are not in input order"


# ------------------------------------------------------------------------------------------------------------ 4. resident pair, hygiene
def test_device_resident_pair_and_format_hygiene(ctx, small_index, tmp_path):
    fq1, fq2 = str(tmp_path / "d_1.fq"), str(tmp_path / "d_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 2000, 150, 10000, 1000, 300, 329)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    for pe in (True, False):
        reads = _pe_reads(fq1, fq2) if pe else bw.read_fastq(fq1)
        n = len(reads[0])
        opt = bw.default_opt()
        opt.n_threads = 4
        if pe:
            opt.flag |= 0x2
        want = ctx.process_seqs_bam_sorted(*reads, opt)
        _assert_sorted_batch(ctx, want, _oracle_sam(small_index["prefix"], [fq1, fq2] if pe else [fq1]), contigs, "host entry")
        with bw.Context(small_index["prefix"]) as c:
            arr, keep = bw.seq_array(*reads)
            sam = c.process_seqs_text_array(arr, n, opt)           # makes the batch resident
            ms = c.batch_run_bam_sorted(opt)
            assert ms["k_sam_size"] > 0 and ms["k_sam_write"] > 0 and ms["sort_gather"] > 0 and 1 <= ms["sort_passes"] <= 8
            rec, keys, off = c.batch_bam_sorted()
            assert rec == want[0] and np.array_equal(keys, want[1]) and np.array_equal(off, want[2])
            c.batch_run_bam(opt)                                    # the unsorted format of the same resident batch is untouched
            unsorted = c.batch_bam()
            assert sref.sorted_bytes(unsorted) == rec
        # the sorted call leaves nothing behind: BAM and SAM on the same context == a fresh context's
        arr, keep = bw.seq_array(*reads)
        got_bam = ctx.process_seqs_bam_array(arr, n, opt)
        arr, keep = bw.seq_array(*reads)
        got_sam = ctx.process_seqs_text_array(arr, n, opt)
        with bw.Context(small_index["prefix"]) as fresh:
            arr, keep = bw.seq_array(*reads)
            assert got_bam == fresh.process_seqs_bam_array(arr, n, opt) == unsorted
            arr, keep = bw.seq_array(*reads)
            assert got_sam == fresh.process_seqs_text_array(arr, n, opt) == sam


# ------------------------------------------------------------------------------------------------------------ 5. the stream driver
K = 600 * 150
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"


@pytest.fixture(scope="module")
def stream_case(small_index, tmp_path_factory):
    """4300 pairs, their oracle SAM with -K (8 batches paired, 4 single-end) and the expected sorted records of both."""
    d = tmp_path_factory.mktemp("sorted_stream")
    fq1, fq2 = str(d / "s_1.fq"), str(d / "s_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 4300, 150, 10000, 2000, 500, 171)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = {}
    for pe in (True, False):
        recs = bam_ref.split_records(bam_ref.sam_to_bam_records(_oracle_sam(small_index["prefix"], [fq1, fq2] if pe else [fq1], ["-K", str(K)]), contigs))
        want[pe] = (len(recs), b"".join(sref.stable_sort(recs)))
    return dict(fq1=fq1, fq2=fq2, want=want, files={})


@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("n_ctx", [1, 2, 3])
def test_stream_driver_files_to_sorted_bam(small_index, stream_case, tmp_path, n_ctx, pe):
    a, b = stream_case["fq1"], stream_case["fq2"] if pe else None
    n_rec, want_recs = stream_case["want"][pe]
    spill = tmp_path / "spill"
    spill.mkdir()
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            want = bw.bam_header_sorted(c0, HDR) + want_recs
            n_batches = 8 if pe else 4
            opt = bw.default_opt()
            opt.n_threads = 4
            for budget in (0, int(1.5 * (len(want_recs) + 16 * n_rec) / n_batches), 1 << 30):
                for level in (0, 1):
                    out = str(tmp_path / "out.bam")
                    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                    try:
                        st, so = bw.stream_run_bam_sorted(ctxs, a, b, fd, HDR, level, opt, chunk_bases=K, reader_threads=2, tmp_dir=str(spill), mem_budget=budget)
                    finally:
                        os.close(fd)
                    got = open(out, "rb").read()
                    what = f"n_ctx {n_ctx}, budget {budget}, level {level}, {'pe' if pe else 'se'}"
                    assert got.endswith(BGZF_EOF), what
                    assert gzip.decompress(got) == want, what
                    assert stream_case["files"].setdefault((pe, level), got) == got, what + ": the file differs from another combination's"
                    assert st.n_batches == n_batches and st.n_reads == (4300 if pe else 2150) and st.sam_bytes == len(want_recs), what
                    assert so.n_runs == n_batches and so.n_records == n_rec and so.merge_s > 0 and so.sort_ms > 0, what
                    if budget == 0:
                        assert so.spilled_bytes == len(want_recs) + 16 * n_rec + 8 * n_batches, what
                    elif budget == 1 << 30:
                        assert so.spilled_bytes == 0, what
                    else:
                        assert 0 < so.spilled_bytes < len(want_recs) + 16 * n_rec + 8 * n_batches, what
                    assert os.listdir(spill) == [], what
                    assert len(got) > 3 * 65536 if level == 0 else len(got) < len(want) // 2
        finally:
            for c in ctxs[1:]:
                c.close()


def test_stream_driver_dropped_output_and_unusable_tmp_dir(small_index, stream_case, tmp_path):
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0, c0.clone_on(0)]
        try:
            opt = bw.default_opt()
            opt.n_threads = 4
            a, b = stream_case["fq1"], stream_case["fq2"]
            st, so = bw.stream_run_bam_sorted(ctxs, a, b, -1, None, 1, opt, chunk_bases=K, max_reads=1000, tmp_dir=str(tmp_path), mem_budget=0)   # produced and dropped
            assert st.n_reads == 1200 and st.n_batches == 2 and so.n_runs == 2 and so.n_records >= 1200 and so.spilled_bytes > 0
            assert os.listdir(tmp_path) == []
            with pytest.raises(bw.BwahipError, match="EIO"):
                bw.stream_run_bam_sorted(ctxs, a, b, -1, None, 1, opt, chunk_bases=K, tmp_dir=str(tmp_path / "nowhere"), mem_budget=0)
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                bw.stream_run_bam_sorted(ctxs, a, b, -1, "@HD\tVN:1.6\tSO:unsorted", 1, opt, chunk_bases=K, tmp_dir=str(tmp_path))
            out = str(tmp_path / "after.bam")                        # the contexts still work
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                bw.stream_run_bam_sorted(ctxs, a, b, fd, HDR, 1, opt, chunk_bases=K, tmp_dir=str(tmp_path), mem_budget=0)
            finally:
                os.close(fd)
            assert gzip.decompress(open(out, "rb").read()) == bw.bam_header_sorted(c0, HDR) + stream_case["want"][True][1]
        finally:
            ctxs[1].close()
