"""The BGZF blocks of the BAM output deflated and checksummed on the GPU (csrc/k_bgzf.hip).  Expected bytes never come from the code
under test: the judges are Python's zlib and tests/bgzf_ref.py (a member parser written from the SAM specification, 4.1); the records
inside the members are pinned through tests/bam_ref.py to SAM the reference side produced, as in test_gpu_bam.py."""
import gzip
import math
import os
import random
import struct
import subprocess
import zlib

import pytest

import bam_ref
import bgzf_ref
import common
from common import bw

pytestmark = pytest.mark.gpu

B = bgzf_ref.BLOCK_IN


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden(built, tmp_path_factory):
    """The 60 kb golden genome and the golden reads (as test_gpu_bam.py unpacks them)."""
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


# ---- known answers -----------------------------------------------------------------------------------------------------------------
def _text(n, seed):
    """Text-like bytes: words of a small vocabulary with separators, so matches of many lengths and distances."""
    rnd = random.Random(seed)
    words = [bytes(rnd.choice(b"ACGTNacgtn0123456789:=_\tIFJ#") for _ in range(rnd.randint(2, 14))) for _ in range(80)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words)
        if rnd.random() < 0.1:
            out += bytes([rnd.randrange(256)])
    return bytes(out[:n])


def _skewed(n, n_sym, ratio, seed):
    rnd = random.Random(seed)
    w = [ratio ** k for k in range(n_sym)]
    return bytes(rnd.choices(range(33, 33 + n_sym), weights=w, k=n))


def _fibonacci_counts(seed):
    """Symbol k occurs fib(k) times (23 symbols, 46 367 bytes, shuffled): a Huffman tree over these counts alone is 22 levels deep."""
    f, out = [1, 1], bytearray()
    while len(f) < 23:
        f.append(f[-1] + f[-2])
    for k, c in enumerate(f):
        out += bytes([65 + k]) * c
    lst = list(out)
    random.Random(seed).shuffle(lst)
    return bytes(lst)


def _kat_inputs():
    rnd = random.Random(20240607)
    half = bytes(rnd.randrange(256) for _ in range(32768))
    per = bytes(rnd.randrange(256) for _ in range(32769))
    perm = list(range(256))
    rnd.shuffle(perm)
    inputs = {f"text_{n}": _text(n, 100 + i) for i, n in enumerate([0, 1, 3, 4, 5, B - 1, B, B + 1, 2 * B, 3 * B + 7])}
    inputs.update({
        "zeros": bytes(B),
        "random": bytes(rnd.randrange(256) for _ in range(B)),
        "each_value_once": bytes(perm) + bytes(range(43, -1, -1)),       # 300 bytes, no 4 bytes occur twice: no match, no distance code
        "one_match": bytes(range(256)) + bytes(range(100, 144)),          # 300 bytes, one match: a single distance code
        "distance_32768": half + half,
        "period_32769": per + per,
        "pattern4_x_17500": b"\x01\xfe\x37\x80" * 17500,                  # 70 000 bytes: the run crosses the cut at 65 280
        "two_symbols": bytes(rnd.choice(b"ab") for _ in range(200000)),
        "forty_symbols_geometric": _skewed(200000, 40, 0.45, 9),
        "fibonacci_counts": _fibonacci_counts(3),
    })
    return inputs


@pytest.fixture(scope="module")
def kat(ctx):
    """Every known-answer input through bwahip_kat_bgzf, twice: name -> (input, first call, second call).  Computed once."""
    out = {}
    for name, data in _kat_inputs().items():
        out[name] = (data, ctx.kat_bgzf(data), ctx.kat_bgzf(data))
    return out


KAT_NAMES = sorted(_kat_inputs())


@pytest.mark.parametrize("name", KAT_NAMES)
def test_known_answers(kat, name):
    """The members inflate to the input, cut at 65 280; ISIZE, CRC32, BSIZE and the size bound hold for every member; two calls agree."""
    data, (got, nb, ns), second = kat[name]
    assert second == (got, nb, ns), "two calls gave different bytes"
    want = bgzf_ref.blocks_of(data)
    assert nb == len(want) == math.ceil(len(data) / B)
    ms = bgzf_ref.parse(got)                                       # header fields, BSIZE, inflate to the end with nothing left, CRC32, ISIZE
    assert len(ms) == nb
    pos = 0
    for i, (m, w) in enumerate(zip(ms, want)):
        assert m["data"] == w, f"member {i} inflates to other bytes"
        assert m["size"] <= 65536
        crc, isize = struct.unpack_from("<II", got, pos + m["size"] - 8)
        assert isize == len(w) and crc == zlib.crc32(w), f"member {i}: trailer"
        assert m["btype"] in (0, 2)
        assert m["size"] <= len(w) + 5 + 26, f"member {i} is larger than its stored form"
        pos += m["size"]
    assert ns == sum(1 for m in ms if m["btype"] == 0)
    if len(data) == 0:
        assert got == b"" and nb == 0 and ns == 0


def test_random_bytes_leave_stored(kat):
    data, (got, nb, ns), _ = kat["random"]
    ms = bgzf_ref.parse(got)
    assert nb == ns == 1 and ms[0]["btype"] == 0 and ms[0]["size"] == 65280 + 5 + 26
    assert got[18:23] == bytes([1, 0x00, 0xff, 0xff, 0x00]) and got[23:23 + 65280] == data


def test_matches_and_codes_do_their_work(kat):
    """Bounds from the inputs themselves, not from what the code gives.  zeros: 65 279 bytes behind the first are covered by 254
    matches of at most 258 at distance 1 -- a few bits each -- plus a code description: a few hundred bytes at the most.  The repeated half
    and the 4-byte pattern are matches throughout from the first repeat on, so well below a quarter.  Two symbols hold at most one bit
    per byte, forty symbols with ratio 0.45 hold -sum p log2 p = 1.81 bits per byte: Huffman codes alone reach within a bit of that."""
    z = bgzf_ref.parse(kat["zeros"][1][0])
    assert z[0]["btype"] == 2 and z[0]["size"] < 600
    d = bgzf_ref.parse(kat["distance_32768"][1][0])
    assert d[0]["btype"] == 2 and d[0]["deflate_len"] < 32768 + 5 + 32512 // 4          # the first half cannot compress, the second is matches
    p = bgzf_ref.parse(kat["pattern4_x_17500"][1][0])
    assert [m["btype"] for m in p] == [2, 2] and p[0]["size"] < 65280 // 4 and p[1]["size"] < 4720 // 4
    for name, bits in (("two_symbols", 2.0), ("forty_symbols_geometric", 2.81), ("fibonacci_counts", 4.0)):
        data, (got, nb, ns), _ = kat[name]
        ms = bgzf_ref.parse(got)
        assert ns == 0 and sum(m["deflate_len"] for m in ms) < len(data) * bits / 8 + 200 * nb, name
    one = bgzf_ref.parse(kat["one_match"][1][0])
    none = bgzf_ref.parse(kat["each_value_once"][1][0])
    assert one[0]["data"] == kat["one_match"][0] and none[0]["data"] == kat["each_value_once"][0]


def test_period_32769_finds_no_match_across_it(kat):
    """The only repeats lie 32 769 back, one more than a distance can say: random bytes, so the block leaves stored (or at least no smaller
    than Huffman coding of random bytes allows) -- and inflates correctly, which test_known_answers checked."""
    data, (got, nb, ns), _ = kat["period_32769"]
    ms = bgzf_ref.parse(got)
    assert nb == 2 and ms[0]["size"] >= 65280                       # no 32 512-byte match run was taken in the first block
    assert ms[0]["data"] + ms[1]["data"] == data


# ---- compression does something ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pe", "se", "opt_W0_long"])
def test_golden_records_compress_below_zlib_huffman_only_and_fixed(ctx, golden, name, capsys):
    """The BAM records of the committed golden SAM: the summed deflate payload is below zlib's Z_HUFFMAN_ONLY and below zlib level 1 with
    Z_FIXED on the same blocks, and no member is stored."""
    contigs = bam_ref.contig_names_of(golden["prefix"])
    rec = bam_ref.sam_to_bam_records(gzip.open(os.path.join(common.GOLDEN, name + ".sam.gz")).read(), contigs)
    blocks = bgzf_ref.blocks_of(rec)
    assert len(blocks) == 2
    got, nb, ns = ctx.kat_bgzf(rec)
    ms = bgzf_ref.parse(got)
    assert [m["data"] for m in ms] == blocks
    ours = sum(m["deflate_len"] for m in ms)
    huff = sum(bgzf_ref.zlib_deflate_len(b, 1, zlib.Z_HUFFMAN_ONLY) for b in blocks)
    fixed = sum(bgzf_ref.zlib_deflate_len(b, 1, zlib.Z_FIXED) for b in blocks)
    l1 = sum(bgzf_ref.zlib_deflate_len(b, 1) for b in blocks)
    l6 = sum(bgzf_ref.zlib_deflate_len(b, 6) for b in blocks)
    with capsys.disabled():
        print(f"\n[bgzf] {name}: {len(rec)} bytes -> GPU {ours}, zlib Huffman-only {huff}, Z_FIXED level 1 {fixed}, level 1 {l1}, level 6 {l6}; GPU / level 1 = {ours / l1:.3f}")
    assert ns == 0 and all(m["btype"] == 2 for m in ms), "a member of compressible records was stored"
    assert ours < huff, f"{ours} bytes, Huffman-only {huff}"
    assert ours < fixed, f"{ours} bytes, Z_FIXED level 1 {fixed}"


# ---- bwahip_process_seqs_bgzf ---------------------------------------------------------------------------------------------------------------
def _check_batch(c, reads, opt, want_sam, contigs, what, pes0=None):
    members, raw_len, n_blocks = c.process_seqs_bgzf(*reads, opt, pes0=pes0)
    ms = bgzf_ref.parse(members)
    rec = b"".join(m["data"] for m in ms)
    assert rec == c.process_seqs_bam(*reads, opt, pes0=pes0), f"{what}: the members do not hold the records of process_seqs_bam"
    if want_sam is not None:
        assert rec == bam_ref.sam_to_bam_records(want_sam, contigs), f"{what}: the members do not hold the reference's records"
    assert raw_len == len(rec) and n_blocks == len(ms) == math.ceil(raw_len / B)
    assert [len(m["data"]) for m in ms] == [len(b) for b in bgzf_ref.blocks_of(rec)]
    assert members == c.process_seqs_bgzf(*reads, opt, pes0=pes0)[0], f"{what}: a second call gave other bytes"
    return members


def test_golden_reads_as_bgzf(golden):
    G, d = common.GOLDEN, golden["dir"]
    contigs = bam_ref.contig_names_of(golden["prefix"])
    se = bw.read_fastq(os.path.join(d, "se.fq"))
    pe = _pe_reads(os.path.join(d, "pe_1.fq"), os.path.join(d, "pe_2.fq"))
    with bw.Context(golden["prefix"]) as c:
        opt = bw.default_opt()
        opt.n_threads = 4
        _check_batch(c, se, opt, gzip.open(os.path.join(G, "se.sam.gz")).read(), contigs, "se")
        opt.flag |= 0x2
        _check_batch(c, pe, opt, gzip.open(os.path.join(G, "pe.sam.gz")).read(), contigs, "pe")


@pytest.fixture(scope="module")
def generated(small_index, tmp_path_factory):
    """3 000 x 150 bp paired reads with indels, N's and chimeras, and the oracle's SAM for them."""
    d = tmp_path_factory.mktemp("gen")
    fq1, fq2 = str(d / "r_1.fq"), str(d / "r_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 3000, 150, 20000, 3000, 1000, 311, 30000)
    return {"fq1": fq1, "fq2": fq2, "reads": _pe_reads(fq1, fq2), "sam": _oracle_sam(small_index["prefix"], [fq1, fq2])}


def test_generated_pairs_as_bgzf_and_the_resident_pair(ctx, small_index, generated):
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    opt = bw.default_opt()
    opt.n_threads = 8
    opt.flag |= 0x2
    reads = generated["reads"]
    members = _check_batch(ctx, reads, opt, generated["sam"], contigs, "generated pe")
    assert len(bgzf_ref.parse(members)) >= 10                       # about 1 MB of records
    # the device-resident pair: the batch is made resident by a SAM call on a second context, then finalised as BGZF there
    with bw.Context(small_index["prefix"]) as c:
        arr, keep = bw.seq_array(*reads)
        c.process_seqs_text_array(arr, len(reads[0]), opt)
        ms = c.batch_run_bgzf(opt)
        assert ms["deflate"] > 0 and ms["k_sam_write"] > 0
        data, raw_len, n_blocks, n_stored = c.batch_bgzf()
        assert data == members and raw_len == len(bgzf_ref.inflate(members)) and n_blocks == len(bgzf_ref.parse(members)) and n_stored == 0
        c.batch_run_bam(opt)                                          # and the plain records of the same resident batch afterwards
        assert c.batch_bam() == bgzf_ref.inflate(members)


def test_a_name_of_255_bytes_is_refused(ctx, generated):
    names, seqs, quals = (list(x[:200]) for x in generated["reads"])
    opt = bw.default_opt()
    opt.n_threads = 4
    opt.flag |= 0x2
    names[4] = names[5] = b"n" * 255
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        ctx.process_seqs_bgzf(names, seqs, quals, opt)
    names[4] = names[5] = b"n" * 254
    members, raw_len, n_blocks = ctx.process_seqs_bgzf(names, seqs, quals, opt)
    assert bgzf_ref.inflate(members) == ctx.process_seqs_bam(names, seqs, quals, opt)


# ---- bwahip_stream_run_bam_dev ----------------------------------------------------------------------------------------------------------
def _to_file(path, fn):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        r = fn(fd)
    finally:
        os.close(fd)
    return r, open(path, "rb").read()


def test_stream_driver_writes_device_made_blocks(small_index, generated, tmp_path):
    """header member | the batches' members in input order | EOF block; the same content as the host level-1 stream; the same bytes over
    one and three contexts; the counters agree with the file."""
    fq1, fq2 = generated["fq1"], generated["fq2"]
    K = 500 * 150                                                   # 6 batches of 500 reads
    hdr = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0, c0.clone_on(0), c0.clone_on(0)]
        try:
            opt = bw.default_opt()
            opt.n_threads = 4
            _, hdr_member = _to_file(str(tmp_path / "hdr.bgzf"), lambda fd: bw.bgzf_write(fd, bw.bam_header(c0, hdr), 1, 1))
            (st1, bs1), one = _to_file(str(tmp_path / "one.bam"), lambda fd: bw.stream_run_bam_dev(ctxs[:1], fq1, fq2, fd, hdr, opt, chunk_bases=K, reader_threads=2))
            (st3, bs3), three = _to_file(str(tmp_path / "three.bam"), lambda fd: bw.stream_run_bam_dev(ctxs, fq1, fq2, fd, hdr, opt, chunk_bases=K, reader_threads=2))
            st_h, host = _to_file(str(tmp_path / "host.bam"), lambda fd: bw.stream_run_bam(ctxs, fq1, fq2, fd, hdr, 1, opt, chunk_bases=K, reader_threads=2))
            assert one == three, "the file depends on the number of contexts"
            assert one.startswith(hdr_member) and one.endswith(bgzf_ref.EOF_BLOCK)
            ms = bgzf_ref.parse(one)
            assert ms[-1]["data"] == b"" and all(len(m["data"]) > 0 for m in ms[:-1])
            assert bgzf_ref.inflate(one) == gzip.decompress(host)
            want = _oracle_sam(small_index["prefix"], [fq1, fq2], ["-K", str(K)])        # the batches cut as the driver cuts them
            assert bgzf_ref.inflate(one) == bw.bam_header(c0, hdr) + bam_ref.sam_to_bam_records(want, bam_ref.contig_names_of(small_index["prefix"]))
            for st, bs in ((st1, bs1), (st3, bs3)):
                assert st.n_batches == 6 and st.n_reads == 3000
                assert bs.raw_bytes == st.sam_bytes == st_h.sam_bytes
                assert bs.bgzf_bytes == len(one) - len(hdr_member) - 28
                assert bs.n_blocks == len(ms) - 2 and bs.n_stored == 0 and bs.deflate_ms > 0
            st, bs = bw.stream_run_bam_dev(ctxs, fq1, fq2, -1, hdr, opt, chunk_bases=K, reader_threads=2)          # produced and dropped
            assert (st.n_reads, st.n_batches, st.sam_bytes, bs.raw_bytes, bs.bgzf_bytes, bs.n_blocks) == (3000, 6, st1.sam_bytes, bs1.raw_bytes, bs1.bgzf_bytes, bs1.n_blocks)
            empty = str(tmp_path / "empty.fq")
            open(empty, "w").close()
            (st, bs), got = _to_file(str(tmp_path / "empty.bam"), lambda fd: bw.stream_run_bam_dev(ctxs, empty, None, fd, hdr, opt, chunk_bases=K))
            assert got == hdr_member + bgzf_ref.EOF_BLOCK and st.n_reads == 0 and bs.n_blocks == 0 and bs.bgzf_bytes == 0
        finally:
            for c in ctxs[1:]:
                c.close()
