"""bwahip_stream_run as a three-stage pipeline per context (stage-in of batch k+1, kernels of batch k, stage-out of batch k-1, two
sets of input and of output buffers): the shapes at which such a pipeline can go wrong, every one against the oracle's `mem -K` output."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import common
from common import bw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(prefix, fqs, K, extra=()):
    return subprocess.run([common.ORACLE, "mem", "-t", "4", "-K", str(K), *extra, prefix, *fqs], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout


def _records(fq):
    """the four-line records of a FASTQ file"""
    lines = open(fq, "rb").read().split(b"\n")
    return [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]


def _write(fq, recs):
    with open(fq, "wb") as f:
        for r in recs:
            f.write(b"\n".join(r) + b"\n")


def _cuts(lens, K, pe=False):
    """reads per batch as bseq_read (bwa.c:191) cuts them: a batch ends once it holds K bases (paired: at an even read)"""
    out, n, size = [], 0, 0
    for l in lens:
        n += 1
        size += l
        if size >= K and (not pe or n % 2 == 0):
            out.append(n)
            n = size = 0
    return out + ([n] if n else [])


def _contexts(c0, n):
    return [c0] + [c0.clone_on(0) for _ in range(n - 1)]


def _stream(ctxs, fq1, fq2, path, K, **kw):
    opt = bw.default_opt()
    opt.n_threads = 4
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        st = bw.stream_run(ctxs, fq1, fq2, fd, opt, chunk_bases=K, reader_threads=2, **kw)
    finally:
        os.close(fd)
    return st, open(path, "rb").read()


@pytest.fixture(scope="module")
def ctx3(small_index):
    """three contexts on the one GPU, kept for the whole file: every test also runs on what the tests before it left behind"""
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = _contexts(c0, 3)
        try:
            yield ctxs
        finally:
            for c in ctxs[1:]:
                c.close()


K_PE = 200 * 150


@pytest.fixture(scope="module")
def pe_inputs(small_index, tmp_path_factory):
    """paired 2 x 150 inputs of 1, 2, 3 and 7 batches of -K 200 * 150 (the last batch of the longest holds one pair), with the oracle's SAM"""
    d = tmp_path_factory.mktemp("pipe_pe")
    fq1, fq2 = str(d / "all_1.fq"), str(d / "all_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 1202, 150, 10000, 2000, 500, 611, 20000)
    r1, r2 = _records(fq1), _records(fq2)
    assert len(r1) == len(r2) == 601
    out = {}
    for n_batches, pairs in ((1, 100), (2, 200), (3, 300), (7, 601)):
        a, b = str(d / f"b{n_batches}_1.fq"), str(d / f"b{n_batches}_2.fq")
        _write(a, r1[:pairs]); _write(b, r2[:pairs])
        cuts = _cuts([len(x[1]) for p in zip(r1[:pairs], r2[:pairs]) for x in p], K_PE, pe=True)
        assert len(cuts) == n_batches and (n_batches != 7 or cuts[-1] == 2), cuts
        out[n_batches] = (a, b, 2 * pairs, _oracle(small_index["prefix"], [a, b], K_PE))
    return out


@pytest.mark.parametrize("n_ctx", [1, 2, 3])
@pytest.mark.parametrize("n_batches", [1, 2, 3, 7])
def test_fewer_batches_than_stages_and_more(ctx3, pe_inputs, tmp_path, n_batches, n_ctx):
    a, b, n_reads, want = pe_inputs[n_batches]
    st, got = _stream(ctx3[:n_ctx], a, b, str(tmp_path / "o.sam"), K_PE)
    assert got == want
    assert st.n_reads == n_reads and st.n_batches == n_batches and st.sam_bytes == len(want)


@pytest.mark.parametrize("n_ctx", [1, 2])
def test_buffers_grow_while_a_neighbour_batch_is_in_flight(small_index, tmp_path, n_ctx):
    """Single end: 100 bp reads, then noisy 250 bp reads (5 % substitutions, indels, chimeras) with long names.  With -K in bases the later
    batches hold more bases per read, more seeds and regions per base and -- checked below -- more SAM text than any batch before them,
    so the sets and the working set are reallocated while the neighbouring stages hold theirs.  Fresh contexts: nothing is grown yet."""
    fa, fb, fq = str(tmp_path / "a.fq"), str(tmp_path / "b.fq"), str(tmp_path / "ab.fq")
    bw.make_reads(small_index["fa"], fa, None, 900, 100, 1000, 0, 0, 621, 0)
    bw.make_reads(small_index["fa"], fb, None, 600, 250, 50000, 5000, 500, 623, 50000)
    rb = _records(fb)
    for k, r in enumerate(rb):
        r[0] += b"_" + b"long_name_%d_" % k * 20
    recs = _records(fa) + rb
    _write(fq, recs)
    K = 300 * 100
    cuts = _cuts([len(r[1]) for r in recs], K)
    want = _oracle(small_index["prefix"], [fq], K)
    # SAM bytes per batch, from the oracle's text: records of read i start with its name
    per_read = {}
    for line in want.split(b"\n")[:-1]:
        nm = line.split(b"\t", 1)[0]
        per_read[nm] = per_read.get(nm, 0) + len(line) + 1
    sizes, i = [], 0
    for n in cuts:
        sizes.append(sum(per_read[r[0][1:].split()[0]] for r in recs[i:i + n]))
        i += n
    assert len(cuts) >= 6 and max(sizes[:3]) * 1.2 < min(sizes[4:-1]), sizes
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = _contexts(c0, n_ctx)
        try:
            st, got = _stream(ctxs, fq, None, str(tmp_path / "o.sam"), K)
        finally:
            for c in ctxs[1:]:
                c.close()
    assert got == want
    assert st.n_batches == len(cuts) and st.n_reads == len(recs)


@pytest.mark.parametrize("n_ctx", [1, 2])
def test_comments_appear_and_disappear(ctx3, small_index, tmp_path, n_ctx):
    """-C with comments in batches 1-3 of 5 only: the comment buffer of a context is there for one batch and gone for the next"""
    fq = str(tmp_path / "c.fq")
    bw.make_reads(small_index["fa"], fq, None, 1000, 150, 10000, 2000, 500, 631, 20000)
    recs = _records(fq)
    K = 200 * 150
    cuts = _cuts([len(r[1]) for r in recs], K)
    assert len(cuts) == 5
    for k in range(cuts[0], sum(cuts[:4])):
        if k % 3:
            recs[k][0] += b" BC:Z:" + b"ACGT"[k % 4:k % 4 + 1] * 6 + b"\tXY:i:%d" % k
    _write(fq, recs)
    want = _oracle(small_index["prefix"], [fq], K, ["-C"])
    assert b"\tBC:Z:" in want
    st, got = _stream(ctx3[:n_ctx], fq, None, str(tmp_path / "o.sam"), K, keep_comments=True)
    assert got == want
    assert st.n_batches == 5


CHILD = textwrap.dedent('''
    import os, sys
    root, prefix, n_ctx, bad, good, K, out = sys.argv[1:8]
    sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
    from common import bw
    opt = bw.default_opt(); opt.n_threads = 4
    with bw.Context(prefix) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(int(n_ctx) - 1)]
        try:
            bw.stream_run(ctxs, bad, None, -1, opt, chunk_bases=int(K), reader_threads=2)
            print("NO_ERROR", flush=True)
        except bw.BwahipError as e:
            print("RAISED", e, flush=True)
        fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        st = bw.stream_run(ctxs, good, None, fd, opt, chunk_bases=int(K), reader_threads=2)
        os.close(fd)
        print("GOOD", st.n_reads, st.n_batches, flush=True)
        for c in ctxs[1:]:
            c.close()
''')


@pytest.mark.parametrize("n_ctx", [1, 3])
def test_a_failure_in_the_middle_ends_the_pass_and_leaves_the_contexts_usable(small_index, tmp_path, n_ctx):
    """Batch 3 of 6 holds a read of 701 bases: refused by the length check on the host, before any launch of that batch, while its
    neighbours are in flight.  In a child process with a time limit of its own: the pass must end with ECAPACITY, not hang, and
    the same contexts then align the good input byte for byte."""
    good, bad = str(tmp_path / "good.fq"), str(tmp_path / "bad.fq")
    bw.make_reads(small_index["fa"], good, None, 1200, 150, 10000, 2000, 500, 641, 20000)
    recs = _records(good)
    K = 200 * 150
    assert len(_cuts([len(r[1]) for r in recs], K)) == 6
    long_read = [list(r) for r in recs]
    long_read[3 * 200 + 57][1] = (recs[0][1] * 5)[:701]
    long_read[3 * 200 + 57][3] = b"I" * 701
    _write(bad, long_read)
    want = _oracle(small_index["prefix"], [good], K)
    out = str(tmp_path / "o.sam")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, small_index["prefix"], str(n_ctx), bad, good, str(K), out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "RAISED" in r.stdout and "ECAPACITY" in r.stdout, r.stdout
    assert "GOOD 1200 6" in r.stdout
    assert open(out, "rb").read() == want


def test_no_state_leaks_out_of_the_stream(ctx3, pe_inputs, small_index, tmp_path):
    """After a stream pass bwahip_process_seqs_text on the same context gives what a fresh context gives, and its text keeps the
    documented lifetime: the first of two consecutive calls' text is intact after the second (valid until the next-but-one call)."""
    a, b, n_reads, want = pe_inputs[3]
    st, got = _stream(ctx3[:2], a, b, str(tmp_path / "o.sam"), K_PE)
    assert got == want
    opt = bw.default_opt()
    opt.n_threads = 4
    opt.flag |= 0x2

    n1, s1, q1 = bw.read_fastq(a)
    n2, s2, q2 = bw.read_fastq(b)
    names = [x for p in zip(n1, n2) for x in p]; seqs = [x for p in zip(s1, s2) for x in p]; quals = [x for p in zip(q1, q2) for x in p]
    assert len(names) == n_reads

    def batch(lo, hi):
        return names[lo:hi], seqs[lo:hi], quals[lo:hi]
    first, second = batch(0, 200), batch(200, 400)                # the stream's first two batches
    with bw.Context(small_index["prefix"]) as fresh:
        arr, keep = bw.seq_array(*first)
        want1 = fresh.process_seqs_text_array(arr, 200, opt)
        arr, keep = bw.seq_array(*second)
        want2 = fresh.process_seqs_text_array(arr, 200, opt, n_processed=200)
    assert want1 + want2 == want[:len(want1) + len(want2)]
    c = ctx3[0]
    texts = []
    for (names, seqs, quals), n, np0 in ((first, 200, 0), (second, 200, 200)):
        arr, keep = bw.seq_array(names, seqs, quals)
        sam, ln, off = C.c_char_p(), C.c_int64(), C.POINTER(C.c_int64)()
        rc = bw.lib().bwahip_process_seqs_text(c._h, C.byref(opt), np0, n, arr, None, C.byref(sam), C.byref(ln), C.byref(off))
        assert rc == 0
        texts.append((C.cast(sam, C.c_void_p).value, ln.value))
    assert C.string_at(texts[1][0], texts[1][1]) == want2
    assert C.string_at(texts[0][0], texts[0][1]) == want1          # still there after the call that followed it


def test_back_to_back_passes_on_the_same_contexts(ctx3, pe_inputs, small_index, tmp_path):
    """single end, paired end, then BAM (level 0) on the same three contexts without recreating them"""
    import gzip
    import bam_ref
    a, b, n_reads, want_pe = pe_inputs[7]
    want_se = _oracle(small_index["prefix"], [a], K_PE)
    st, got = _stream(ctx3, a, None, str(tmp_path / "se.sam"), K_PE)
    assert got == want_se and st.n_reads == n_reads // 2
    st, got = _stream(ctx3, a, b, str(tmp_path / "pe.sam"), K_PE)
    assert got == want_pe and st.n_reads == n_reads and st.n_batches == 7
    hdr = "@PG\tID:bwahip"
    opt = bw.default_opt()
    opt.n_threads = 4
    out = str(tmp_path / "pe.bam")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        st = bw.stream_run_bam(ctx3, a, b, fd, hdr, 0, opt, chunk_bases=K_PE, reader_threads=2)
    finally:
        os.close(fd)
    want_bam = bw.bam_header(ctx3[0], hdr) + bam_ref.sam_to_bam_records(want_pe, bam_ref.contig_names_of(small_index["prefix"]))
    assert gzip.decompress(open(out, "rb").read()) == want_bam
    assert st.n_batches == 7 and st.n_reads == n_reads


# ---------------------------------------------------------------------------------------------- the context's own batch beside the sets
def _interleaved(fq1, fq2):
    n1, s1, q1 = bw.read_fastq(fq1)
    n2, s2, q2 = bw.read_fastq(fq2)
    return [x for p in zip(n1, n2) for x in p], [x for p in zip(s1, s2) for x in p], [x for p in zip(q1, q2) for x in p]


def _pe_opt():
    opt = bw.default_opt()
    opt.n_threads = 4
    opt.flag |= 0x2
    return opt


K_100 = 100 * 100


@pytest.fixture(scope="module")
def pe100(small_index, tmp_path_factory):
    """300 pairs of 2 x 100: six batches of -K 100 * 100"""
    d = tmp_path_factory.mktemp("pipe_pe100")
    fq1, fq2 = str(d / "h_1.fq"), str(d / "h_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 600, 100, 10000, 2000, 500, 651, 20000)
    assert len(_records(fq1)) == len(_records(fq2)) == 300
    return fq1, fq2


def test_an_uploaded_batch_survives_a_stream_pass(ctx3, pe_inputs, pe100, small_index, tmp_path):
    """200 reads of 2 x 150 made resident in a context's own buffers (text by a SAM call, bases by bwahip_batch_upload), then stream passes of
    600 reads of 2 x 100 through that context as one of two: bwahip_batch_run_sam / _bam_sorted over the resident batch give the same bytes
    before and after, without a new upload."""
    a, b, n_reads, want = pe_inputs[1]
    names, seqs, quals = _interleaved(a, b)
    assert n_reads == len(names) == 200
    opt = _pe_opt()
    c = ctx3[0]
    arr, keep = bw.seq_array(names, seqs, quals)
    assert c.process_seqs_text_array(arr, 200, opt) == want
    c.batch_upload(*bw.pack_reads(seqs))

    def resident():
        c.batch_run_sam(opt)
        sam = c.batch_sam()
        c.batch_run_bam_sorted(opt)
        return sam, c.batch_bam_sorted()

    def same(x, y):
        assert x[0] == y[0]
        assert x[1][0] == y[1][0] and np.array_equal(x[1][1], y[1][1]) and np.array_equal(x[1][2], y[1][2])
    before = resident()
    assert before[0] == want and len(before[1][1]) > 0 and len(before[1][2]) == len(before[1][1]) + 1 and before[1][2][-1] == len(before[1][0])
    fq1, fq2 = pe100
    st, got = _stream(ctx3[:2], fq1, fq2, str(tmp_path / "o.sam"), K_100)
    assert got == _oracle(small_index["prefix"], [fq1, fq2], K_100) and st.n_batches == 6 and st.n_reads == 600
    same(resident(), before)
    fd = os.open(str(tmp_path / "o.bam"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        st, so = bw.stream_run_bam_sorted(ctx3[:2], fq1, fq2, fd, "@PG\tID:bwahip", 0, opt, chunk_bases=K_100, reader_threads=2)
    finally:
        os.close(fd)
    assert st.n_batches == 6 and st.n_reads == 600
    same(resident(), before)


FORMS = ["text", "bam", "bam_sorted", "bgzf"]


def _one_piece(c, form, reads, np0, opt):
    """One bwahip_process_seqs_<form> call: the (address, bytes) of every buffer it hands out, and the scalars beside them"""
    arr, keep = bw.seq_array(*reads)
    n, L = len(reads[0]), bw.lib()
    ln = C.c_int64()
    if form == "text":
        sam, off = C.c_char_p(), C.POINTER(C.c_int64)()
        rc = L.bwahip_process_seqs_text(c._h, C.byref(opt), np0, n, arr, None, C.byref(sam), C.byref(ln), C.byref(off))
        out = [(C.cast(sam, C.c_void_p).value, ln.value)], ()
    elif form == "bam":
        p, off = C.c_void_p(), C.POINTER(C.c_int64)()
        rc = L.bwahip_process_seqs_bam(c._h, C.byref(opt), np0, n, arr, None, C.byref(p), C.byref(ln), C.byref(off))
        out = [(p.value, ln.value)], ()
    elif form == "bam_sorted":
        p, keys, roff, nr = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        rc = L.bwahip_process_seqs_bam_sorted(c._h, C.byref(opt), np0, n, arr, None, C.byref(p), C.byref(ln), C.byref(keys), C.byref(roff), C.byref(nr))
        out = [(p.value, ln.value), (keys.value, nr.value * 8), (roff.value, (nr.value + 1) * 8)], ()
    else:
        p, raw, nb = C.c_void_p(), C.c_int64(), C.c_int64()
        rc = L.bwahip_process_seqs_bgzf(c._h, C.byref(opt), np0, n, arr, None, C.byref(p), C.byref(ln), C.byref(raw), C.byref(nb))
        out = [(p.value, ln.value)], (raw.value, nb.value)
    assert rc == 0
    return out


def _bytes_at(pieces):
    return [C.string_at(addr, n) for addr, n in pieces]


@pytest.fixture(scope="module")
def two_batches(small_index, pe_inputs):
    """two different batches of 200 reads (2 x 150) and, per output form, what a fresh context hands out for each (copied at once)"""
    a, b, n_reads, _ = pe_inputs[2]
    names, seqs, quals = _interleaved(a, b)
    assert n_reads == len(names) == 400
    batches = [(names[lo:lo + 200], seqs[lo:lo + 200], quals[lo:lo + 200]) for lo in (0, 200)]
    want = {}
    with bw.Context(small_index["prefix"]) as fresh:
        for form in FORMS:
            want[form] = []
            for k, reads in enumerate(batches):
                pieces, scalars = _one_piece(fresh, form, reads, 200 * k, _pe_opt())
                want[form].append((_bytes_at(pieces), scalars))
    return batches, want


@pytest.mark.parametrize("form", FORMS)
def test_one_piece_calls_take_their_buffers_in_turn(ctx3, two_batches, form):
    """Every one-piece form keeps the documented lifetime: after the second of two consecutive calls on different batches the first call's
    bytes still stand at the addresses it returned -- records, and for the sorted form keys and record offsets, which have pinned buffers
    of their own -- and both equal what a fresh context gives."""
    batches, want = two_batches
    opt = _pe_opt()
    first, scalars1 = _one_piece(ctx3[0], form, batches[0], 0, opt)
    second, scalars2 = _one_piece(ctx3[0], form, batches[1], 200, opt)
    assert all(n > 0 for _, n in first + second)
    assert want[form][0][0] != want[form][1][0]
    assert (_bytes_at(second), scalars2) == want[form][1]
    assert (_bytes_at(first), scalars1) == want[form][0]          # still there after the call that followed it


def test_comments_come_and_go_on_the_direct_path(ctx3, pe100, small_index, tmp_path):
    """-C through bwahip_process_seqs_text on one context: a batch with comments, one without, one with -- the comment buffer stays with the
    context and the kernels are told per batch whether it counts.  Each batch against the oracle's SAM of that batch alone."""
    r1, r2 = _records(pe100[0]), _records(pe100[1])
    opt = _pe_opt()
    for k in range(3):
        pairs = range(100 * k, 100 * k + 100)
        cm = [b"BC:Z:" + b"ACGT"[i % 4:i % 4 + 1] * 6 + b"\tXY:i:%d" % i if k != 1 and i % 3 else None for i in pairs]
        a, b = str(tmp_path / f"c{k}_1.fq"), str(tmp_path / f"c{k}_2.fq")
        _write(a, [r1[i] for i in pairs]); _write(b, [r2[i] for i in pairs])
        names, seqs, quals = _interleaved(a, b)
        for path, recs in ((a, r1), (b, r2)):
            _write(path, [[recs[i][0] + (b" " + c if c else b"")] + recs[i][1:] for i, c in zip(pairs, cm)])
        want = _oracle(small_index["prefix"], [a, b], 1 << 30, ["-C"])
        assert (b"\tBC:Z:" in want) == (k != 1)
        arr, keep = bw.seq_array(names, seqs, quals, [c for c in cm for _ in (0, 1)])
        assert ctx3[0].process_seqs_text_array(arr, 200, opt) == want, f"batch {k}"
