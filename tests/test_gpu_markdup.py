"""Duplicate marking on the device (csrc/k_markdup.hip): the batch's descriptor kernel, the decision stage, the marked finish of the device
merger and the stream driver's entry point.  The judge is tests/markdup_ref.py -- plain Python over the records' bytes -- and, for the
decision, also the host restatement bwahip_markdup_decide_host.  Files are compared byte for byte with what the deflate stage alone
(Context.kat_bgzf) makes of the judge's marked records: no tolerance anywhere."""
import gzip
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bai_ref
import bam_ref
import bam_sort_ref as sref
import bgzf_ref
import common
import markdup_cases as cases
import markdup_ref as ref
from common import bw

pytestmark = pytest.mark.gpu

BLOCK = 65280


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def record_sets():
    out = {}
    for paired in (False, True):
        c = cases.record_set(paired)
        cases.assert_record_families(c)
        c["descs"] = cases.judge_descs(c)
        out[paired] = c
    return out


@pytest.fixture(scope="module")
def desc_sets():
    s = cases.desc_sets()
    cases.assert_desc_families(s)
    return s


# ---------------------------------------------------------------------------------------------------------------- 1. the descriptor kernel
def test_kat_dup_desc_equals_the_judge(ctx, record_sets):
    for paired, c in record_sets.items():
        want = cases.as_desc_array(c["descs"])
        got = ctx.kat_dup_desc(c["buf"], c["off"], paired)
        assert got.tobytes() == want.tobytes(), f"paired {paired}: first difference at template {np.nonzero(got != want)[0][:1]}"
        shifted = ctx.kat_dup_desc(b"\x5a" * 13 + c["buf"], c["off"] + 13, paired)       # every record 13 bytes further on
        assert shifted.tobytes() == want.tobytes(), f"paired {paired}, shifted by 13 bytes"
    assert len(ctx.kat_dup_desc(b"", np.zeros(1, dtype=np.int64), False)) == 0
    one = record_sets[False]
    n0 = int(one["off"][1])
    assert ctx.kat_dup_desc(one["buf"][:n0], one["off"][:2], False).tobytes() == cases.as_desc_array(one["descs"][:1]).tobytes()


def test_kat_dup_desc_refusals(ctx, record_sets):
    """The bad read first, then at least 300 KB of ordinary records: even a kernel that read beyond a record would stay inside the
    allocation.  An error code is expected and nothing else."""
    rng = random.Random(4)
    tail = [cases.rec(b"o%d" % k, 0, 100 + k, [(100, cases.M)], 16 * (k & 1), bytes(rng.randrange(2, 42) for _ in range(100))) for k in range(1700)]
    assert sum(map(len, tail)) >= 300000
    good = cases.rec(b"bad", 0, 5000, [(10, cases.M)], 0, b"\x20" * 10)
    patched = lambda at, fmt, v: (lambda b: (struct.pack_into(fmt, b, at, v), bytes(b))[1])(bytearray(good))
    raw = lambda n: struct.pack("<iiiBBHHH", n - 4, 0, 5000, 1, 0, 0, 0, 0) + bytes(n - 20)
    bads = {"block_size below 32": raw(20), "a read of 35 bytes": raw(35), "block_size one too large": patched(0, "<i", len(good) - 3),
            "block_size one too small": patched(0, "<i", len(good) - 5), "bytes after the last record": good + b"\0" * 10,
            "n_cigar_op beyond the record": patched(16, "<H", 60000), "l_read_name beyond the record": patched(12, "<B", 255),
            "l_seq beyond the record": patched(20, "<i", 1 << 30), "l_seq negative": patched(20, "<i", -1), "l_seq one too large": patched(20, "<i", 11),
            "a later record shorter than its fields": good + patched(20, "<i", 500)}      # the primary is whole, the record after it is not
    for what, bad in bads.items():
        for paired in (False, True):
            reads = [bad] + tail[:len(tail) - 1 + (len(tail) & 1)]
            off = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.int64)
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                ctx.kat_dup_desc(b"".join(reads), off, paired)
    with pytest.raises(bw.BwahipError, match="EINVAL"):                                    # an odd number of reads cannot be pairs
        ctx.kat_dup_desc(good, np.array([0, len(good)], dtype=np.int64), True)
    with pytest.raises(bw.BwahipError, match="EINVAL"):                                    # offsets that decrease
        ctx.kat_dup_desc(good + good, np.array([0, 2 * len(good), len(good)], dtype=np.int64), False)
    c = record_sets[True]
    assert ctx.kat_dup_desc(c["buf"], c["off"], True).tobytes() == cases.as_desc_array(c["descs"]).tobytes()   # the context still works


# ---------------------------------------------------------------------------------------------------------------- 2. the decision stage
def test_kat_markdup_equals_the_judge_and_the_host(ctx, desc_sets):
    for name, descs in desc_sets.items():
        a = cases.as_desc_array(descs)
        want, _ = ref.decide(descs)
        got = ctx.kat_markdup(a)
        assert got.tolist() == want, f"{name}: first difference at template {[i for i, (x, y) in enumerate(zip(got.tolist(), want)) if x != y][:1]}"
        assert got.tobytes() == bw.markdup_decide_host(a).tobytes(), name
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        ctx.kat_markdup(cases.as_desc_array([(1, 2, 3, 3)]))


# ---------------------------------------------------------------------------------------------------------------- 3. the merger
def _key(rec):
    return sref.packed_key(rec, cases.N_SEQS, cases.LONGEST)


def _run_of(templates, descs):
    """Consecutive templates -> what add_dup takes: the run's records sorted, keys, offsets, the records' templates, the descriptors."""
    recs = [(x, t) for t, (_, reads) in enumerate(templates) for r in reads for x in r]
    recs.sort(key=lambda p: sref.order_key(p[0]))                                          # stable: ties keep input order
    return (*sref.run_arrays([x for x, _ in recs], _key), np.array([t for _, t in recs], dtype=np.uint32), cases.as_desc_array(descs))


def _cut(case, n_runs, rng):
    n = len(case["templates"])
    b = [0] + (sorted(rng.sample(range(1, n), n_runs - 1)) if n_runs > 1 else []) + [n]
    return [_run_of(case["templates"][b[k]:b[k + 1]], case["descs"][b[k]:b[k + 1]]) for k in range(n_runs)]


def _finish(ctx, runs, order, pb, path, marked):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, pb) as m:
            for k in order:
                (m.add_dup(k, *runs[k]) if marked else m.add(k, *runs[k][:3]))
            res = m.finish_markdup(fd) if marked else (m.finish(fd), None, None)
    finally:
        os.close(fd)
    return open(path, "rb").read(), res


@pytest.fixture(scope="module")
def merge_want(ctx, record_sets):
    out = {}
    for paired, c in record_sets.items():
        unmarked = sref.stable_sort([x for r in c["reads"] for x in r])
        j = ref.mark(unmarked, c["names"], paired)
        assert j["descs"] == c["descs"] and j["stats"][2] > 20 and any(a == b and not struct.unpack_from("<H", a, 18)[0] & 0x4 for a, b in zip(unmarked, j["records"]))
        marked = b"".join(j["records"])
        out[paired] = dict(unmarked=b"".join(unmarked), marked=marked, members=ctx.kat_bgzf(marked)[0], judge=j, n_rec=len(unmarked))
    return out


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n_runs", [1, 3, 7])
def test_marked_finish_equals_the_judge_for_every_cut_and_piece_size(ctx, record_sets, merge_want, tmp_path, n_runs, paired):
    rng = random.Random(n_runs)
    c, w = record_sets[paired], merge_want[paired]
    runs = _cut(c, n_runs, rng)
    order = list(range(n_runs))
    rng.shuffle(order)
    plain, _ = _finish(ctx, runs, order, 1, str(tmp_path / "plain.bin"), False)
    assert bgzf_ref.inflate(plain) == w["unmarked"]
    for pb in (1, 0):
        got, (st, _, ms) = _finish(ctx, runs, order, pb, str(tmp_path / "marked.bin"), True)
        what = f"{n_runs} runs added as {order}, piece_blocks {pb}, paired {paired}"
        data = bgzf_ref.inflate(got)
        assert data == w["marked"], what
        assert got == w["members"], what + ": not the deflate stage's members of the marked records"
        a, b = np.frombuffer(data, dtype=np.uint8).copy(), np.frombuffer(w["unmarked"], dtype=np.uint8).copy()
        at = np.cumsum([0] + [len(r) for r in w["judge"]["records"]])[:-1] + 19
        a[at] = b[at] = 0
        assert (a == b).all(), what + ": more than byte 19 of a record differs from the unmarked finish"
        n_kind, n_dup, n_marked = w["judge"]["stats"]
        assert (list(ms.n_templates), list(ms.n_dup_templates), ms.n_marked) == (n_kind, n_dup, n_marked), what
        assert (st.n_records, st.n_runs, st.raw_bytes) == (w["n_rec"], n_runs, len(w["marked"])) and ms.hbm_bytes > 0 and ms.markdup_ms > 0, what


def test_marked_finish_refusals(ctx, record_sets, merge_want, tmp_path):
    c, w = record_sets[True], merge_want[True]
    runs = _cut(c, 3, random.Random(9))
    out = str(tmp_path / "m.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 1) as m:                                                   # a run without descriptors among the others
            m.add_dup(0, *runs[0])
            m.add(1, *runs[1][:3])
            m.add_dup(2, *runs[2])
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                m.finish_markdup(fd)
            assert os.fstat(fd).st_size == 0                                               # before a byte is written
        with bw.DevMerger(ctx, 1) as m:
            m.add_dup(0, *runs[0])
            rec, keys, off, tmpl, desc = runs[1]
            bad = tmpl.copy()
            bad[len(bad) // 2] = len(desc)
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # a template index outside the run's descriptors
                m.add_dup(1, rec, keys, off, bad, desc)
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                m.add_dup(1, rec, keys, off, tmpl, desc[:int(tmpl.max())])
            m.add_dup(1, rec, keys, off, tmpl, desc)                                       # the merger is as before
            m.add_dup(2, *runs[2])
            st, _, ms = m.finish_markdup(fd)
            assert st.n_runs == 3 and ms.n_marked == w["judge"]["stats"][2]
    finally:
        os.close(fd)
    assert open(out, "rb").read() == w["members"]


def test_marked_finish_with_nothing_to_mark(ctx, tmp_path):
    got, (st, _, ms) = _finish(ctx, [], [], 1, str(tmp_path / "e.bin"), True)
    assert got == b"" and st.n_records == 0 and ms.n_marked == 0 and list(ms.n_templates) == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- 4. the stream driver
K = 600 * 150
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"


def _oracle_sam(prefix, fqs, extra=()):
    out = subprocess.run([common.ORACLE, "mem", "-t", "8", *extra, prefix, *fqs], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    return b"".join(l + b"\n" for l in out.split(b"\n") if l and not l.startswith(b"@"))


def stream_input(fa, d):
    """The 4300 reads of test_gpu_bam_devmerge.py::stream_case (2150 pairs, all qualities 'I'), and appended to both files, in this order:
    60 pairs whose second mate is random bases -- the first mate of 30 is the first mate of an earlier pair, of the other 30 a read no pair
    has; 300 copies of earlier pairs under new names with lower, higher and equal qualities; copies of the 60.  Batches are 300 pairs, so
    every copy is in a later batch than its original.  Returns (fq1, fq2, the templates' names in input order)."""
    fq1, fq2, x1, x2 = (os.path.join(d, n) for n in ("s_1.fq", "s_2.fq", "x_1.fq", "x_2.fq"))
    bw.make_reads(fa, fq1, fq2, 4300, 150, 10000, 2000, 500, 171)
    bw.make_reads(fa, x1, x2, 60, 150, 10000, 2000, 500, 172)
    n1, s1, q1 = bw.read_fastq(fq1)
    n2, s2, q2 = bw.read_fastq(fq2)
    _, sx, _ = bw.read_fastq(x1)
    assert len(n1) == 2150 and n1 == n2 and len(sx) == 30
    rng = random.Random(31)
    names, a, b = list(n1), list(zip(s1, q1)), list(zip(s2, q2))
    requal = lambda q, k: (q, bytes([q[0] - 20]) * len(q), q[:-1] + bytes([q[-1] + 1]))[k % 3]   # equal; lower; higher by one
    def add(name, m1, m2):
        names.append(name)
        a.append(m1)
        b.append(m2)
    half = []
    for k in range(60):                                                                    # 2150 .. 2209: batch 7
        first = a[100 + 7 * k] if k < 30 else (sx[k - 30], b"I" * len(sx[k - 30]))
        junk = bytes(rng.choices(b"ACGT", k=150))
        add(b"half%d" % k, first, (junk, b"I" * 150))
        half.append(len(names) - 1)
    for k in range(300):                                                                   # 2210 .. 2509: of pairs in batches 0 .. 6
        o = rng.randrange(0, 2000)
        add(b"copy%d" % k, (a[o][0], requal(a[o][1], k)), (b[o][0], requal(b[o][1], k // 3)))
    for k, o in enumerate(half):                                                           # 2510 .. 2569: batch 8
        add(b"halfcopy%d" % k, (a[o][0], requal(a[o][1], k)), (bytes(rng.choices(b"ACGT", k=150)), b"I" * 150))
    for path, reads in ((fq1, a), (fq2, b)):
        with open(path, "wb") as f:
            for n, (s, q) in zip(names, reads):
                f.write(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n")
    return fq1, fq2, names


@pytest.fixture(scope="module")
def stream_case(small_index, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("markdup_stream"))
    fq1, fq2, names = stream_input(small_index["fa"], d)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = {}
    for pe in (True, False):
        recs = bam_ref.split_records(bam_ref.sam_to_bam_records(_oracle_sam(small_index["prefix"], [fq1, fq2] if pe else [fq1], ["-K", str(K)]), contigs))
        unmarked = sref.stable_sort(recs)
        j = ref.mark(unmarked, names, pe)
        want[pe] = dict(n_rec=len(recs), unmarked=b"".join(unmarked), marked=b"".join(j["records"]), judge=j)
    cl = want[True]["judge"]["classes"]
    assert min(cl["pair"], cl["frag_pair"], cl["frag_frag"]) >= 20, f"the input does not hold 20 templates of every duplicate class: {cl}"   # a condition on the input
    assert want[False]["judge"]["classes"]["frag_frag"] >= 300
    return dict(fq1=fq1, fq2=fq2, names=names, want=want, members={}, bai={})


def _run_marked(ctxs, case, pe, d, with_bai=True, **kw):
    opt = bw.default_opt()
    opt.n_threads = 4
    out, bai = os.path.join(d, "out.bam"), os.path.join(d, "out.bam.bai")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fb = os.open(bai, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if with_bai else -1
    try:
        res = bw.stream_run_bam_sorted_dev_markdup(ctxs, case["fq1"], case["fq2"] if pe else None, fd, fb, HDR, opt, chunk_bases=K, reader_threads=2, **kw)
    finally:
        os.close(fd)
        if with_bai:
            os.close(fb)
    return open(out, "rb").read(), (open(bai, "rb").read() if with_bai else None), res


def _want_file(c0, case, pe, key, d):
    if (pe, key) not in case["members"]:
        case["members"][pe, key] = c0.kat_bgzf(case["want"][pe][key])[0]
    hdr_member = os.path.join(d, "hdr.bin")
    fd = os.open(hdr_member, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    bw.bgzf_write(fd, bw.bam_header_sorted(c0, HDR), 1, 1)
    os.close(fd)
    return open(hdr_member, "rb").read() + case["members"][pe, key] + bgzf_ref.EOF_BLOCK


@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("n_ctx", [1, 3])
def test_stream_driver_marks_duplicates_before_the_deflate(small_index, stream_case, tmp_path, n_ctx, pe):
    w = stream_case["want"][pe]
    n_reads = 5140 if pe else 2570
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            want_file = _want_file(c0, stream_case, pe, "marked", str(tmp_path))
            for pb in (1, 0):
                what = f"n_ctx {n_ctx}, piece_blocks {pb}, {'pe' if pe else 'se'}"
                got, bai, (st, sd, ms) = _run_marked(ctxs, stream_case, pe, str(tmp_path), hbm_budget=8 << 30, piece_blocks=pb)
                assert got == want_file, what + ": not header member + the deflate stage's members of the judge's marked records + EOF"
                if pe not in stream_case["bai"]:                     # the Python judges of the file and of its index, once: every later run must give the same bytes
                    assert gzip.decompress(got) == bw.bam_header_sorted(c0, HDR) + w["marked"], what
                    n_ref, recs, offs, _ = bai_ref.split_file(got)
                    assert bai == bai_ref.from_file(got) and bai_ref.check_semantics(bai, recs, offs, n_ref) > len(recs) // 2, what + ": not the canonical index of the file"
                    stream_case["bai"][pe] = bai
                assert bai == stream_case["bai"][pe], what
                n_kind, n_dup, n_marked = w["judge"]["stats"]
                assert (list(ms.n_templates), list(ms.n_dup_templates), ms.n_marked) == (n_kind, n_dup, n_marked), what
                assert sum(n_kind) == 2570 and n_marked > 300 and ms.hbm_bytes > 0 and ms.markdup_ms > 0, what
                assert st.n_reads == n_reads and sd.fell_back == 0 and (sd.n_records, sd.dev.n_records, sd.dev.raw_bytes) == (w["n_rec"], w["n_rec"], len(w["marked"])), what
        finally:
            for c in ctxs[1:]:
                c.close()


def test_stream_driver_budget_no_index_and_the_unmarked_entry_point(small_index, stream_case, tmp_path):
    w = stream_case["want"][True]
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0, c0.clone_on(0)]
        try:
            with pytest.raises(bw.BwahipError, match="ECAPACITY"):                        # no fall-back: a run that does not fit ends the call
                _run_marked(ctxs, stream_case, True, str(tmp_path), hbm_budget=1)
            need = (bw.bam_devmerge_hbm_need(len(w["marked"]), w["n_rec"], 9, 1024) + bw.bam_devmerge_bai_hbm_need(w["n_rec"], (len(w["marked"]) + BLOCK - 1) // BLOCK, 3, 63))   # 63: the 16 Kbp windows of the three contigs
            with pytest.raises(bw.BwahipError, match="ECAPACITY"):                        # what the unmarked run takes is not enough
                _run_marked(ctxs, stream_case, True, str(tmp_path), hbm_budget=need)
            got, bai, (st, sd, ms) = _run_marked(ctxs, stream_case, True, str(tmp_path), hbm_budget=need + bw.bam_devmerge_markdup_hbm_need(w["n_rec"], 2570))
            assert got == _want_file(c0, stream_case, True, "marked", str(tmp_path)) and bai == stream_case["bai"].get(True, bai) and bai[:4] == b"BAI\1"
            got, bai, _ = _run_marked(ctxs, stream_case, True, str(tmp_path), with_bai=False)   # no index asked for; the default budget
            assert got == _want_file(c0, stream_case, True, "marked", str(tmp_path)) and bai is None
            # the unmarked entry point on the same input still writes the unmarked file
            opt = bw.default_opt()
            opt.n_threads = 4
            out = str(tmp_path / "plain.bam")
            fd, fb = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644), os.open(out + ".bai", os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                _, sd = bw.stream_run_bam_sorted_dev_bai(ctxs, stream_case["fq1"], stream_case["fq2"], fd, fb, HDR, opt, chunk_bases=K, reader_threads=2, hbm_budget=8 << 30)
            finally:
                os.close(fd)
                os.close(fb)
            plain = open(out, "rb").read()
            assert sd.fell_back == 0 and plain == _want_file(c0, stream_case, True, "unmarked", str(tmp_path)) and w["unmarked"] != w["marked"]
            assert not any(struct.unpack_from("<H", r, 18)[0] & 0x400 for r in bam_ref.split_records(w["unmarked"]))
        finally:
            ctxs[1].close()


def test_process_seqs_bam_sorted_dup(ctx, stream_case):
    """One batch through the one-piece entry point: the sorted records are those of the unmarked form, the templates and descriptors are
    the judge's for these records."""
    opt = bw.default_opt()
    opt.n_threads = 4
    opt.flag |= 0x2
    with bw.FastqReader(stream_case["fq1"], stream_case["fq2"]) as rd:
        arr, n = rd.next(K)
        rec, keys, off, tmpl, desc = ctx.process_seqs_bam_sorted_dup_array(arr, n, opt, 0)
        rec2, keys2, off2 = ctx.process_seqs_bam_sorted_array(arr, n, opt, 0)
    assert n == 600 and rec == rec2 and (keys == keys2).all() and (off == off2).all() and len(tmpl) == len(keys) and len(desc) == 300
    recs = bam_ref.split_records(rec)
    names = stream_case["names"][:300]
    j = ref.mark(recs, names, True)
    assert desc.tobytes() == cases.as_desc_array(j["descs"]).tobytes()
    assert [names[t] for t in tmpl.tolist()] == [ref.parse(r)["name"] for r in recs]
