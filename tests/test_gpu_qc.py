"""The QC summary and depth of coverage on the device (csrc/k_qc.hip): the stage alone (Context.kat_qc), the armed device merger and the
stream driver's entry point.  The judge is tests/qc_ref.py -- plain Python over the records' bytes and the contig lengths, written from the
rule in include/bwahip.h.  Every comparison is byte for byte: no tolerance anywhere."""
import gzip
import os
import random
import struct

import numpy as np
import pytest

import bai_ref
import bam_sort_ref as sref
import common
import markdup_cases as mcases
import markdup_ref as mref
import qc_cases as cases
import qc_ref as ref
from common import bw

pytestmark = pytest.mark.gpu

OPTS = [(4, -1, 0), (8, -1, 0), (14, -1, 0), (29, -1, 0), (0, 0, 0), (0, -1, 30)]


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(built):
    c = cases.record_set()
    cases.assert_families(c)
    c["want"] = {o: ref.build(c["records"], c["ref_len"], o) for o in OPTS}
    return c


def _same(got, want, what):
    assert got == want, f"{what}: {ref.first_difference(got, want)}"


# ---------------------------------------------------------------------------------------------------------------- 1. the stage
@pytest.mark.parametrize("opt", OPTS)
def test_kat_qc_equals_the_judge(ctx, case, opt):
    _same(ctx.kat_qc(case["buf"], case["off"], case["ref_len"], opt), case["want"][opt], f"options {opt}")
    if opt[0] == 29:
        assert all(len(r["windows"]) == 1 for r in ref.parse(case["want"][opt])["refs"])


def test_kat_qc_invariances(ctx, case):
    opt = (4, -1, 0)
    want = case["want"][opt]
    recs = list(case["records"])
    random.Random(5).shuffle(recs)
    c = cases.make_case(recs)
    _same(ctx.kat_qc(c["buf"], c["off"], c["ref_len"], opt), want, "shuffled")
    c = cases.make_case(sref.stable_sort(case["records"]))                                # as a sorted file holds them: neighbours share their counters
    _same(ctx.kat_qc(c["buf"], c["off"], c["ref_len"], opt), want, "sorted")
    c = cases.make_case(case["records"], shift=13)
    _same(ctx.kat_qc(c["buf"], c["off"], c["ref_len"], opt), want, "every record 13 bytes further on")
    _same(ctx.kat_qc(case["buf"], case["off"], case["ref_len"], opt), want, "a second call on the same context")
    few = case["records"][:3]
    c = cases.make_case(few)
    _same(ctx.kat_qc(c["buf"], c["off"], c["ref_len"], opt), ref.build(few, c["ref_len"], opt), "three records after thousands: the tables were cleared")


def test_kat_qc_degenerate_inputs(ctx):
    lens = cases.REF_LEN
    for opt in ((), (4, 0, 0)):
        want = ref.build([], lens, opt)
        _same(ctx.kat_qc(b"", np.zeros(1, dtype=np.int64), lens, opt), want, "no record")
        s = ref.parse(want)
        assert s["depth_hist"] == [sum(lens)] + [0] * 255 and not any(map(any, s["count"])) and not any(any(r["windows"]) for r in s["refs"])
    nc = [cases.rec(b"a", -1, -1, [], 0x4), cases.rec(b"b", -1, 5, [(3, cases.M)], 0x4 | 0x200)]
    c = cases.make_case(nc, ref_len=[])
    _same(ctx.kat_qc(c["buf"], c["off"], [], ()), ref.build(nc, [], ()), "no reference at all")
    one = [cases.rec(b"c", 1, 0, [(4, cases.M)])]
    c = cases.make_case(one, ref_len=[0, 5])
    _same(ctx.kat_qc(c["buf"], c["off"], [0, 5], (4, -1, 0)), ref.build(one, [0, 5], (4, -1, 0)), "a reference of no bases")


def test_kat_qc_refusals(ctx, case):
    """The bad record first, then at least 300 KB of ordinary records: even a kernel that read beyond a record would stay inside the
    allocation.  An error code is expected and nothing else; what the rule does not check counts as it is."""
    tail = cases.ordinary(300000)
    assert sum(map(len, tail)) >= 300000
    for what, (bad, refused) in cases.bad_records().items():
        c = cases.make_case([bad] + tail)
        if refused:
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                ctx.kat_qc(c["buf"], c["off"], c["ref_len"], ())
        else:
            _same(ctx.kat_qc(c["buf"], c["off"], c["ref_len"], ()), ref.build(c["records"], c["ref_len"]), what)
    c = cases.make_case(tail[:700] + [cases.bad_records()["a read of 35 bytes"][0]] + tail[700:])   # in a later workgroup
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        ctx.kat_qc(c["buf"], c["off"], c["ref_len"], ())
    for opt in ((3, -1, 0), (30, -1, 0), (-1, -1, 0), (0, 65536, 0), (0, -1, -1), (0, -1, 256)):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.kat_qc(case["buf"], case["off"], case["ref_len"], opt)
    for lens in (case["ref_len"][:-1] + [-1], case["ref_len"][:-1] + [1 << 31]):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.kat_qc(case["buf"], case["off"], lens, ())
    with pytest.raises(bw.BwahipError, match="EINVAL"):                                    # offsets that decrease
        ctx.kat_qc(case["buf"], np.array([0, 100, 50], dtype=np.int64), case["ref_len"], ())
    _same(ctx.kat_qc(case["buf"], case["off"], case["ref_len"], (8, -1, 0)), case["want"][(8, -1, 0)], "the context after the refusals")


# ---------------------------------------------------------------------------------------------------------------- 2. the armed merger
def _finish(ctx, runs, order, path, arm=None, how="finish", with_dup=False, n_ref=0):
    """The members a DevMerger writes for these runs and, when armed with (ref_len, opt), the summary."""
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fq = os.open(path + ".bqc", os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    qs = None
    try:
        with bw.DevMerger(ctx, 1) as m:
            for k in order:
                (m.add_dup(k, *runs[k]) if with_dup else m.add(k, *runs[k][:3]))
            if arm:
                qs = m.set_qc(arm[0], fq, arm[1])
            if how == "finish":
                m.finish(fd)
            elif how == "bai":
                m.finish_bai(fd, -1, 0, n_ref)
            else:
                m.finish_markdup(fd)
    finally:
        os.close(fd)
        os.close(fq)
    return open(path, "rb").read(), open(path + ".bqc", "rb").read(), qs


@pytest.mark.parametrize("n_runs", [1, 3, 7])
def test_armed_merger_leaves_the_members_alone_and_writes_the_judges_summary(ctx, case, tmp_path, n_runs):
    key_of = lambda r: sref.packed_key(r, len(cases.REF_LEN), 2 ** 31 - 1)
    rng = random.Random(n_runs)
    runs = [sref.run_arrays(r, key_of) for r in sref.make_runs(case["records"], n_runs, rng, empty=1 if n_runs > 1 else None)]
    order = list(range(n_runs))
    rng.shuffle(order)
    plain, none, _ = _finish(ctx, runs, order, str(tmp_path / "plain.bin"))
    assert none == b""
    for opt, how in (((4, -1, 0), "finish"), ((14, -1, 0), "bai"), ((0, 0, 0), "finish")):
        got, qc, qs = _finish(ctx, runs, order, str(tmp_path / "armed.bin"), (case["ref_len"], opt), how, n_ref=len(cases.REF_LEN))
        what = f"{n_runs} runs added as {order}, options {opt}, {how}"
        assert got == plain, what + ": the members changed"
        _same(qc, case["want"][opt], what)
        assert qs.qc_bytes == len(qc) and qs.n_windows == sum(len(r["windows"]) for r in ref.parse(qc)["refs"]) and qs.hbm_bytes > 0 and qs.qc_ms >= qs.scan_ms > 0 and qs.record_ms > 0, what


def test_armed_merger_refusals_and_disarming(ctx, case, tmp_path):
    key_of = lambda r: sref.packed_key(r, len(cases.REF_LEN), 2 ** 31 - 1)
    run = sref.run_arrays(sref.stable_sort(case["records"]), key_of)
    short = case["ref_len"][:5]                                                           # most records name a reference that is not there
    out = str(tmp_path / "r.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 1) as m:
            m.add(0, *run)
            for opt in ((3, -1, 0), (0, -1, 300)):
                with pytest.raises(bw.BwahipError, match="EINVAL"):
                    m.set_qc(case["ref_len"], fd, opt)
            m.set_qc(short, fd, ())
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                m.finish(fd)
            assert os.fstat(fd).st_size == 0                                              # before a byte of the members, and no summary
            m.set_qc(None)
            m.finish(fd)                                                                   # disarmed: the plain finish
            n_plain = os.fstat(fd).st_size
            assert n_plain > 0
            m.set_qc(case["ref_len"], -1, (8, -1, 0))                                      # built and dropped
            m.finish(-1)
            assert os.fstat(fd).st_size == n_plain
    finally:
        os.close(fd)
    got, qc, qs = _finish(ctx, [], [], str(tmp_path / "e.bin"), (case["ref_len"], ()))    # nothing to merge: the summary of no record
    assert got == b"" and qc == ref.build([], case["ref_len"]) and qs.qc_bytes == len(qc)


@pytest.mark.parametrize("n_runs", [1, 3, 7])
def test_armed_marked_finish_sees_the_duplicate_flag(ctx, tmp_path, n_runs):
    c = mcases.record_set(True)
    descs = mcases.judge_descs(c)
    lens = [5000, 100000, 1000, 3000, 64]                                                  # the set's five references; what lies beyond a contig is clipped
    rng = random.Random(n_runs)
    n = len(c["templates"])
    b = [0] + (sorted(rng.sample(range(1, n), n_runs - 1)) if n_runs > 1 else []) + [n]
    key_of = lambda r: sref.packed_key(r, mcases.N_SEQS, mcases.LONGEST)
    runs = []
    for k in range(n_runs):
        recs = [(x, t) for t, (_, reads) in enumerate(c["templates"][b[k]:b[k + 1]]) for r in reads for x in r]
        recs.sort(key=lambda p: sref.order_key(p[0]))
        runs.append((*sref.run_arrays([x for x, _ in recs], key_of), np.array([t for _, t in recs], dtype=np.uint32), mcases.as_desc_array(descs[b[k]:b[k + 1]])))
    order = list(range(n_runs))
    rng.shuffle(order)
    unmarked = sref.stable_sort([x for r in c["reads"] for x in r])
    marked = mref.mark(unmarked, c["names"], True)["records"]
    opt = (8, 0x400, 0)                                                                    # duplicates alone are kept out of the coverage
    want, want_unmarked = ref.build(marked, lens, opt), ref.build(unmarked, lens, opt)
    assert want != want_unmarked and ref.parse(want)["count"][0][4] > 20 and ref.parse(want_unmarked)["count"][0][4] == 0
    plain, _, _ = _finish(ctx, runs, order, str(tmp_path / "plain.bin"), how="markdup", with_dup=True)
    got, qc, qs = _finish(ctx, runs, order, str(tmp_path / "armed.bin"), (lens, opt), "markdup", with_dup=True)
    assert got == plain, f"{n_runs} runs: the members changed"
    _same(qc, want, f"{n_runs} runs added as {order}, marked")
    got, qc, _ = _finish(ctx, runs, order, str(tmp_path / "unmarked.bin"), (lens, opt), "finish", with_dup=True)
    _same(qc, want_unmarked, f"{n_runs} runs, the unmarked finish of the same runs")


# ---------------------------------------------------------------------------------------------------------------- 3. the stream driver
K = 300 * 2 * 150
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"
LIBS = ("mid_insert", "rf", "mixed4", "edges")


@pytest.fixture(scope="module")
def stream_case(built, tmp_path_factory):
    """Four of the committed paired-end libraries over the suite's 1 Mb genome (300 pairs each), one after the other, then the first 100
    pairs once more under other names, so that marking finds duplicates: five batches."""
    d = tmp_path_factory.mktemp("qc_stream")
    fqs = []
    for mate in (1, 2):
        path = str(d / f"s_{mate}.fq")
        with open(path, "wb") as f:
            for name in LIBS:
                f.write(gzip.open(os.path.join(common.GOLDEN, f"pelib_{name}_{mate}.fq.gz")).read())
        names, seqs, quals = bw.read_fastq(path)
        with open(path, "ab") as f:
            for n, s, q in list(zip(names, seqs, quals))[:100]:
                f.write(b"@again_" + n + b"\n" + s + b"\n+\n" + q + b"\n")
        fqs.append(path)
    return dict(fq1=fqs[0], fq2=fqs[1])


def _stream(fn, ctxs, sc, tmp_path, qc=None, **kw):
    opt = bw.default_opt()
    opt.n_threads = 4
    out = str(tmp_path / "o.bam")
    fd, fb, fq = (os.open(out + x, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for x in ("", ".bai", ".bqc"))
    try:
        extra = dict(qc_fd=fq, qc=qc) if qc is not None else {}
        res = fn(ctxs, sc["fq1"], sc["fq2"], fd, fb, hdr_line=HDR, opt=opt, chunk_bases=K, reader_threads=2, **extra, **kw)
    finally:
        for x in (fd, fb, fq):
            os.close(x)
    return open(out, "rb").read(), open(out + ".bai", "rb").read(), open(out + ".bqc", "rb").read(), res


@pytest.mark.parametrize("markdup", [1, 0])
@pytest.mark.parametrize("n_ctx", [1, 2])
def test_stream_driver_writes_the_summary_of_the_file(small_index, stream_case, tmp_path, n_ctx, markdup):
    spill = tmp_path / "spill"
    spill.mkdir()
    qc_opt = (8, -1, 0) if markdup else (0, 0, 20)
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            bns = bw.lib().bwahip_bns(c0._h).contents
            lens = [bns.anns[i].len for i in range(bns.n_seqs)]
            what = f"n_ctx {n_ctx}, markdup {markdup}"
            base = bw.stream_run_bam_sorted_dev_markdup if markdup else bw.stream_run_bam_sorted_dev_bai
            bam0, bai0, none, res0 = _stream(base, ctxs, stream_case, tmp_path, hbm_budget=8 << 30)
            assert none == b"" and res0[1].fell_back == 0 and res0[0].n_batches == 5 and res0[0].n_reads == 2600, what
            bam, bai, qc, (st, sd, ms, qs) = _stream(bw.stream_run_bam_sorted_dev_qc, ctxs, stream_case, tmp_path, qc=qc_opt, markdup=markdup, hbm_budget=8 << 30)
            assert bam == bam0 and bai == bai0 and sd.fell_back == 0, what + ": the file or its index changed"
            n_ref, recs, _, _ = bai_ref.split_file(bam)
            assert n_ref == len(lens) and len(recs) >= 2600
            want = ref.build(recs, lens, qc_opt)
            _same(qc, want, what + ", device")
            s = ref.parse(qc)
            assert (s["count"][0][4] > 0) == bool(markdup) and s["count"][0][11] > 1000 and sum(r["covered"] for r in s["refs"]) > 100000, what
            assert qs.qc_bytes == len(qc) and qs.hbm_bytes > 0 and qs.qc_ms > 0 and (ms.n_marked > 0) == bool(markdup), what
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # bad options: before anything starts
                _stream(bw.stream_run_bam_sorted_dev_qc, ctxs, stream_case, tmp_path, qc=(3, -1, 0), markdup=markdup, hbm_budget=8 << 30)
            if markdup:
                return
            # a budget for one and a half batches and the QC stage: the fall-back begins at run 1, the summary comes from the host builder
            raw, n_rec = int(1.5 / 5 * sd.dev.raw_bytes), int(1.5 / 5 * sd.dev.n_records)
            windows = sum((n + 16383) >> 14 for n in lens)
            budget = bw.bam_devmerge_hbm_need(raw, n_rec, 2, 1024) + bw.bam_devmerge_bai_hbm_need(n_rec, (raw + 65279) // 65280, n_ref, windows)
            fb0, fbai0, _, res0 = _stream(base, ctxs, stream_case, tmp_path, hbm_budget=budget, tmp_dir=str(spill), level=1)
            assert res0[1].fell_back == 1
            budget += bw.qc_hbm_need(n_ref, sum(lens), windows, 0)
            fbam, fbai, fqc, (st, sd, ms, qs) = _stream(bw.stream_run_bam_sorted_dev_qc, ctxs, stream_case, tmp_path, qc=qc_opt, markdup=0, hbm_budget=budget, tmp_dir=str(spill), level=1)
            assert sd.fell_back == 1 and sd.fell_back_at_run == res0[1].fell_back_at_run and fbam == fb0 and fbai == fbai0, what + ": the fall-back's file or index changed"
            assert gzip.decompress(fbam) == gzip.decompress(bam), what
            _same(fqc, qc, what + ": the fall-back's summary is not the device's")
            assert qs.qc_bytes == len(fqc) and qs.hbm_bytes == 0 and os.listdir(spill) == []
        finally:
            for c in ctxs[1:]:
                c.close()
