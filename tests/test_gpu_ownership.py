"""Who owns what on the device: bwahip_live_resources() -- device buffers and bytes, pinned buffers and bytes, events, streams the library
holds in this process -- around every way of making, growing and dropping them.  A context and everything that ran on it give back exactly
what they took; a refused call holds nothing; a finish's HBM figures are the stages' own tallies and lie within what is alive."""
import os
import random
import subprocess

import numpy as np
import pytest

import bai_ref
import bam_sort_ref as sref
import bgzf_ref
import common
import dedup_cases
import dp_kat
import mark_cases
import markdup_cases as mcases
import markdup_ref as mref
import mate_insert_cases
import qc_ref
from common import bw
from test_gpu_bam_spill import K, QC_LENS, QC_OPT, STREAM_QC, _bam_header, _budget_for_a_split_after_run_0, _indexable, _lens, _stream, stream_input

pytestmark = pytest.mark.gpu

N_REF = mcases.N_SEQS
FIGURES = ("device buffers", "device bytes", "pinned buffers", "pinned bytes", "events", "streams")


def _oracle(prefix, fqs, extra=()):
    out = subprocess.run([common.ORACLE, "mem", "-t", "8", *extra, prefix, *fqs], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    return [l for l in out.split(b"\n") if l and not l.startswith(b"@")]


def _records_of(sam):
    return [l for l in bytes(sam).split(b"\n") if l and not l.startswith(b"@")]


@pytest.fixture(scope="module")
def reads(small_index, tmp_path_factory):
    """200 single-end reads, 200 pairs, and the stream tests' 2 570 pairs (three batches of K bases), with the oracle's SAM records."""
    d = str(tmp_path_factory.mktemp("own_reads"))
    se, p1, p2 = (os.path.join(d, n) for n in ("se.fq", "p_1.fq", "p_2.fq"))
    bw.make_reads(small_index["fa"], se, None, 200, 150, 10000, 2000, 500, 301)
    bw.make_reads(small_index["fa"], p1, p2, 400, 150, 10000, 2000, 500, 302)
    fq1, fq2, _ = stream_input(small_index["fa"], d)
    se50 = os.path.join(d, "se50.fq")
    with open(se50, "wb") as f:
        f.write(b"".join(open(se, "rb").read().split(b"\n")[k] + b"\n" for k in range(4 * 50)))
    return dict(se=se, se50=se50, p1=p1, p2=p2, fq1=fq1, fq2=fq2, want_se=_oracle(small_index["prefix"], [se]), want_se50=_oracle(small_index["prefix"], [se50]),
                want_stream=_oracle(small_index["prefix"], [fq1, fq2], ["-K", str(K)]))


@pytest.fixture(scope="module")
def marked(small_index, tmp_path_factory):
    """Three synthetic runs with templates and descriptors, as a merger takes them with add_dup, and the judges' answers: the marked
    records, their members after a header, the index and the QC summary of that file.  Made once."""
    d = tmp_path_factory.mktemp("own_marked")
    c = mcases.record_set(True, n_tmpl=400, seed=9)
    c["templates"] = [t for t in c["templates"] if all(_indexable(x) for r in t[1] for x in r)]
    c["names"], c["reads"] = [n for n, _ in c["templates"]], [r for _, rr in c["templates"] for r in rr]
    descs = mcases.judge_descs(c)
    n = len(c["templates"])
    b = [0] + sorted(random.Random(6).sample(range(1, n), 2)) + [n]
    key_of = lambda r: sref.packed_key(r, mcases.N_SEQS, mcases.LONGEST)
    runs = []
    for k in range(3):
        recs = [(x, t) for t, (_, rr) in enumerate(c["templates"][b[k]:b[k + 1]]) for r in rr for x in r]
        recs.sort(key=lambda p: sref.order_key(p[0]))
        runs.append((*sref.run_arrays([x for x, _ in recs], key_of), np.array([t for _, t in recs], dtype=np.uint32), mcases.as_desc_array(descs[b[k]:b[k + 1]])))
    j = mref.mark(sref.stable_sort([x for r in c["reads"] for x in r]), c["names"], True)
    hdr_path = str(d / "hdr.bgzf")
    fd = os.open(hdr_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    bw.bgzf_write(fd, _bam_header(N_REF), 1, 1)
    os.close(fd)
    return dict(runs=runs, records=j["records"], stats=j["stats"], hdr=open(hdr_path, "rb").read(), qc=qc_ref.build(j["records"], QC_LENS, QC_OPT),
                dup_case=mcases.record_set(True, n_tmpl=60, seed=3))


def _hand_finish(ctx, s, d):
    """The merger driven by hand: three runs, the QC stage armed, finish_markdup with the index.  Returns the three files, the five stats and
    the live figures while the merger still holds everything."""
    paths = [os.path.join(d, n) for n in ("m.bin", "m.bai", "m.bqc")]
    fd, fb, fq = (os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths)
    try:
        with bw.DevMerger(ctx, 1) as m:
            m.set_spill(1 << 30, None, 2)
            for k in (2, 0, 1):
                m.add_spilled(k, *s["runs"][k]) if k == 1 else m.add_dup(k, *s["runs"][k])
            qs = m.set_qc(QC_LENS, fq, QC_OPT)
            st, bs, ms = m.finish_markdup(fd, fb, len(s["hdr"]), N_REF)
            sp = m.spill_stats()
            live = bw.live_resources()
    finally:
        for x in (fd, fb, fq):
            os.close(x)
    members, bai, qc = (open(p, "rb").read() for p in paths)
    marked = b"".join(s["records"])
    assert bgzf_ref.inflate(members) == marked and members == ctx.kat_bgzf(marked)[0], "the merger's members are not the judge's marked records"
    assert bai == bai_ref.from_file(s["hdr"] + members + bgzf_ref.EOF_BLOCK) and qc == s["qc"]
    assert [list(ms.n_templates), list(ms.n_dup_templates), ms.n_marked] == [list(s["stats"][0]), list(s["stats"][1]), s["stats"][2]] and st.n_records == len(s["records"])
    return (members, bai, qc), (st, bs, ms, qs, sp), live


def _member_lens(members):
    out, at = [], 0
    while at < len(members):
        out.append(int.from_bytes(members[at + 16:at + 18], "little") + 1)
        at += out[-1]
    return np.array(out, dtype=np.int32)


def _known_answers(ctx, s, members, bai, qc):
    """One successful call of each known-answer entry point that makes buffers (and, two of them, events) of its own."""
    assert ctx.kat_occ4(np.array([0, 1, 1000], dtype=np.uint64)).shape[0] == 3
    case = dp_kat.rand_case(np.random.default_rng(4), "glb", qlen=60, w=20)
    assert dp_kat.device_global(ctx, [case], bw.KAT_GLOBAL_AUTO_BIG)[0][1] >= 1
    gap, mlr, build = mate_insert_cases.SETS["state"]
    opt = bw.default_opt()
    opt.max_chain_gap, opt.mask_level_redun = gap, mlr
    items = build()
    assert len(ctx.kat_mate_insert(*mate_insert_cases.pack(items), opt)[1]) == len(items)
    recs, _ = ctx.kat_chain([700], [0, 1], [[5000, 10, 20, 0]], [0, 0], np.zeros((0, 3)))
    assert int(common.by_read(recs)[0][bw.STAGE_CHAIN_FLT][0]) == 1
    assert len(ctx.kat_mark([0, 1], [mark_cases.reg(0, 100, 90)])) > 0
    dcs = [dedup_cases.Case("own", np.zeros(150, np.uint8), [dedup_cases.reg(100 + k, 200 + k, 0, 100, 50, rid=0), dedup_cases.reg(5000, 5100, 10, 110, 60, rid=0)]) for k in range(2)]
    assert [len(x) for x in ctx.kat_dedup(*dedup_cases.pack(dcs)[:4])[0]] == [2, 2]
    buf = b"".join(s["records"])
    off = np.concatenate(([0], np.cumsum([len(r) for r in s["records"]]))).astype(np.int64)
    assert ctx.kat_bai(buf, off, _member_lens(members), len(s["hdr"]), N_REF) == bai
    assert ctx.kat_qc(buf, off, QC_LENS, QC_OPT) == qc
    c = s["dup_case"]
    assert ctx.kat_dup_desc(c["buf"], c["off"], True).tobytes() == mcases.as_desc_array(mcases.judge_descs(c)).tobytes()
    assert bgzf_ref.inflate(ctx.kat_bgzf(buf)[0]) == buf


def test_destroy_gives_everything_back(small_index, reads, marked, tmp_path):
    start = bw.live_resources()
    spill_dir = tmp_path / "spill"
    spill_dir.mkdir()
    pe = bw.default_opt()
    pe.flag |= 0x2
    c0 = bw.Context(small_index["prefix"])
    c1 = c0.clone()
    try:
        # the one-piece entry points: SAM, sorted BAM with templates, BGZF members
        with bw.FastqReader(reads["se"]) as rd:
            arr, n = rd.next(10 ** 9)
            assert n == 200 and _records_of(c0.process_seqs_text_array(arr, n)) == reads["want_se"]
        with bw.FastqReader(reads["p1"], reads["p2"]) as rd:
            arr, n = rd.next(10 ** 9)
            assert n == 400
            rec, keys, rec_off, tmpl, desc = c0.process_seqs_bam_sorted_dup_array(arr, n, pe)[:5]
            assert len(keys) >= 400 and len(tmpl) == len(keys) and len(desc) == 200
            members = c1.process_seqs_bgzf_array(arr, n, pe)[0]
            assert len(bgzf_ref.inflate(bytes(members))) > 400 * 150
        # the stream driver on both contexts: SAM, then sorted BAM all resident (to find the budget), then with the second run spilled
        opt = bw.default_opt()
        opt.n_threads = 4
        sam_path = str(tmp_path / "o.sam")
        fd = os.open(sam_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            st = bw.stream_run([c0, c1], reads["fq1"], reads["fq2"], fd, opt, chunk_bases=K, reader_threads=2)
        finally:
            os.close(fd)
        assert st.n_batches >= 3 and _records_of(open(sam_path, "rb").read()) == reads["want_stream"]
        case = dict(fq1=reads["fq1"], fq2=reads["fq2"])
        resident = lambda ctxs, fq1, fq2, fd, fb, fq, **kw: bw.stream_run_bam_sorted_dev_qc(ctxs, fq1, fq2, fd, fb, fq, True, STREAM_QC, **kw)
        files0, (st0, sd0, _, _) = _stream(resident, [c0, c1], case, True, str(tmp_path), hbm_budget=8 << 30, piece_blocks=1)
        assert sd0.fell_back == 0 and st0.n_batches == 3
        longest = max(len(r) for r in bai_ref.split_file(files0[0])[1])
        budget = _budget_for_a_split_after_run_0(_lens(c0), sd0, st0.n_reads, 2570, longest, 1, 2)
        spill = lambda ctxs, fq1, fq2, fd, fb, fq, **kw: bw.stream_run_bam_sorted_dev_spill(ctxs, fq1, fq2, fd, fb, fq, True, STREAM_QC, **kw)
        files, (_, sd, sp, _, _) = _stream(spill, [c0, c1], case, True, str(tmp_path), hbm_budget=budget, piece_blocks=1, window_pieces=2,
                                           host_budget=int(0.325 * sd0.dev.raw_bytes), tmp_dir=str(spill_dir))
        assert files == files0 and (sp.first_spilled_run, sp.n_spilled_runs, sd.fell_back) == (1, 2, 0) and os.listdir(spill_dir) == []
        # a merger by hand, and the known answers
        (members, bai, qc), _, middle = _hand_finish(c0, marked, str(tmp_path))
        _known_answers(c0, marked, members, bai, qc)
        assert middle[1] > start[1] and middle[4] > start[4], "device bytes and events in the middle are not above the start"
        assert bw.live_resources()[5] == start[5] + 8                                   # four streams a context; the drivers' own are gone
    finally:
        c1.close()
        c0.close()
    end = bw.live_resources()
    assert end == start, "left behind: " + ", ".join(f"{e - s} {name}" for name, s, e in zip(FIGURES, start, end) if e != s)


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


def test_refused_calls_hold_nothing(ctx, reads, marked):
    """Every refusal that comes after an entry point's argument checks, 20 times over: what is alive after the 20th is what was alive
    after the first (the first may grow a buffer of the context)."""
    names, seqs, quals = bw.read_fastq(reads["se"])
    c = marked["dup_case"]
    bad_off = c["off"].copy()
    bad_off[3] = bad_off[2] + 5                                                          # a read that ends inside a record: the kernel refuses it
    case = dp_kat.rand_case(np.random.default_rng(4), "glb", qlen=60)
    runs = marked["runs"]
    with bw.DevMerger(ctx, 1) as m, bw.DevMerger(ctx, 1) as closed:
        m.add_dup(0, *runs[0])
        closed.set_spill(0, None, 2)                                                     # no byte of host memory and no directory: no run can be placed
        refusals = {
            "kat_ksw_global with an unknown form": (lambda: dp_kat.device_global(ctx, [case], 7), "EINVAL"),
            "kat_dup_desc with a read cut inside a record": (lambda: ctx.kat_dup_desc(c["buf"], bad_off, True), "EINVAL"),
            "add of a run number held": (lambda: m.add(0, *runs[1][:3]), "EINVAL"),
            "add_dup of a run that is held with its templates": (lambda: m.add_dup(0, *runs[0]), "EINVAL"),
            "add_spilled on a closed budget": (lambda: closed.add_spilled(1, *runs[1]), "EIO"),
            "set_spill with a negative budget": (lambda: m.set_spill(-1, None, 2), "EINVAL"),
            "process_seqs_bam with a name of 256 bytes": (lambda: ctx.process_seqs_bam([b"n" * 256] + names[1:5], seqs[:5], quals[:5]), "EINVAL"),
        }
        for what, (call, code) in refusals.items():
            after_first = None
            for k in range(20):
                with pytest.raises(bw.BwahipError, match=code):
                    call()
                if k == 0:
                    after_first = bw.live_resources()
            assert bw.live_resources() == after_first, what
    with bw.FastqReader(reads["se50"]) as rd:
        arr, n = rd.next(10 ** 9)
        assert n == 50 and _records_of(ctx.process_seqs_text_array(arr, n)) == reads["want_se50"], "the context no longer gives the oracle's SAM"


def test_stage_figures_are_the_tally(ctx, marked, tmp_path):
    _, (st, bs, ms, qs, sp), live = _hand_finish(ctx, marked, str(tmp_path))
    figures = (st.hbm_bytes, bs.hbm_bytes, ms.hbm_bytes, qs.hbm_bytes, sp.window_hbm_bytes)
    assert all(f > 0 for f in figures), figures
    resident = [marked["runs"][k] for k in (0, 2)]
    run_bytes = sum(len(rec) + 20 * len(keys) + 8 + 24 * len(desc) for rec, keys, _, _, desc in resident)
    rec, keys, _, _, desc = marked["runs"][1]                                            # the spilled run: its record bytes are in the store
    run_bytes += 20 * len(keys) + 8 + 24 * len(desc)
    assert sum(figures) + run_bytes <= live[1], (figures, run_bytes, live)
