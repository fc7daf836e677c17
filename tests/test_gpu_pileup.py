"""The pileup of candidate variant sites on the device (csrc/k_pileup.hip): the stage alone (Context.kat_pileup), the armed device merger and
the stream driver's entry point.  The judge is tests/pileup_ref.py -- plain Python over the records' bytes, the contig lengths and the packed
reference, written from the rule in include/bwahip.h.  Every comparison is byte for byte: no tolerance anywhere."""
import gzip
import os
import random
import struct

import numpy as np
import pytest

import bai_ref
import bam_sort_ref as sref
import bgzf_ref
import common
import markdup_cases as mcases
import markdup_ref as mref
import pileup_cases as cases
import pileup_ref as ref
import qc_ref
from common import bw

pytestmark = pytest.mark.gpu

OPTS = [(), (0, cases.MIN_BASEQ, -1, 1), (cases.MIN_MAPQ, 0, -1, 3), (0, cases.MIN_BASEQ, 0, 2), (20, 19, 0x400, 2)]


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(built):
    c = cases.record_set()
    cases.assert_families(c)
    c["want"] = {o: ref.build(c["records"], c["ref_len"], c["pac"], o) for o in OPTS}
    return c


def _same(got, want, what):
    assert got == want, f"{what}: {ref.first_difference(got, want)}"


def _kat(ctx, c, opt=()):
    return ctx.kat_pileup(c["buf"], c["off"], c["ref_len"], c["pac"], opt)


# ---------------------------------------------------------------------------------------------------------------- 1. the stage
@pytest.mark.parametrize("opt", OPTS)
def test_kat_pileup_equals_the_judge(ctx, case, opt):
    _same(_kat(ctx, case, opt), case["want"][opt], f"options {opt}")


def test_kat_pileup_invariances(ctx, case):
    opt = (0, cases.MIN_BASEQ, -1, 1)
    want = case["want"][opt]
    recs = list(case["records"])
    random.Random(5).shuffle(recs)
    _same(_kat(ctx, cases.make_case(recs, case["refs"]), opt), want, "shuffled")
    _same(_kat(ctx, cases.make_case(sref.stable_sort(case["records"]), case["refs"]), opt), want, "sorted")   # as a sorted file holds them
    _same(_kat(ctx, cases.make_case(case["records"], case["refs"], shift=13), opt), want, "every record 13 bytes further on")
    _same(_kat(ctx, case, opt), want, "a second call on the same context")
    few = case["records"][:3]
    c = cases.make_case(few, case["refs"])
    _same(_kat(ctx, c, opt), ref.build(few, c["ref_len"], c["pac"], opt), "three records after thousands: nothing of them is left")


def test_kat_pileup_degenerate_inputs(ctx):
    refs = cases.reference()
    lens, pac = cases.REF_LEN, ref.pack_reference(refs)
    for opt in ((), (0, 0, 0, 1)):
        want = ref.build([], lens, pac, opt)
        assert len(want) == 64
        _same(ctx.kat_pileup(b"", np.zeros(1, dtype=np.int64), lens, pac, opt), want, "no record")
    nc = [cases.rec(b"a", -1, -1, [], [1, 2], flag=0x4), cases.rec(b"b", -1, 5, [(3, cases.M)], [1, 2, 4], flag=0x4 | 0x200)]
    c = cases.make_case(nc, [])
    _same(ctx.kat_pileup(c["buf"], c["off"], [], None, ()), ref.build(nc, [], b"", ()), "no reference at all")
    quiet = [cases.rec(b"a", cases.BIG, 100, [(50, cases.M)], cases.read_over(refs, cases.BIG, 100, [(50, cases.M)])),
             cases.rec(b"c", cases.QUIET, 7, [(4, cases.S), (9, cases.M)], [15] * 4 + cases.read_over(refs, cases.QUIET, 7, [(9, cases.M)]), flag=0x10)]
    c = cases.make_case(quiet, refs)
    want = ref.build(quiet, lens, pac, (0, 0, -1, 1))
    assert ref.parse(want)["n_obs"] == [0, 0, 0]
    _same(_kat(ctx, c, (0, 0, -1, 1)), want, "no observation")
    one = [cases.rec(b"x", 1, 0, [(5, cases.M)], [8] * 5)]
    c = cases.make_case(one, [[], [0] * 5])
    _same(_kat(ctx, c, (0, 0, -1, 1)), ref.build(one, [0, 5], c["pac"], (0, 0, -1, 1)), "a reference of no bases")


def test_kat_pileup_refusals(ctx, case):
    """The bad record first, then at least 300 KB of ordinary records: even a kernel that read beyond a record would stay inside the
    allocation.  An error code is expected and nothing else; what the rule does not check counts as it is."""
    tail = cases.ordinary(300000)
    assert sum(map(len, tail)) >= 300000
    for what, (bad, refused) in cases.bad_records().items():
        c = cases.make_case([bad] + tail, case["refs"])
        if refused:
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                _kat(ctx, c)
        else:
            _same(_kat(ctx, c), ref.build(c["records"], c["ref_len"], c["pac"]), what)
    c = cases.make_case(tail[:700] + [cases.bad_records()["l_seq one too large"][0]] + tail[700:], case["refs"])   # in a later workgroup
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        _kat(ctx, c)
    for opt in ((-1, 0, -1, 0), (256, 0, -1, 0), (0, -1, -1, 0), (0, 94, -1, 0), (0, 0, 65536, 0), (0, 0, -1, -1), (0, 0, -1, 65536)):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            _kat(ctx, case, opt)
    for lens in (case["ref_len"][:-1] + [-1], case["ref_len"][:-1] + [1 << 31]):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.kat_pileup(case["buf"], case["off"], lens, case["pac"], ())
    with pytest.raises(bw.BwahipError, match="ECAPACITY"):
        ctx.kat_pileup(case["buf"], case["off"], [(1 << 31) - 1] * 513, case["pac"], ())
    with pytest.raises(bw.BwahipError, match="EINVAL"):                                    # offsets that decrease
        ctx.kat_pileup(case["buf"], np.array([0, 100, 50], dtype=np.int64), case["ref_len"], case["pac"], ())
    _same(_kat(ctx, case, OPTS[2]), case["want"][OPTS[2]], "the context after the refusals")


# ---------------------------------------------------------------------------------------------------------------- 2. the armed merger
def _finish(ctx, runs, order, path, arm=None, how="finish", with_dup=False, n_ref=0):
    """The members a DevMerger writes for these runs and, when armed with (ref_len, pac, opt), the pileup."""
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fp = os.open(path + ".bpu", os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    ps = None
    try:
        with bw.DevMerger(ctx, 1) as m:
            for k in order:
                (m.add_dup(k, *runs[k]) if with_dup else m.add(k, *runs[k][:3]))
            if arm:
                ps = m.set_pileup(arm[0], arm[1], fp, arm[2])
            if how == "finish":
                m.finish(fd)
            elif how == "bai":
                m.finish_bai(fd, -1, 0, n_ref)
            else:
                m.finish_markdup(fd)
    finally:
        os.close(fd)
        os.close(fp)
    return open(path, "rb").read(), open(path + ".bpu", "rb").read(), ps


@pytest.mark.parametrize("n_runs", [1, 3, 7])
def test_armed_merger_leaves_the_members_alone_and_writes_the_judges_pileup(ctx, case, tmp_path, n_runs):
    key_of = lambda r: sref.packed_key(r, len(cases.REF_LEN), 2 ** 31 - 1)
    rng = random.Random(n_runs)
    runs = [sref.run_arrays(r, key_of) for r in sref.make_runs(case["records"], n_runs, rng, empty=1 if n_runs > 1 else None)]
    order = list(range(n_runs))
    rng.shuffle(order)
    plain, none, _ = _finish(ctx, runs, order, str(tmp_path / "plain.bin"))
    assert none == b""
    for opt, how in ((OPTS[0], "finish"), (OPTS[1], "bai"), (OPTS[4], "finish")):
        got, pu, ps = _finish(ctx, runs, order, str(tmp_path / "armed.bin"), (case["ref_len"], case["pac"], opt), how, n_ref=len(cases.REF_LEN))
        what = f"{n_runs} runs added as {order}, options {opt}, {how}"
        assert got == plain, what + ": the members changed"
        _same(pu, case["want"][opt], what)
        s = ref.parse(pu)
        assert ps.pu_bytes == len(pu) and ps.n_sites == len(s["sites"]) and ps.n_alleles == sum(len(x["alleles"]) for x in s["sites"]) and list(ps.n_obs) == s["n_obs"], what
        assert ps.hbm_bytes > 0 and ps.pileup_ms >= ps.observe_ms > 0 and ps.sort_ms > 0 and ps.evidence_ms > 0, what


def test_armed_merger_refusals_disarming_and_the_spill_interlock(ctx, case, tmp_path):
    key_of = lambda r: sref.packed_key(r, len(cases.REF_LEN), 2 ** 31 - 1)
    run = sref.run_arrays(sref.stable_sort(case["records"]), key_of)
    short = case["ref_len"][:5]                                                           # most records name a reference that is not there
    out = str(tmp_path / "r.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 1) as m:
            m.add(0, *run)
            for opt in ((0, 94, -1, 0), (300, 0, -1, 0)):
                with pytest.raises(bw.BwahipError, match="EINVAL"):
                    m.set_pileup(case["ref_len"], case["pac"], fd, opt)
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # the context's index has other contigs than these
                m.set_pileup(case["ref_len"], None, fd, ())
            m.set_pileup(short, case["pac"], fd, ())
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                m.finish(fd)
            assert os.fstat(fd).st_size == 0                                              # before a byte of the members, and no pileup
            m.set_pileup(None)
            m.finish(fd)                                                                   # disarmed: the plain finish
            n_plain = os.fstat(fd).st_size
            assert n_plain > 0
            m.set_pileup(case["ref_len"], case["pac"], -1, OPTS[1])                        # built and dropped
            m.finish(-1)
            assert os.fstat(fd).st_size == n_plain
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # armed for the pileup: no spilling
                m.set_spill(1 << 20, str(tmp_path))
        with bw.DevMerger(ctx, 1) as m:                                                    # armed first, before any run: the same both ways
            m.set_pileup(case["ref_len"], case["pac"], -1, ())
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                m.set_spill(1 << 20, str(tmp_path))
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                m.add_spilled(0, *run)
        with bw.DevMerger(ctx, 1) as m:
            m.set_spill(1 << 20, str(tmp_path))
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # armed for spilling: no pileup
                m.set_pileup(case["ref_len"], case["pac"], -1, ())
            m.add_spilled(0, *run)
            m.finish(-1)
    finally:
        os.close(fd)
    got, pu, ps = _finish(ctx, [], [], str(tmp_path / "e.bin"), (case["ref_len"], case["pac"], ()))   # nothing to merge: the pileup of no record
    assert got == b"" and pu == ref.build([], case["ref_len"], case["pac"]) and ps.pu_bytes == len(pu) == 64


@pytest.mark.parametrize("n_runs", [1, 3])
def test_armed_marked_finish_sees_the_duplicate_flag(ctx, tmp_path, n_runs):
    c = mcases.record_set(True)
    descs = mcases.judge_descs(c)
    lens = [5000, 100000, 1000, 3000, 64]                                                  # the set's five references; what lies beyond a contig is clipped
    rng = random.Random(n_runs)
    pac = ref.pack_reference([[rng.randrange(4) for _ in range(n)] for n in lens])          # the set's reads are all A: mismatches wherever the reference is not
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
    opt = (0, 15, 0x400, 2)                                                                # duplicates alone are kept out
    want, want_unmarked = ref.build(marked, lens, pac, opt), ref.build(unmarked, lens, pac, opt)
    assert want != want_unmarked and len(ref.parse(want)["sites"]) > 50
    plain, _, _ = _finish(ctx, runs, order, str(tmp_path / "plain.bin"), how="markdup", with_dup=True)
    got, pu, ps = _finish(ctx, runs, order, str(tmp_path / "armed.bin"), (lens, pac, opt), "markdup", with_dup=True)
    assert got == plain, f"{n_runs} runs: the members changed"
    _same(pu, want, f"{n_runs} runs added as {order}, marked")
    got, pu, _ = _finish(ctx, runs, order, str(tmp_path / "unmarked.bin"), (lens, pac, opt), "finish", with_dup=True)
    _same(pu, want_unmarked, f"{n_runs} runs, the unmarked finish of the same runs")


def test_marking_index_qc_and_pileup_in_one_finish(ctx, tmp_path):
    """Three resident runs of about a thousand records at piece_blocks 1 (several pieces); one finish with marking, the index, the QC summary
    and the pileup all armed writes the members and the three files that the same merger writes with each product armed alone, and the
    files are the judges' on the marked records.  With QC disarmed again the pileup is still the same: no stage moved or went missing."""
    c = mcases.record_set(True, n_tmpl=1250, seed=33)
    n_seqs = mcases.N_SEQS
    rng = random.Random(33)
    def pad(x):                                                                            # 100 to 300 bytes a record, by a trailing Z tag: several pieces
        n = rng.randrange(max(len(x) + 4, 100), 301)
        x += b"XPZ" + b"p" * (n - len(x) - 4) + b"\0"
        return struct.pack("<i", len(x) - 4) + x[4:]
    c["templates"] = [(name, [[pad(x) for x in r] for r in rr]) for name, rr in c["templates"]
                      if all(bai_ref.fields(x, n_seqs)[2] <= bai_ref.MAX_END for r in rr for x in r)]   # what BAI can index
    c["names"] = [n for n, _ in c["templates"]]
    descs = mcases.judge_descs(c)
    lens = [5000, 100000, 1000, 3000, 64]                                                  # the set's five references; what lies beyond a contig is clipped
    pac = ref.pack_reference([[rng.randrange(4) for _ in range(n)] for n in lens])
    n = len(c["templates"])
    b = [0, 3 * n // 10, 13 * n // 20, n]
    key_of = lambda r: sref.packed_key(r, n_seqs, mcases.LONGEST)
    runs = []
    for k in range(3):
        recs = [(x, t) for t, (_, reads) in enumerate(c["templates"][b[k]:b[k + 1]]) for r in reads for x in r]
        recs.sort(key=lambda p: sref.order_key(p[0]))
        assert len(recs) > 600
        runs.append((*sref.run_arrays([x for x, _ in recs], key_of), np.array([t for _, t in recs], dtype=np.uint32), mcases.as_desc_array(descs[b[k]:b[k + 1]])))
    assert 2500 < sum(len(r[1]) for r in runs) < 3800 and sum(len(r[0]) for r in runs) > 3 * 65280
    qc_opt, pu_opt, base = (8, 0x400, 0), (0, 15, 0x400, 2), 4321
    paths = [str(tmp_path / x) for x in ("m.bin", "m.bai", "m.bqc", "m.bpu")]

    def finish(m, index, qc, pileup):
        """A marked finish of merger m with these products armed: the four files' bytes (b"" for a product that is not armed)."""
        fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths]
        try:
            m.set_qc(lens, fds[2], qc_opt) if qc else m.set_qc(None)
            m.set_pileup(lens, pac, fds[3], pu_opt) if pileup else m.set_pileup(None)
            m.finish_markdup(fds[0], fds[1], base, n_seqs if index else -1)
        finally:
            for fd in fds:
                os.close(fd)
        return [open(p, "rb").read() for p in paths]

    with bw.DevMerger(ctx, 1) as m:
        for k in (1, 2, 0):
            m.add_dup(k, *runs[k])
        alone = [finish(m, False, False, False), finish(m, True, False, False), finish(m, False, True, False), finish(m, False, False, True)]
        members, bai, qc, pu = finish(m, True, True, True)                                 # (set_qc before set_pileup here; the stages' order is the merger's)
        for k, part in enumerate(("members", "index", "QC summary", "pileup")):
            assert [bool(x) for x in alone[k]] == [True] + [j == k for j in range(1, 4)], part
            assert (members, bai, qc, pu)[k] == alone[k][k], f"all four armed: the {part} differs from the one the merger writes with it armed alone"
            assert alone[k][0] == members, part
        again = finish(m, False, False, True)
        assert again[3] == pu and again[0] == members and again[1] == again[2] == b"", "QC disarmed, the pileup still armed"
    unmarked = sref.stable_sort([x for _, rr in c["templates"] for r in rr for x in r])
    marked = mref.mark(unmarked, c["names"], True)["records"]
    assert bgzf_ref.inflate(members) == b"".join(marked) and marked != unmarked
    offs = [base]
    for mem in bgzf_ref.parse(members):
        offs.append(offs[-1] + mem["size"])
    assert len(offs) > 3
    assert bai == bai_ref.build(marked, offs, n_seqs), "the index is not the judge's"
    assert qc == qc_ref.build(marked, lens, qc_opt), qc_ref.first_difference(qc, qc_ref.build(marked, lens, qc_opt))
    _same(pu, ref.build(marked, lens, pac, pu_opt), "all four armed")
    assert len(ref.parse(pu)["sites"]) > 50


# ---------------------------------------------------------------------------------------------------------------- 3. the stream driver
K = 300 * 2 * 150
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"
LIBS = ("mid_insert", "rf", "mixed4", "edges")


@pytest.fixture(scope="module")
def stream_case(built, tmp_path_factory):
    """The case of tests/test_gpu_qc.py: four of the committed paired-end libraries over the suite's 1 Mb genome (300 pairs each), then the
    first 100 pairs once more under other names, so that marking finds duplicates: five batches.  The simulated reads carry sequencing
    errors and variants -- of the 2 396 alignments the oracle makes of the four libraries 1 586 have NM > 0, 5 926 edits in all -- so the
    pileup of the file has sites, and the repeated pairs raise some alleles to two observations."""
    d = tmp_path_factory.mktemp("pu_stream")
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


def _stream(fn, ctxs, sc, tmp_path, index=True, hbm_budget=8 << 30, **kw):
    opt = bw.default_opt()
    opt.n_threads = 4
    out = str(tmp_path / "o.bam")
    fd, fb, fq, fp = (os.open(out + x, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for x in ("", ".bai", ".bqc", ".bpu"))
    try:
        extra = dict(pu_fd=fp) if "pileup" in kw else {}
        res = fn(ctxs, sc["fq1"], sc["fq2"], fd, fb if index else -1, fq, hdr_line=HDR, opt=opt, chunk_bases=K, reader_threads=2, hbm_budget=hbm_budget, **extra, **kw)
    finally:
        for x in (fd, fb, fq, fp):
            os.close(x)
    return [open(out + x, "rb").read() for x in ("", ".bai", ".bqc", ".bpu")], res


@pytest.mark.parametrize("markdup", [1, 0])
@pytest.mark.parametrize("n_ctx", [1, 2])
def test_stream_driver_writes_the_pileup_of_the_file(small_index, stream_case, tmp_path, n_ctx, markdup):
    qc_opt = (8, -1, 0)
    pu_opt = (0, 13, -1, 1) if markdup else (20, 0, 0, 2)
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            bns = bw.lib().bwahip_bns(c0._h).contents
            lens = [bns.anns[i].len for i in range(bns.n_seqs)]
            pac = open(small_index["prefix"] + ".pac", "rb").read()[:(sum(lens) + 3) // 4]
            what = f"n_ctx {n_ctx}, markdup {markdup}"
            (bam0, bai0, qc0, none), res0 = _stream(bw.stream_run_bam_sorted_dev_qc, ctxs, stream_case, tmp_path, qc=qc_opt, markdup=markdup)
            assert none == b"" and res0[1].fell_back == 0 and res0[0].n_batches == 5 and res0[0].n_reads == 2600, what
            (bam, bai, qc, pu), (st, sd, ms, qs, ps) = _stream(bw.stream_run_bam_sorted_dev_pileup, ctxs, stream_case, tmp_path, qc=qc_opt, markdup=markdup, pileup=pu_opt)
            assert bam == bam0 and bai == bai0 and qc == qc0 and sd.fell_back == 0, what + ": the file, its index or its summary changed"
            n_ref, recs, _, _ = bai_ref.split_file(bam)
            assert n_ref == len(lens) and len(recs) >= 2600
            _same(pu, ref.build(recs, lens, pac, pu_opt), what)
            s = ref.parse(pu)
            assert len(s["sites"]) > 20 and s["n_obs"][0] > 1000 and ps.pu_bytes == len(pu) and ps.n_sites == len(s["sites"]) and ps.hbm_bytes > 0 and ps.pileup_ms > 0, what
            assert (ms.n_marked > 0) == bool(markdup), what
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # bad options: before anything starts
                _stream(bw.stream_run_bam_sorted_dev_pileup, ctxs, stream_case, tmp_path, markdup=markdup, pileup=(0, 94, -1, 0))
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # no options at all
                _stream(bw.stream_run_bam_sorted_dev_pileup, ctxs, stream_case, tmp_path, markdup=markdup, pileup=None)
        finally:
            for c in ctxs[1:]:
                c.close()


@pytest.mark.parametrize("with_index_and_qc", [False, True])
def test_stream_driver_budget_counts_the_pileup_to_the_byte(small_index, stream_case, tmp_path, with_index_and_qc):
    """The entry point's HBM budget at its boundary: the merger's need for all five runs plus bwahip_pileup_hbm_need of their records -- with
    the index and the QC summary, their shares as well -- is a budget the run fits (no fall-back, every file that of the ample run); one
    byte less and the last run is refused, as this entry point never falls back."""
    qc_opt = (8, -1, 0) if with_index_and_qc else None
    kw = dict(index=with_index_and_qc, qc=qc_opt, markdup=0, pileup=(20, 0, 0, 2))
    with bw.Context(small_index["prefix"]) as c0:
        bns = bw.lib().bwahip_bns(c0._h).contents
        lens = [bns.anns[i].len for i in range(bns.n_seqs)]
        files0, (st, sd, _, _, ps) = _stream(bw.stream_run_bam_sorted_dev_pileup, [c0], stream_case, tmp_path, **kw)
        raw, n_rec, n_runs = sd.dev.raw_bytes, sd.dev.n_records, sd.dev.n_runs
        assert sd.fell_back == 0 and n_runs == 5 and n_rec >= 2600 and files0[3] and bool(files0[1]) == bool(files0[2]) == with_index_and_qc
        need = bw.bam_devmerge_hbm_need(raw, n_rec, n_runs, 1024) + bw.pileup_hbm_need(n_rec)
        if with_index_and_qc:
            need += bw.bam_devmerge_bai_hbm_need(n_rec, (raw + 65279) // 65280, len(lens), sum((n + 16383) >> 14 for n in lens))
            need += bw.qc_hbm_need(len(lens), sum(lens), sum((n + 255) >> 8 for n in lens), 0)
        print(f"index and QC {with_index_and_qc}: raw {raw}, records {n_rec}, runs {n_runs}, need {need}, of it the pileup's {bw.pileup_hbm_need(n_rec)}")
        files, (_, sd, _, _, _) = _stream(bw.stream_run_bam_sorted_dev_pileup, [c0], stream_case, tmp_path, hbm_budget=need, **kw)
        assert sd.fell_back == 0 and files == files0, "a budget of exactly the need"
        with pytest.raises(bw.BwahipError, match="ECAPACITY"):
            _stream(bw.stream_run_bam_sorted_dev_pileup, [c0], stream_case, tmp_path, hbm_budget=need - 1, **kw)
