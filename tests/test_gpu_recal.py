"""The base-quality recalibration table on the device (csrc/k_recal.hip): the stage alone (Context.kat_recal), the armed device merger with
resident and spilled runs, and the stream driver's entry point.  The judge is tests/recal_ref.py -- plain Python over the records' bytes,
the contig lengths, the packed reference and the mask, written from the rule in include/bwahip.h.  Every comparison is byte for byte with
the judge: no tolerance anywhere."""
import ctypes as C
import gzip
import os
import random

import numpy as np
import pytest

import bai_ref
import bam_sort_ref as sref
import bgzf_ref
import common
import markdup_cases as mcases
import markdup_ref as mref
import pileup_ref
import qc_ref
import recal_cases as cases
import recal_ref as ref
from common import bw

pytestmark = pytest.mark.gpu

# defaults; max_cycle 700; min_baseq 20; min_mapq 30; exclude_flags 0 -- each with and without the mask
OPTS = [(), (0, 0, -1, cases.MAX_CYCLE), (0, 20, -1, 0), (30, 0, -1, 0), (0, 0, 0, 0)]
N_REF = len(cases.REF_LEN)


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(built):
    c = cases.record_set()
    cases.assert_families(c)
    short = [r for r in c["records"] if ref.fields(r, N_REF)["l_seq"] <= cases.MAX_CYCLE]      # max_cycle 700: without the one longer read
    c["short"] = cases.make_case(short, c["refs"], mask=c["mask"])
    c["want"] = {(o, m): ref.build(_case_for(c, o)["records"], c["ref_len"], c["pac"], c["mask"] if m else None, o) for o in OPTS for m in (True, False)}
    assert len(set(c["want"].values())) == 2 * len(OPTS)
    return c


def _case_for(c, opt):
    return c["short"] if opt and opt[3] == cases.MAX_CYCLE else c


def _same(got, want, what):
    assert got == want, f"{what}: {ref.first_difference(got, want)}"


def _kat(ctx, c, opt=(), mask=True):
    return ctx.kat_recal(c["buf"], c["off"], c["ref_len"], c["pac"], c["mask"] if mask else None, opt)


def _judge(c, opt=(), mask=True):
    return ref.build(c["records"], c["ref_len"], c["pac"], c["mask"] if mask else None, opt)


# ---------------------------------------------------------------------------------------------------------------- 1. the stage
@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("opt", OPTS)
def test_kat_recal_equals_the_judge(ctx, case, opt, mask):
    _same(_kat(ctx, _case_for(case, opt), opt, mask), case["want"][(opt, mask)], f"options {opt}, mask {mask}")


def test_kat_recal_invariances(ctx, case):
    want = case["want"][((), True)]
    recs = list(case["records"])
    random.Random(5).shuffle(recs)
    _same(_kat(ctx, cases.make_case(recs, case["refs"], mask=case["mask"])), want, "shuffled")
    _same(_kat(ctx, cases.make_case(case["records"][::-1], case["refs"], mask=case["mask"])), want, "reversed")
    _same(_kat(ctx, cases.make_case(case["records"], case["refs"], shift=13, mask=case["mask"])), want, "every record 13 bytes further on")
    _same(_kat(ctx, case), want, "a second call on the same context")
    few = cases.make_case(case["records"][:3], case["refs"], mask=case["mask"])
    _same(_kat(ctx, few), _judge(few), "three records after thousands: nothing of them is left")


def test_kat_recal_degenerate_inputs(ctx, case):
    refs = cases.reference()
    lens, pac = cases.REF_LEN, pileup_ref.pack_reference(refs)
    for opt in ((), (0, 0, 0, 5)):
        want = ref.build([], lens, pac, None, opt)
        assert len(want) == 80
        _same(ctx.kat_recal(b"", np.zeros(1, dtype=np.int64), lens, pac, None, opt), want, "no record")
    quiet = [cases.rec(b"a", cases.BIG, 100, [(50, cases.M)], [15] * 50), cases.rec(b"b", -1, -1, [], [1, 2, 4], flag=0x4),
             cases.rec(b"c", cases.QUIET, 7, [(4, cases.S), (9, cases.I)], [1] * 13, flag=0x10), cases.rec(b"d", cases.BIG, 7, [(9, cases.M)], [1] * 9, [0xff] * 9),
             cases.rec(b"e", cases.BIG, 7, [(9, cases.M)], [1] * 9, flag=0x400)]
    c = cases.make_case(quiet, refs, mask=case["mask"])
    want = _judge(c)
    assert len(want) == 80 and ref.parse(want)["n_records"] == 2                           # a and c take part and count no base
    _same(_kat(ctx, c), want, "no counted base")
    c = cases.make_case(quiet[1:2] + quiet[3:], refs)
    want = _judge(c, mask=False)
    assert len(want) == 80 and ref.parse(want)["n_records"] == 0
    _same(_kat(ctx, c, mask=False), want, "no record that takes part")
    # a reference of a dozen bases: three bytes of packed sequence and two of mask, below the words the kernel reads by
    tiny = [[0, 1, 2, 3, 3, 2, 1, 0, 0, 2, 1, 3]]
    reads = [cases.rec(b"t%d" % k, 0, p, [(n, cases.M)], cases.read_over(tiny, 0, p, [(n, cases.M)], random.Random(k), 0.3), [20 + k] * n, f)
             for k, (p, n, f) in enumerate(((0, 12, 0), (3, 9, 0x10), (5, 10, 0x81), (11, 1, 0x91), (0, 1, 0x41)))]
    for mask in (None, ref.make_mask(12, {0, 7, 8, 11}), b"\xff\xff"):
        c = cases.make_case(reads, tiny, mask=mask)
        assert len(c["pac"]) == 3 and (mask is None or len(mask) == 2)
        want = _judge(c)
        assert (len(want) == 80) == (mask == b"\xff\xff") and ref.parse(want)["n_records"] == 5
        _same(_kat(ctx, c), want, f"a dozen bases, mask {mask}")
    # counts of records that are no multiple of the 16 a workgroup takes at a time, of its share, of anything
    for n in (1, 15, 17, 511, 513, 1000):
        c = cases.make_case(case["records"][:n], case["refs"], mask=case["mask"])
        _same(_kat(ctx, c), _judge(c), f"the first {n} records")


def test_kat_recal_refusals(ctx, case):
    """The offending record first, then at least 300 KB of ordinary records: even a kernel that read beyond a record would stay inside the
    allocation.  The first offender in the order given decides between EINVAL and ECAPACITY."""
    refs, mask = case["refs"], case["mask"]
    tail = cases.ordinary(300000)
    assert sum(map(len, tail)) >= 300000 and len(tail) > cases.WG_RECORDS + 200
    kat = lambda recs, opt=(): _kat(ctx, cases.make_case(recs, refs, mask=mask), opt)
    for what, (bad, refused) in cases.bad_records().items():
        if refused:
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                kat([bad] + tail)
        else:
            _same(kat([bad] + tail), ref.build([bad] + tail, case["ref_len"], case["pac"], mask), what)
    bad = cases.bad_records()["l_seq one too large"][0]
    for max_cycle in (0, cases.MAX_CYCLE, 151):                                            # (the ordinary records have at most 150 bases)
        n_long = (max_cycle or ref.DEFAULT_CYCLE) + 1
        long = cases.too_long(refs, n_long - 1)
        opt = (0, 0, -1, max_cycle)
        with pytest.raises(ref.TooLong):
            ref.build([long], case["ref_len"], case["pac"], mask, opt)
        for before, after, code in (([long], [bad], "ECAPACITY"), ([bad], [long], "EINVAL"), ([long], [], "ECAPACITY")):
            for lead in (0, cases.WG_RECORDS + 88):                                                          # in the first workgroup's share, and in a later one's
                with pytest.raises(bw.BwahipError, match=code):
                    kat(tail[:lead] + before + tail[lead:lead + 40] + after + tail[lead + 40:], opt)
        excluded = cases.rec(b"dup", cases.BIG, 50, [(n_long, cases.M)], [1] * n_long, flag=0x400)   # as long, and takes no part: not refused
        _same(kat(tail[:100] + [excluded], opt), ref.build(tail[:100] + [excluded], case["ref_len"], case["pac"], mask, opt), "a long record that takes no part")
    for opt in ((-1, 0, -1, 0), (256, 0, -1, 0), (0, -1, -1, 0), (0, 94, -1, 0), (0, 0, 65536, 0), (0, 0, -1, -1), (0, 0, -1, 65537)):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            _kat(ctx, case, opt)
    for lens in (case["ref_len"][:-1] + [-1], case["ref_len"][:-1] + [1 << 31]):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.kat_recal(case["buf"], case["off"], lens, case["pac"], mask, ())
    with pytest.raises(bw.BwahipError, match="EINVAL"):                                    # offsets that decrease
        ctx.kat_recal(case["buf"], np.array([0, 100, 50], dtype=np.int64), case["ref_len"], case["pac"], mask, ())
    # out_cap too small: ECAPACITY, and *out_len says what it takes
    want = case["want"][((), True)]
    src, off, lens = np.frombuffer(case["buf"], dtype=np.uint8), case["off"], np.asarray(case["ref_len"], dtype=np.int64)
    for cap in (0, 79, len(want) - 1):
        out, ln = np.zeros(max(cap, 1), dtype=np.uint8), C.c_int64(-1)
        rc = bw.lib().bwahip_kat_recal(ctx._h, src.ctypes.data, off.ctypes.data, len(off) - 1, len(lens), lens.ctypes.data, case["pac"], mask, C.byref(bw.recal_opt()),
                                       out.ctypes.data if cap else None, cap, C.byref(ln))
        assert (rc, ln.value) == (-5, len(want)) and not out.any(), cap
    _same(_kat(ctx, case, OPTS[2]), case["want"][(OPTS[2], True)], "the context after the refusals")


# ---------------------------------------------------------------------------------------------------------------- 2. the armed merger
def _key(r):
    return sref.packed_key(r, N_REF, 2 ** 31 - 1)


def _finish(ctx, runs, order, path, arm=None, how="finish", with_dup=False, n_ref=0, spilled=(), pb=1, wp=0):
    """The members a DevMerger writes for these runs and, when armed with (ref_len, pac, mask, opt), the table.  wp > 0: armed for spilling, the
    runs in `spilled` are held so."""
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fr = os.open(path + ".brc", os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    rs = None
    try:
        with bw.DevMerger(ctx, pb) as m:
            if arm:                                                                        # before set_spill: the two are not interlocked
                rs = m.set_recal(arm[0], arm[1], arm[2], fr, arm[3])
            if wp:
                m.set_spill(1 << 30, None, wp)
            for k in order:
                if k in spilled:
                    m.add_spilled(k, *runs[k])
                else:
                    (m.add_dup(k, *runs[k]) if with_dup else m.add(k, *runs[k][:3]))
            if how == "finish":
                m.finish(fd)
            elif how == "bai":
                m.finish_bai(fd, -1, 0, n_ref)
            else:
                m.finish_markdup(fd)
    finally:
        os.close(fd)
        os.close(fr)
    return open(path, "rb").read(), open(path + ".brc", "rb").read(), rs


@pytest.mark.parametrize("n_runs", [1, 3, 7])
def test_armed_merger_leaves_the_members_alone_and_writes_the_judges_table(ctx, case, tmp_path, n_runs):
    rng = random.Random(n_runs)
    order = list(range(n_runs))
    rng.shuffle(order)
    plain = {}
    for opt, mask, how in ((OPTS[0], True, "finish"), (OPTS[1], False, "bai"), (OPTS[4], True, "finish")):
        c = _case_for(case, opt)
        if id(c) not in plain:
            runs = [sref.run_arrays(r, _key) for r in sref.make_runs(c["records"], n_runs, random.Random(n_runs), empty=1 if n_runs > 1 else None)]
            members, none, _ = _finish(ctx, runs, order, str(tmp_path / "plain.bin"))
            assert none == b"" and bgzf_ref.inflate(members) == b"".join(sref.stable_sort(c["records"]))
            plain[id(c)] = (runs, members)
        runs, members = plain[id(c)]
        got, brc, rs = _finish(ctx, runs, order, str(tmp_path / "armed.bin"), (c["ref_len"], c["pac"], c["mask"] if mask else None, opt), how, n_ref=N_REF)
        what = f"{n_runs} runs added as {order}, options {opt}, mask {mask}, {how}"
        assert got == members, what + ": the members changed"
        _same(brc, case["want"][(opt, mask)], what)
        s = ref.parse(brc)
        assert (rs.rc_bytes, rs.n_records, rs.n_bases, rs.n_err, rs.n_masked, list(rs.n_rows)) == (len(brc), s["n_records"], s["n_bases"], s["n_err"], s["n_masked"],
                                                                                                  [len(t) for t in s["tables"]]), what
        assert rs.hbm_bytes >= 16 * 94 * (2 * s["opt"][3] + 18) and rs.recal_ms > 0, what


def test_armed_merger_refusals_and_disarming(ctx, case, tmp_path):
    run = sref.run_arrays(sref.stable_sort(case["records"]), _key)
    short = case["ref_len"][:5]                                                           # most records name a reference that is not there
    out = str(tmp_path / "r.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 1) as m:
            m.add(0, *run)
            for opt in ((0, 94, -1, 0), (300, 0, -1, 0), (0, 0, -1, 65537)):
                with pytest.raises(bw.BwahipError, match="EINVAL"):
                    m.set_recal(case["ref_len"], case["pac"], None, fd, opt)
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # the context's index has other contigs than these
                m.set_recal(case["ref_len"], None, None, fd, ())
            m.finish(fd)                                                                   # the refused calls armed nothing
            n_plain = os.fstat(fd).st_size
            assert n_plain > 0
            os.ftruncate(fd, 0)
            os.lseek(fd, 0, os.SEEK_SET)
            m.set_recal(short, case["pac"], None, fd, ())
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                m.finish(fd)
            m.set_recal(case["ref_len"], case["pac"], case["mask"], fd, (0, 0, -1, cases.MAX_CYCLE))   # the read of 1 024 bases is too long
            with pytest.raises(bw.BwahipError, match="ECAPACITY"):
                m.finish(fd)
            assert os.fstat(fd).st_size == 0                                              # before a byte of the members, and no table
            m.set_recal(None)
            m.finish(fd)                                                                   # disarmed: the plain finish
            assert os.fstat(fd).st_size == n_plain
            m.set_recal(case["ref_len"], case["pac"], case["mask"], -1, OPTS[2])           # built and dropped
            m.finish(-1)
            assert os.fstat(fd).st_size == n_plain
    finally:
        os.close(fd)
    arm = (case["ref_len"], case["pac"], case["mask"], ())
    got, brc, rs = _finish(ctx, [], [], str(tmp_path / "e.bin"), arm)                      # nothing to merge: the table of no record
    assert got == b"" and brc == ref.build([], case["ref_len"], case["pac"], case["mask"]) and rs.rc_bytes == len(brc) == 80
    got, brc, rs = _finish(ctx, [], [], str(tmp_path / "e.bin"), arm, wp=2)
    assert got == b"" and len(brc) == 80


def _marked_set(n_tmpl=420, seed=5, n_runs=3, indexable=False):
    """A paired set of tests/markdup_cases.py cut into runs with templates and descriptors, a random reference under its five contigs (the
    set's reads are all A: mismatches wherever the reference is not) and a mask; the sorted records unmarked and as the judge marks them."""
    c = mcases.record_set(True, n_tmpl=n_tmpl, seed=seed)
    if indexable:
        c["templates"] = [(name, rr) for name, rr in c["templates"] if all(bai_ref.fields(x, mcases.N_SEQS)[2] <= bai_ref.MAX_END for r in rr for x in r)]   # what BAI can index
        c["names"] = [n for n, _ in c["templates"]]
    descs = mcases.judge_descs(c)
    lens = [5000, 100000, 1000, 3000, 64]
    rng = random.Random(seed)
    pac = pileup_ref.pack_reference([[rng.randrange(4) for _ in range(n)] for n in lens])
    mask = ref.make_mask(sum(lens), {g for g in range(sum(lens)) if rng.random() < 0.02})
    n = len(c["templates"])
    b = [0] + (sorted(rng.sample(range(1, n), n_runs - 1)) if n_runs > 1 else []) + [n]
    key_of = lambda r: sref.packed_key(r, mcases.N_SEQS, mcases.LONGEST)
    runs = []
    for k in range(n_runs):
        recs = [(x, t) for t, (_, reads) in enumerate(c["templates"][b[k]:b[k + 1]]) for r in reads for x in r]
        recs.sort(key=lambda p: sref.order_key(p[0]))
        runs.append((*sref.run_arrays([x for x, _ in recs], key_of), np.array([t for _, t in recs], dtype=np.uint32), mcases.as_desc_array(descs[b[k]:b[k + 1]])))
    unmarked = sref.stable_sort([x for _, rr in c["templates"] for r in rr for x in r])
    marked = mref.mark(unmarked, c["names"], True)["records"]
    return dict(runs=runs, lens=lens, pac=pac, mask=mask, unmarked=unmarked, marked=marked)


@pytest.mark.parametrize("n_runs", [1, 3])
def test_armed_marked_finish_leaves_the_marked_records_out(ctx, tmp_path, n_runs):
    s = _marked_set(n_runs=n_runs)
    order = list(range(n_runs))
    random.Random(n_runs).shuffle(order)
    arm = (s["lens"], s["pac"], s["mask"], ())                                             # the defaults: 0x400 is excluded
    plain, _, _ = _finish(ctx, s["runs"], order, str(tmp_path / "plain.bin"), how="markdup", with_dup=True)
    got, brc, _ = _finish(ctx, s["runs"], order, str(tmp_path / "armed.bin"), arm, "markdup", with_dup=True)
    assert got == plain, f"{n_runs} runs: the members changed"
    written = bgzf_ref.inflate(got)
    assert written == b"".join(s["marked"]) and s["marked"] != s["unmarked"]
    want, want_unmarked = ref.build(s["marked"], *arm), ref.build(s["unmarked"], *arm)     # the judge over the written file's records
    assert ref.parse(want)["n_records"] < ref.parse(want_unmarked)["n_records"] and ref.parse(want)["n_bases"] > 1000
    _same(brc, want, f"{n_runs} runs added as {order}, marked")
    _, brc, _ = _finish(ctx, s["runs"], order, str(tmp_path / "unmarked.bin"), arm, "finish", with_dup=True)
    _same(brc, want_unmarked, f"{n_runs} runs, the unmarked finish of the same runs")


def test_marking_index_qc_pileup_and_recal_in_one_finish(ctx, tmp_path):
    """One resident finish with marking, the index, the QC summary, the pileup and the recalibration table all armed writes the members and the
    four files that the same merger writes with each product armed alone, and the table is the judge's on the marked records."""
    s = _marked_set(n_tmpl=1250, seed=33, indexable=True)
    lens, pac, mask = s["lens"], s["pac"], s["mask"]
    qc_opt, pu_opt, rc_opt, base = (8, 0x400, 0), (0, 15, 0x400, 2), (0, 10, -1, 0), 4321
    paths = [str(tmp_path / x) for x in ("m.bin", "m.bai", "m.bqc", "m.bpu", "m.brc")]

    def finish(m, index, qc, pileup, recal):
        fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths]
        try:
            m.set_qc(lens, fds[2], qc_opt) if qc else m.set_qc(None)
            m.set_pileup(lens, pac, fds[3], pu_opt) if pileup else m.set_pileup(None)
            m.set_recal(lens, pac, mask, fds[4], rc_opt) if recal else m.set_recal(None)
            m.finish_markdup(fds[0], fds[1], base, mcases.N_SEQS if index else -1)
        finally:
            for fd in fds:
                os.close(fd)
        return [open(p, "rb").read() for p in paths]

    with bw.DevMerger(ctx, 1) as m:
        for k in (1, 2, 0):
            m.add_dup(k, *s["runs"][k])
        alone = [finish(m, *(j == k for j in range(1, 5))) for k in range(5)]
        every = finish(m, True, True, True, True)
        for k, part in enumerate(("members", "index", "QC summary", "pileup", "recalibration table")):
            assert [bool(x) for x in alone[k]] == [True] + [j == k for j in range(1, 5)], part
            assert every[k] == alone[k][k], f"all armed: the {part} differs from the one the merger writes with it armed alone"
            assert alone[k][0] == every[0], part
        again = finish(m, False, False, False, True)
        assert again[4] == every[4] and again[0] == every[0] and again[1] == again[2] == again[3] == b"", "the others disarmed, the table still armed"
    assert bgzf_ref.inflate(every[0]) == b"".join(s["marked"]) and s["marked"] != s["unmarked"]
    assert every[2] == qc_ref.build(s["marked"], lens, qc_opt) and every[3] == pileup_ref.build(s["marked"], lens, pac, pu_opt)
    _same(every[4], ref.build(s["marked"], lens, pac, mask, rc_opt), "all armed")
    assert ref.parse(every[4])["n_bases"] > 1000                                           # (the input is no empty one)


@pytest.mark.parametrize("n_runs", [3, 7])
def test_resident_and_spilled_runs_give_the_same_table(ctx, case, tmp_path, n_runs):
    """Small windows (piece_blocks 1, window_pieces 1 and 2: a window of one or two BGZF blocks) over any mix of resident and spilled
    runs: the members and the table are those of the merger with every run resident, and the table is the judge's."""
    rng = random.Random(n_runs)
    runs = [sref.run_arrays(r, _key) for r in sref.make_runs(case["records"], n_runs, rng, empty=1)]
    order = list(range(n_runs))
    rng.shuffle(order)
    arm = (case["ref_len"], case["pac"], case["mask"], ())
    out = str(tmp_path / "m.bin")
    members, brc0, _ = _finish(ctx, runs, order, out, arm)
    _same(brc0, case["want"][((), True)], "every run resident")
    for spilled in (set(range(n_runs)), set(range(1, n_runs, 2)), {n_runs - 1}):
        for wp in (1, 2):
            what = f"{n_runs} runs added as {order}, spilled {sorted(spilled)}, window_pieces {wp}"
            got, brc, rs = _finish(ctx, runs, order, out, arm, spilled=spilled, wp=wp)
            assert got == members, what + ": the members changed"
            _same(brc, case["want"][((), True)], what)
            assert rs.n_records == ref.parse(brc)["n_records"], what
    # a refusal over spilled runs follows the members
    got, brc, _ = _finish(ctx, runs, order, out, spilled={0}, wp=1)
    assert got == members and brc == b""
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 1) as m:
            m.set_spill(1 << 30, None, 1)
            m.set_recal(case["ref_len"], case["pac"], None, fd, (0, 0, -1, cases.MAX_CYCLE))   # after set_spill as well
            for k in order:
                m.add_spilled(k, *runs[k]) if k == 0 else m.add(k, *runs[k])
            with pytest.raises(bw.BwahipError, match="ECAPACITY"):
                m.finish(fd)
            assert os.fstat(fd).st_size == len(members)
    finally:
        os.close(fd)


def test_marked_finish_over_spilled_runs_gives_the_resident_table(ctx, tmp_path):
    s = _marked_set(n_tmpl=1250, seed=33)
    arm = (s["lens"], s["pac"], s["mask"], ())
    order = [1, 2, 0]
    out = str(tmp_path / "m.bin")
    members, brc0, _ = _finish(ctx, s["runs"], order, out, arm, "markdup", with_dup=True)
    _same(brc0, ref.build(s["marked"], *arm), "every run resident")
    for spilled in ({0, 1, 2}, {1}):
        got, brc, _ = _finish(ctx, s["runs"], order, out, arm, "markdup", with_dup=True, spilled=spilled, wp=1)
        assert got == members and brc == brc0, f"spilled {sorted(spilled)}: {ref.first_difference(brc, brc0)}"


def test_the_stage_gives_back_what_it_took(ctx, case, tmp_path):
    """bwahip_live_resources before and after the stage alone, an armed merger and a refusal: what the context itself keeps from call to call
    (its sort and scan buffers) has its size after the first round."""
    runs = [sref.run_arrays(r, _key) for r in sref.make_runs(case["records"], 3, random.Random(3))]
    arm = (case["ref_len"], case["pac"], case["mask"], ())

    def round_():
        _same(_kat(ctx, case), case["want"][((), True)], "the stage alone")
        with pytest.raises(bw.BwahipError, match="ECAPACITY"):
            _kat(ctx, case, (0, 0, -1, cases.MAX_CYCLE))
        _, brc, _ = _finish(ctx, runs, [2, 0, 1], str(tmp_path / "m.bin"), arm, spilled={1}, wp=2)
        _same(brc, case["want"][((), True)], "the armed merger")

    round_()
    before = bw.live_resources()
    round_()
    assert bw.live_resources() == before


# ---------------------------------------------------------------------------------------------------------------- 3. the stream driver
K = 300 * 2 * 150
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"
LIBS = ("mid_insert", "rf", "mixed4", "edges")


@pytest.fixture(scope="module")
def stream_case(built, tmp_path_factory):
    """The case of tests/test_gpu_pileup.py: four of the committed paired-end libraries over the suite's 1 Mb genome (300 pairs each), then
    the first 100 pairs once more under other names, so that marking finds duplicates: five batches."""
    d = tmp_path_factory.mktemp("rc_stream")
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
    fd, fb, fq, fr = (os.open(out + x, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for x in ("", ".bai", ".bqc", ".brc"))
    try:
        extra = dict(rc_fd=fr) if "recal" in kw else {}
        res = fn(ctxs, sc["fq1"], sc["fq2"], fd, fb if index else -1, fq, hdr_line=HDR, opt=opt, chunk_bases=K, reader_threads=2, hbm_budget=hbm_budget, **extra, **kw)
    finally:
        for x in (fd, fb, fq, fr):
            os.close(x)
    return [open(out + x, "rb").read() for x in ("", ".bai", ".bqc", ".brc")], res


@pytest.mark.parametrize("markdup", [1, 0])
@pytest.mark.parametrize("n_ctx", [1, 2])
def test_stream_driver_writes_the_table_of_the_file(small_index, stream_case, tmp_path, n_ctx, markdup):
    qc_opt = (8, -1, 0)
    rc_opt = (0, 13, -1, 0) if markdup else (20, 0, 0, 300)
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            bns = bw.lib().bwahip_bns(c0._h).contents
            lens = [bns.anns[i].len for i in range(bns.n_seqs)]
            pac = open(small_index["prefix"] + ".pac", "rb").read()[:(sum(lens) + 3) // 4]
            rng = random.Random(9)
            mask = ref.make_mask(sum(lens), {g for g in range(sum(lens)) if rng.random() < 0.01}) if markdup else None
            what = f"n_ctx {n_ctx}, markdup {markdup}"
            (bam0, bai0, qc0, none), res0 = _stream(bw.stream_run_bam_sorted_dev_spill, ctxs, stream_case, tmp_path, qc=qc_opt, markdup=markdup)
            assert none == b"" and res0[1].fell_back == 0 and res0[0].n_batches == 5 and res0[0].n_reads == 2600, what
            (bam, bai, qc, brc), (st, sd, sp, ms, qs, rs) = _stream(bw.stream_run_bam_sorted_dev_recal, ctxs, stream_case, tmp_path, qc=qc_opt, markdup=markdup, recal=rc_opt,
                                                                     mask=mask)
            assert bam == bam0 and bai == bai0 and qc == qc0 and sd.fell_back == 0, what + ": the file, its index or its summary changed"
            n_ref, recs, _, _ = bai_ref.split_file(bam)
            assert n_ref == len(lens) and len(recs) >= 2600
            _same(brc, ref.build(recs, lens, pac, mask, rc_opt), what)
            s = ref.parse(brc)
            assert s["n_bases"] > 100000 and s["n_err"] > 100 and (s["n_masked"] > 100) == bool(markdup) and rs.rc_bytes == len(brc) and rs.n_records == s["n_records"], what
            assert rs.hbm_bytes > 0 and rs.recal_ms > 0 and (ms.n_marked > 0) == bool(markdup), what
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # bad options: before anything starts
                _stream(bw.stream_run_bam_sorted_dev_recal, ctxs, stream_case, tmp_path, markdup=markdup, recal=(0, 94, -1, 0))
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # no options at all
                _stream(bw.stream_run_bam_sorted_dev_recal, ctxs, stream_case, tmp_path, markdup=markdup, recal=None)
        finally:
            for c in ctxs[1:]:
                c.close()


@pytest.mark.parametrize("with_mask", [False, True])
def test_stream_driver_budget_counts_the_table_to_the_byte(small_index, stream_case, tmp_path, with_mask):
    """The spilling entry point's HBM budget at its boundary: the merger's need for all five runs resident, one window of staging reserved,
    plus bwahip_recal_hbm_need -- the mask's bytes in it or not -- is a budget under which no run is spilled; one byte less and the last run
    is held spilled, and the file and the table are still the resident run's."""
    pb, wp = 1, 2
    with bw.Context(small_index["prefix"]) as c0:
        bns = bw.lib().bwahip_bns(c0._h).contents
        l_pac = sum(bns.anns[i].len for i in range(bns.n_seqs))
        assert l_pac == bns.l_pac
        rng = random.Random(9)
        mask = ref.make_mask(l_pac, {g for g in range(l_pac) if rng.random() < 0.01}) if with_mask else None
        kw = dict(index=False, qc=None, markdup=0, recal=(20, 0, 0, 0), mask=mask, piece_blocks=pb, window_pieces=wp, host_budget=1 << 30)
        files0, (st, sd, sp, _, _, rs) = _stream(bw.stream_run_bam_sorted_dev_recal, [c0], stream_case, tmp_path, **kw)
        raw, n_rec, n_runs = sd.dev.raw_bytes, sd.dev.n_records, sd.dev.n_runs
        assert sp.n_spilled_runs == 0 and n_runs == 5 and n_rec >= 2600 and files0[3] and files0[1] == files0[2] == b""
        need = bw.bam_devmerge_spill_hbm_need(raw, wp * pb * 65280, 0, n_rec, n_runs, pb, wp) + bw.recal_hbm_need(l_pac, 0, with_mask)
        print(f"mask {with_mask}: raw {raw}, records {n_rec}, runs {n_runs}, need {need}, of it the table's {bw.recal_hbm_need(l_pac, 0, with_mask)}")
        files, (_, sd, sp, _, _, _) = _stream(bw.stream_run_bam_sorted_dev_recal, [c0], stream_case, tmp_path, hbm_budget=need, **kw)
        assert sp.n_spilled_runs == 0 and sd.fell_back == 0 and files == files0, "a budget of exactly the need"
        files, (_, sd, sp, _, _, _) = _stream(bw.stream_run_bam_sorted_dev_recal, [c0], stream_case, tmp_path, hbm_budget=need - 1, **kw)
        assert sp.n_spilled_runs >= 1 and sd.fell_back == 0 and files == files0, "one byte less: the file or the table changed, or nothing was spilled"
