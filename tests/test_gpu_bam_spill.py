"""A device merger whose runs' record bytes outgrow HBM (csrc/k_bamspill.hip, csrc/spill_store.cpp): spilled runs keep their record bytes in
a host-side store and every finish stages them window by window.  For any mix of resident and spilled runs the members, the index, the QC
summary and the counts must be those of a merger with all runs resident.  The judges are the Python restatements the other merger tests
use -- bam_sort_ref's stable sort, bgzf_ref / gzip on what came out, markdup_ref, bai_ref, qc_ref -- with Context.kat_bgzf (the deflate stage
alone) for the member bytes; the all-resident finish is a second, cheaper witness.  Byte for byte, no tolerance.

Shapes: records of 200 to 400 bytes, a few thousand in all, so that piece_blocks 1 and window_pieces 1 cut the stream into a dozen
windows; the duplicate-marking sets keep the record sizes markdup_cases gives them (about 120 bytes)."""
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
import markdup_cases as mcases
import markdup_ref as mref
import qc_ref
from common import bw

pytestmark = pytest.mark.gpu

BLOCK = 65280
N_SEQS, LONGEST = 5, 2 ** 31 - 1
SHAPES = [(pb, wp) for pb in (1, 3) for wp in (1, 2, 65536)]
SUBSETS = ("all", "odd", "last")


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


def _key(rec):
    return sref.packed_key(rec, N_SEQS, LONGEST)


def _rec(length, ref_id, pos, rev, rng):
    """An arbitrary byte string of `length` >= 20 bytes whose first 20 carry what bam_sort_ref reads: refID, pos, flag."""
    head = struct.pack("<iiiBBHHH", length - 4, ref_id, pos, 1, 0, 0, 0, 0x10 if rev else 0)
    body = bytes(rng.choices(b"ACGT", k=length - 20)) if length < 60000 else rng.randbytes(length - 20)
    return head + body


def _subset(name, n_runs):
    return {"all": set(range(n_runs)), "odd": set(range(1, n_runs, 2)), "last": {n_runs - 1}}[name]


def _merge(ctx, runs, order, spilled, pb, wp, path, host_budget=1 << 30, tmp_dir=None, twice=False):
    """runs: list of add() tuples (or add_dup() tuples); run k is held spilled when k is in `spilled`.  Returns the members, the
    DevMergeStats and the SpillStats; twice: a second finish must write the same bytes again."""
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, pb) as m:
            m.set_spill(host_budget, tmp_dir, wp)
            for k in order:
                m.add_spilled(k, *runs[k]) if k in spilled else (m.add_dup(k, *runs[k]) if len(runs[k]) == 5 else m.add(k, *runs[k]))
            st = m.finish(fd)
            sp = m.spill_stats()
            first = os.fstat(fd).st_size
            if twice:
                m.finish(fd)
    finally:
        os.close(fd)
    got = open(path, "rb").read()
    if twice:
        assert got[first:] == got[:first], "the second finish wrote other bytes"
    return got[:first], st, sp


def _counts(st):
    return st.n_records, st.n_runs, st.raw_bytes, st.bgzf_bytes, st.n_blocks, st.n_stored


# ---------------------------------------------------------------------------------------------------------------- 1. cuts, windows, subsets
@pytest.fixture(scope="module")
def plain(ctx):
    rng = random.Random(77)
    recs = [_rec(rng.randrange(200, 401), rng.choice((0, 1, 2, 3, -1)), rng.randrange(0, 3000), rng.random() < 0.5, rng) for _ in range(2400)]
    want = b"".join(sref.stable_sort(recs))
    members, n_blocks, _ = ctx.kat_bgzf(want)
    assert bgzf_ref.inflate(members) == want and n_blocks == (len(want) + BLOCK - 1) // BLOCK >= 10
    return dict(recs=recs, want=want, members=members, n_blocks=n_blocks)


@pytest.mark.parametrize("n_runs", [1, 3, 7])
def test_members_for_every_cut_window_and_subset(ctx, plain, tmp_path, n_runs):
    rng = random.Random(n_runs)
    runs = sref.make_runs(plain["recs"], n_runs, rng, empty=1 if n_runs > 1 else None)   # run 1 is empty: spilled in "all" and "odd"
    arrays = [sref.run_arrays(r, _key) for r in runs]
    order = list(range(n_runs))
    rng.shuffle(order)
    out = str(tmp_path / "m.bin")
    resident, st0, sp0 = _merge(ctx, arrays, order, set(), 1, 1, out)
    assert resident == plain["members"] and sp0.n_spilled_runs == 0 and sp0.first_spilled_run == -1 and sp0.n_windows == 0
    for name in SUBSETS:
        spilled = _subset(name, n_runs)
        for pb, wp in SHAPES:
            what = f"{n_runs} runs added as {order}, spilled {sorted(spilled)}, piece_blocks {pb}, window_pieces {wp}"
            got, st, sp = _merge(ctx, arrays, order, spilled, pb, wp, out, twice=True)
            assert bgzf_ref.inflate(got) == plain["want"], what
            assert got == plain["members"], what + ": not the deflate stage's members of the sorted records"
            assert _counts(st) == _counts(st0), what
            n_pieces = (plain["n_blocks"] + pb - 1) // pb
            sp_bytes = sum(len(arrays[k][0]) for k in spilled)
            assert (sp.n_spilled_runs, sp.first_spilled_run) == (len(spilled), min(spilled) if spilled else -1), what
            assert sp.host_bytes == sp_bytes and sp.file_bytes == 0 and sp.n_windows == (n_pieces + wp - 1) // wp * bool(spilled), what
            assert not spilled or sp.window_hbm_bytes > 0, what


# ---------------------------------------------------------------------------------------------------------------- 2. where the store puts a run
def test_store_placement_does_not_change_the_bytes(ctx, plain, tmp_path):
    rng = random.Random(12)
    arrays = [sref.run_arrays(r, _key) for r in sref.make_runs(plain["recs"], 3, rng)]
    sizes = sorted(len(a[0]) for a in arrays)
    assert sizes[0] < sizes[1]
    d = tmp_path / "spill"
    d.mkdir()
    total = sum(sizes)
    for budget, in_mem in ((1 << 30, total), (0, 0), ((sizes[0] + sizes[1]) // 2, sizes[0])):   # the last: only the smallest run fits
        for pb, wp in ((1, 1), (3, 2)):
            what = f"host_budget {budget}, piece_blocks {pb}, window_pieces {wp}"
            got, st, sp = _merge(ctx, arrays, [2, 0, 1], {0, 1, 2}, pb, wp, str(tmp_path / "m.bin"), budget, str(d), twice=True)
            assert got == plain["members"], what
            assert (sp.host_bytes, sp.file_bytes) == (in_mem, total - in_mem) and sp.host_bytes + sp.file_bytes == st.raw_bytes, what
            assert os.listdir(d) == [], what + ": a file was left behind"


# ---------------------------------------------------------------------------------------------------------------- 3. ties
def test_a_tie_block_longer_than_three_windows_keeps_run_then_position(ctx, tmp_path):
    rng = random.Random(3)
    runs = []
    for k in range(5):
        mapped = [_rec(rng.randrange(200, 401), rng.choice((0, 1)), rng.randrange(0, 500), False, rng) for _ in range(40)]
        tail = [_rec(rng.randrange(200, 401), -1, -1, False, rng) for _ in range(rng.randrange(320, 380))]   # one key: the unmapped tail
        runs.append(sref.stable_sort(mapped) + tail)
    n_tail = sum(len(r) for run in runs for r in run if struct.unpack_from("<i", r, 4)[0] < 0)
    assert n_tail > 3 * 2 * BLOCK and len({bytes(r) for run in runs for r in run}) == sum(map(len, runs))
    want = b"".join(sref.stable_sort([r for run in runs for r in run]))                   # stable over run order = (key, run_no, position)
    arrays = [sref.run_arrays(r, _key) for r in runs]
    members = ctx.kat_bgzf(want)[0]
    for spilled in ({0, 1, 2, 3, 4}, {1, 3}, {4}):
        for pb, wp in ((1, 1), (1, 2)):
            got, _, sp = _merge(ctx, arrays, [3, 0, 4, 2, 1], spilled, pb, wp, str(tmp_path / "t.bin"))
            assert bgzf_ref.inflate(got) == want and got == members, f"spilled {sorted(spilled)}, window_pieces {wp}"
            assert sp.n_windows >= 8 // wp


# ---------------------------------------------------------------------------------------------------------------- 4. a record longer than a window
def test_a_record_that_spans_three_windows(ctx, tmp_path):
    rng = random.Random(4)
    recs = [_rec(rng.randrange(200, 401), 0, rng.randrange(0, 200), False, rng) for _ in range(400)]
    recs.append(_rec(140000, 0, 100, False, rng))
    rng.shuffle(recs)
    want_recs = sref.stable_sort(recs)
    off = np.concatenate(([0], np.cumsum([len(r) for r in want_recs])))
    at = [len(r) for r in want_recs].index(140000)
    assert off[at + 1] // BLOCK - off[at] // BLOCK >= 2 and off[at] > 0 and off[at + 1] < off[-1]   # in three windows of one block, records on both sides
    want = b"".join(want_recs)
    members = ctx.kat_bgzf(want)[0]
    runs = sref.make_runs(recs, 3, rng)
    arrays = [sref.run_arrays(r, _key) for r in runs]
    for spilled in ({0, 1, 2}, {1}, {0, 2}):
        got, st, sp = _merge(ctx, arrays, [1, 2, 0], spilled, 1, 1, str(tmp_path / "l.bin"), twice=True)
        assert bgzf_ref.inflate(got) == want and got == members, f"spilled {sorted(spilled)}"
        assert sp.n_windows == st.n_blocks >= 4


# ---------------------------------------------------------------------------------------------------------------- 5. all sidecars
QC_LENS = [5000, 100000, 1000, 3000, 64]                                                  # markdup_cases' five references
QC_OPT = (8, 0x400, 0)


def _bam_header(n_ref):
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for k in range(n_ref):
        name = b"c%d\0" % k
        out += struct.pack("<i", len(name)) + name + struct.pack("<i", 1 << 29)
    return out


def _indexable(rec):
    try:
        return bai_ref.fields(rec, N_SEQS)[2] <= bai_ref.MAX_END
    except Exception:
        return False


@pytest.fixture(scope="module")
def marked_sets(ctx, tmp_path_factory):
    """Per paired / single-end: the runs' add_dup tuples, and every judge's answer, made once."""
    d = tmp_path_factory.mktemp("spill_sidecars")
    hdr_path = str(d / "hdr.bgzf")
    fd = os.open(hdr_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    bw.bgzf_write(fd, _bam_header(N_SEQS), 1, 1)
    os.close(fd)
    hdr = open(hdr_path, "rb").read()
    out = {}
    for paired in (True, False):
        c = mcases.record_set(paired, n_tmpl=1500, seed=9)
        c["templates"] = [t for t in c["templates"] if all(_indexable(x) for r in t[1] for x in r)]   # the set also holds records BAI cannot index
        c["names"], c["reads"] = [n for n, _ in c["templates"]], [r for _, rr in c["templates"] for r in rr]
        assert len(c["names"]) > 1300
        descs = mcases.judge_descs(c)
        rng = random.Random(5 + paired)
        n, n_runs = len(c["templates"]), 3
        b = [0] + sorted(rng.sample(range(1, n), n_runs - 1)) + [n]
        key_of = lambda r: sref.packed_key(r, mcases.N_SEQS, mcases.LONGEST)
        runs = []
        for k in range(n_runs):
            recs = [(x, t) for t, (_, reads) in enumerate(c["templates"][b[k]:b[k + 1]]) for r in reads for x in r]
            recs.sort(key=lambda p: sref.order_key(p[0]))
            runs.append((*sref.run_arrays([x for x, _ in recs], key_of), np.array([t for _, t in recs], dtype=np.uint32), mcases.as_desc_array(descs[b[k]:b[k + 1]])))
        unmarked = sref.stable_sort([x for r in c["reads"] for x in r])
        j = mref.mark(unmarked, c["names"], paired)
        marked = b"".join(j["records"])
        members = ctx.kat_bgzf(marked)[0]
        assert bgzf_ref.inflate(members) == marked and j["stats"][2] > 20 and len(marked) > 3 * BLOCK
        file = hdr + members + bgzf_ref.EOF_BLOCK
        n_ref, in_file, offs, base = bai_ref.split_file(file)
        bai = bai_ref.from_file(file)
        assert n_ref == N_SEQS and base == len(hdr) and in_file == j["records"] and bai_ref.check_semantics(bai, in_file, offs, n_ref) > 100
        out[paired] = dict(runs=runs, members=members, bai=bai, qc=qc_ref.build(j["records"], QC_LENS, QC_OPT), judge=j, base=len(hdr), n_rec=len(unmarked), n_tmpl=n,
                           longest=max(map(len, unmarked)), raw=len(marked))
    return out


def _finish_all(ctx, s, spilled, pb, wp, d, host_budget=1 << 30):
    paths = [os.path.join(d, n) for n in ("m.bin", "m.bai", "m.bqc")]
    fd, fb, fq = (os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths)
    try:
        with bw.DevMerger(ctx, pb) as m:
            m.set_spill(host_budget, d, wp)
            for k in (2, 0, 1):
                m.add_spilled(k, *s["runs"][k]) if k in spilled else m.add_dup(k, *s["runs"][k])
            qs = m.set_qc(QC_LENS, fq, QC_OPT)
            st, bs, ms = m.finish_markdup(fd, fb, s["base"], N_SEQS)
            sp = m.spill_stats()
    finally:
        for x in (fd, fb, fq):
            os.close(x)
    return [open(p, "rb").read() for p in paths], (st, bs, ms, qs, sp)


@pytest.mark.parametrize("paired", [True, False])
def test_marking_index_and_qc_over_spilled_runs(ctx, marked_sets, tmp_path, paired):
    s = marked_sets[paired]
    (mem0, bai0, qc0), (st0, bs0, ms0, qs0, _) = _finish_all(ctx, s, set(), 1, 1, str(tmp_path))
    assert mem0 == s["members"] and bai0 == s["bai"] and qc0 == s["qc"], "the all-resident finish is not the judges'"
    n_kind, n_dup, n_marked = s["judge"]["stats"]
    for spilled in ({0, 1, 2}, {1}, {2}):
        for pb, wp in SHAPES:
            for budget in ((1 << 30,) if (pb, wp) != (1, 1) else (1 << 30, 0)):            # the smallest shape also from files
                what = f"paired {paired}, spilled {sorted(spilled)}, piece_blocks {pb}, window_pieces {wp}, host_budget {budget}"
                (mem, bai, qc), (st, bs, ms, qs, sp) = _finish_all(ctx, s, spilled, pb, wp, str(tmp_path), budget)
                assert mem == s["members"], what + ": members"
                assert bai == s["bai"], what + ": index"
                assert qc == s["qc"], what + ": " + qc_ref.first_difference(qc, s["qc"])
                assert _counts(st) == _counts(st0), what
                assert (bs.n_chunks, bs.n_windows, bs.n_no_coor) == (bs0.n_chunks, bs0.n_windows, bs0.n_no_coor), what
                assert (list(ms.n_templates), list(ms.n_dup_templates), ms.n_marked) == (list(ms0.n_templates), list(ms0.n_dup_templates), ms0.n_marked) == (n_kind, n_dup, n_marked), what
                cnt = qc_ref.parse(qc)["count"]
                assert cnt[0][0] + cnt[1][0] == s["n_rec"] == st.n_records, what + ": a straddling record counted twice, or not at all"
                sp_raw = sum(len(s["runs"][k][0]) for k in spilled)
                need = (bw.bam_devmerge_spill_hbm_need(s["raw"] - sp_raw, sp_raw, s["longest"], s["n_rec"], 3, pb, wp) + bw.bam_devmerge_bai_hbm_need(s["n_rec"], st.n_blocks, N_SEQS, bs.n_windows) +
                        bw.bam_devmerge_markdup_hbm_need(s["n_rec"], s["n_tmpl"]) + bw.qc_hbm_need(N_SEQS, sum(QC_LENS), qs.n_windows, s["n_rec"]))
                assert st.hbm_bytes + bs.hbm_bytes + ms.hbm_bytes + qs.hbm_bytes + sp.window_hbm_bytes <= need, what
                assert sorted(os.listdir(tmp_path)) == ["m.bai", "m.bin", "m.bqc"], what + ": a file of the store was left behind"


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_merger_usable(ctx, plain, marked_sets, tmp_path):
    runs = sref.make_runs(plain["recs"], 3, random.Random(8))
    arrays = [sref.run_arrays(r, _key) for r in runs]
    not_a_dir = tmp_path / "file"
    not_a_dir.write_bytes(b"x")
    out = str(tmp_path / "m.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 1) as m:
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # unarmed
                m.add_spilled(0, *arrays[0])
            for bad in (dict(window_pieces=65537), dict(host_budget=-1)):
                with pytest.raises(bw.BwahipError, match="EINVAL"):
                    m.set_spill(**bad)
            m.add(0, *arrays[0])
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # after an add
                m.set_spill(1 << 30, None, 1)
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                m.add_spilled(1, *arrays[1])
            m.add(1, *arrays[1])
            m.add(2, *arrays[2])
            m.finish(fd)
        assert open(out, "rb").read() == plain["members"]
        os.ftruncate(fd, 0)
        os.lseek(fd, 0, os.SEEK_SET)
        for tmp_dir in (None, str(not_a_dir), str(tmp_path / "missing")):
            with bw.DevMerger(ctx, 1) as m:
                m.set_spill(0, tmp_dir, 1)                                                 # every spilled run needs a file
                with pytest.raises(bw.BwahipError, match="EIO"):
                    m.add_spilled(0, *arrays[0])
                m.add_spilled(3, b"", np.zeros(0, dtype=np.uint64), np.zeros(1, dtype=np.int64))   # no bytes: no file
                assert m.finish(-1).n_records == 0 and m.spill_stats().n_spilled_runs == 1
                for k in (2, 0, 1):                                                        # the refused run number is free, the merger takes the runs resident
                    m.add(k, *arrays[k])
                st = m.finish(fd)
                sp = m.spill_stats()
                assert (st.n_runs, st.n_records, sp.n_spilled_runs, sp.host_bytes, sp.file_bytes) == (4, len(plain["recs"]), 1, 0, 0)
            assert open(out, "rb").read() == plain["members"], f"after the refusal with tmp_dir {tmp_dir}"
            os.ftruncate(fd, 0)
            os.lseek(fd, 0, os.SEEK_SET)
            with bw.DevMerger(ctx, 1) as m:
                m.set_spill(len(arrays[1][0]), tmp_dir, 2)                                 # run 1 fits the memory, the next spilled run needs a file
                m.add_spilled(1, *arrays[1])
                with pytest.raises(bw.BwahipError, match="EIO"):
                    m.add_spilled(0, *arrays[0])
                assert m.spill_stats().host_bytes == len(arrays[1][0]) and m.spill_stats().n_spilled_runs == 1   # the store holds what it held
                m.add(0, *arrays[0])
                m.add(2, *arrays[2])
                assert m.finish(fd).n_runs == 3
            assert open(out, "rb").read() == plain["members"], f"a spilled and two resident runs after the refusal with tmp_dir {tmp_dir}"
            os.ftruncate(fd, 0)
            os.lseek(fd, 0, os.SEEK_SET)
        with bw.DevMerger(ctx, 1) as m:
            m.set_spill(1 << 30, None, 1)
            m.add(0, *arrays[0])
            m.add_spilled(2, *arrays[2])
            for no in (0, 2):
                with pytest.raises(bw.BwahipError, match="EINVAL"):                        # a run number given twice, across add and add_spilled
                    m.add_spilled(no, *arrays[1])
                with pytest.raises(bw.BwahipError, match="EINVAL"):
                    m.add(no, *arrays[1])
            rec, keys, off = arrays[1]
            bad = off.copy()
            bad[-1] -= 1
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # offsets that do not end at the run's length
                m.add_spilled(1, rec, keys, bad)
            bad = off.copy()
            bad[1], bad[2] = off[2], off[1]
            with pytest.raises(bw.BwahipError, match="EINVAL"):                            # offsets that decrease
                m.add_spilled(1, rec, keys, bad)
            assert m.spill_stats().host_bytes == len(arrays[2][0])                         # the store holds what it held
            m.add_spilled(1, rec, keys, off)
            st = m.finish(fd)
            assert st.n_runs == 3 and m.spill_stats().n_spilled_runs == 2
        assert open(out, "rb").read() == plain["members"]
    finally:
        os.close(fd)
    s = marked_sets[True]
    with bw.DevMerger(ctx, 1) as m:                                                        # a template index outside the run's descriptors, as add_dup refuses it
        m.set_spill(1 << 30, None, 1)
        m.add_spilled(0, *s["runs"][0])
        rec, keys, off, tmpl, desc = s["runs"][1]
        bad = tmpl.copy()
        bad[len(bad) // 2] = len(desc)
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            m.add_spilled(1, rec, keys, off, bad, desc)
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            m.add_spilled(1, rec, keys, off, tmpl, desc[:int(tmpl.max())])
        m.add_spilled(1, rec, keys, off, tmpl, desc)
        m.add_dup(2, *s["runs"][2])
        fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            st, _, ms = m.finish_markdup(fd)
        finally:
            os.close(fd)
        assert st.n_runs == 3 and ms.n_marked == s["judge"]["stats"][2] and open(out, "rb").read() == s["members"]
        m.add_spilled(3, *arrays[0])                                                       # a run without descriptors: the marked finish refuses, before a byte
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            m.finish_markdup(-1)


# ---------------------------------------------------------------------------------------------------------------- 7. finish after finish
LEAK_BASE = 4321                                                                        # any first_member_offset: both mergers get the same


@pytest.fixture(scope="module")
def leak_runs():
    """Three runs of about 1 000 records of 100 to 300 bytes with templates and descriptors: markdup_cases' paired templates, every record
    lengthened by a trailing Z tag (nothing the stages read), cut into runs as marked_sets cuts them."""
    c = mcases.record_set(True, n_tmpl=1250, seed=21)
    rng = random.Random(21)
    def pad(x):
        n = rng.randrange(max(len(x) + 4, 100), 301)
        x += b"XPZ" + b"p" * (n - len(x) - 4) + b"\0"
        return struct.pack("<i", len(x) - 4) + x[4:]
    c["templates"] = [(name, [[pad(x) for x in r] for r in rr]) for name, rr in c["templates"] if all(_indexable(x) for r in rr for x in r)]
    descs = mcases.judge_descs(c)
    n = len(c["templates"])
    b = [0, 3 * n // 10, 13 * n // 20, n]
    key_of = lambda r: sref.packed_key(r, mcases.N_SEQS, mcases.LONGEST)
    runs = []
    for k in range(3):
        recs = [(x, t) for t, (_, reads) in enumerate(c["templates"][b[k]:b[k + 1]]) for r in reads for x in r]
        recs.sort(key=lambda p: sref.order_key(p[0]))
        assert all(100 <= len(x) <= 300 for x, _ in recs) and len(recs) > 800
        runs.append((*sref.run_arrays([x for x, _ in recs], key_of), np.array([t for _, t in recs], dtype=np.uint32), mcases.as_desc_array(descs[b[k]:b[k + 1]])))
    assert 2500 < sum(len(r[1]) for r in runs) < 3800 and sum(len(r[0]) for r in runs) > 3 * BLOCK
    return runs


def _leak_merger(ctx, runs, spilled):
    m = bw.DevMerger(ctx, 1)
    m.set_spill(1 << 30, None, 1)
    for k in (1, 2, 0):
        m.add_spilled(k, *runs[k]) if spilled else m.add_dup(k, *runs[k])
    return m


def _leak_step(m, k, d):
    """Step k of the five finishes on merger m: the three files' bytes and every count the call reports."""
    paths = [os.path.join(d, n) for n in ("m.bin", "m.bai", "m.bqc")]
    fd, fb, fq = (os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths)
    bs = ms = qs = None
    try:
        if k == 0:
            st = m.finish(fd)
        elif k == 1:
            st, bs = m.finish_bai(fd, fb, LEAK_BASE, N_SEQS)
        elif k == 2:
            qs = m.set_qc(QC_LENS, fq, QC_OPT)
            st = m.finish(fd)
        elif k == 3:
            m.set_qc(None)
            st = m.finish(fd)
        else:
            st, bs, ms = m.finish_markdup(fd, fb, LEAK_BASE, N_SEQS)
        sp = m.spill_stats()
    finally:
        for x in (fd, fb, fq):
            os.close(x)
    counts = dict(dev=_counts(st), bai=bs and (bs.n_chunks, bs.n_windows, bs.n_no_coor), qc=qs and (qs.n_windows, qs.qc_bytes),
                  markdup=ms and (list(ms.n_templates), list(ms.n_dup_templates), ms.n_marked),
                  spill=(sp.n_spilled_runs, sp.first_spilled_run, sp.host_bytes, sp.file_bytes, sp.n_windows))
    return [open(p, "rb").read() for p in paths], counts


LEAK_STEPS = ("finish", "finish_bai", "set_qc, finish", "set_qc(None), finish", "finish_markdup with the index")


@pytest.mark.parametrize("spilled", [False, True])
def test_no_stage_state_leaks_from_one_finish_into_the_next(ctx, leak_runs, tmp_path, spilled):
    """One merger finished five times -- plain, indexed, armed, disarmed, marked and indexed -- writes at every step what a fresh merger
    with the same runs writes when that step is its only call (the marked finish last: it changes resident records in place)."""
    d_one, d_fresh = tmp_path / "one", tmp_path / "fresh"
    d_one.mkdir()
    d_fresh.mkdir()
    files = []
    with _leak_merger(ctx, leak_runs, spilled) as one:
        for k, name in enumerate(LEAK_STEPS):
            what = f"{'spilled' if spilled else 'resident'}, step {k + 1} ({name})"
            got, got_counts = _leak_step(one, k, str(d_one))
            with _leak_merger(ctx, leak_runs, spilled) as fresh:
                want, want_counts = _leak_step(fresh, k, str(d_fresh))
            for part, a, b in zip(("members", "index", "QC summary"), got, want):
                assert a == b, f"{what}: {part} differ from a fresh merger's ({len(a)} and {len(b)} bytes)"
            assert got_counts == want_counts, what
            files.append(got)
    n_pieces = (sum(len(r[0]) for r in leak_runs) + BLOCK - 1) // BLOCK
    assert n_pieces >= 3 and got_counts["spill"][4] == (n_pieces if spilled else 0)
    members, bai, qc = zip(*files)
    assert members[0] == members[1] == members[2] == members[3] != members[4] and got_counts["markdup"][2] > 0
    assert [bool(x) for x in bai] == [False, True, False, False, True] and [bool(x) for x in qc] == [False, False, True, False, False]


# ---------------------------------------------------------------------------------------------------------------- 8. the stream driver
K = 1800 * 150                                                                        # batches of 900 pairs (or 1800 single reads): three runs, or two
PER_BATCH = 1800
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"
STREAM_QC = (8, -1, 0)


def _oracle_sam(prefix, fqs, extra=()):
    out = subprocess.run([common.ORACLE, "mem", "-t", "8", *extra, prefix, *fqs], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    return b"".join(l + b"\n" for l in out.split(b"\n") if l and not l.startswith(b"@"))


def stream_input(fa, d):
    """The input of test_gpu_markdup.py's stream tests, rebuilt: 2150 pairs, then 60 pairs whose second mate is random bases (the first
    mate of 30 is that of an earlier pair), 300 copies of earlier pairs under new names with lower, higher and equal qualities, copies
    of the 60.  Returns (fq1, fq2, the templates' names in input order)."""
    fq1, fq2, x1, x2 = (os.path.join(d, n) for n in ("s_1.fq", "s_2.fq", "x_1.fq", "x_2.fq"))
    bw.make_reads(fa, fq1, fq2, 4300, 150, 10000, 2000, 500, 171)
    bw.make_reads(fa, x1, x2, 60, 150, 10000, 2000, 500, 172)
    n1, s1, q1 = bw.read_fastq(fq1)
    n2, s2, q2 = bw.read_fastq(fq2)
    _, sx, _ = bw.read_fastq(x1)
    assert len(n1) == 2150 and n1 == n2 and len(sx) == 30
    rng = random.Random(31)
    names, a, b = list(n1), list(zip(s1, q1)), list(zip(s2, q2))
    requal = lambda q, k: (q, bytes([q[0] - 20]) * len(q), q[:-1] + bytes([q[-1] + 1]))[k % 3]
    def add(name, m1, m2):
        names.append(name)
        a.append(m1)
        b.append(m2)
    half = []
    for k in range(60):
        first = a[100 + 7 * k] if k < 30 else (sx[k - 30], b"I" * len(sx[k - 30]))
        add(b"half%d" % k, first, (bytes(rng.choices(b"ACGT", k=150)), b"I" * 150))
        half.append(len(names) - 1)
    for k in range(300):
        o = rng.randrange(0, 2000)
        add(b"copy%d" % k, (a[o][0], requal(a[o][1], k)), (b[o][0], requal(b[o][1], k // 3)))
    for k, o in enumerate(half):
        add(b"halfcopy%d" % k, (a[o][0], requal(a[o][1], k)), (bytes(rng.choices(b"ACGT", k=150)), b"I" * 150))
    for path, reads in ((fq1, a), (fq2, b)):
        with open(path, "wb") as f:
            for n, (s, q) in zip(names, reads):
                f.write(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n")
    return fq1, fq2, names


@pytest.fixture(scope="module")
def stream_case(small_index, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("spill_stream"))
    fq1, fq2, names = stream_input(small_index["fa"], d)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = {}
    for pe in (True, False):
        recs = bam_ref.split_records(bam_ref.sam_to_bam_records(_oracle_sam(small_index["prefix"], [fq1, fq2] if pe else [fq1], ["-K", str(K)]), contigs))
        unmarked = sref.stable_sort(recs)
        j = mref.mark(unmarked, names, pe)
        want[pe] = dict(n_rec=len(recs), unmarked=b"".join(unmarked), marked=b"".join(j["records"]), judge=j)
    return dict(fq1=fq1, fq2=fq2, want=want, split={})


def _stream(fn, ctxs, case, pe, d, **kw):
    opt = bw.default_opt()
    opt.n_threads = 4
    out = os.path.join(d, "o.bam")
    fds = [os.open(out + x, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for x in ("", ".bai", ".bqc")]
    try:
        res = fn(ctxs, case["fq1"], case["fq2"] if pe else None, fds[0], fds[1], fds[2], hdr_line=HDR, opt=opt, chunk_bases=K, reader_threads=2, **kw)
    finally:
        for x in fds:
            os.close(x)
    return [open(out + x, "rb").read() for x in ("", ".bai", ".bqc")], res


def _want_file(c0, records_bytes, d):
    hdr_member = os.path.join(d, "hdr.bin")
    fd = os.open(hdr_member, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    bw.bgzf_write(fd, bw.bam_header_sorted(c0, HDR), 1, 1)
    os.close(fd)
    return open(hdr_member, "rb").read() + c0.kat_bgzf(records_bytes)[0] + bgzf_ref.EOF_BLOCK


def _lens(c0):
    bns = bw.lib().bwahip_bns(c0._h).contents
    return [bns.anns[i].len for i in range(bns.n_seqs)]


def _need(lens, res_raw, sp_raw, longest, n_rec, n_tmpl, n_runs, pb, wp, mark=True, bai=True, qc=True):
    """What the entry point counts against hbm_budget (include/bwahip.h)."""
    raw = res_raw + sp_raw
    need = bw.bam_devmerge_spill_hbm_need(res_raw, sp_raw, longest, n_rec, n_runs, pb, wp)
    if bai:
        need += bw.bam_devmerge_bai_hbm_need(n_rec, (raw + BLOCK - 1) // BLOCK, len(lens), sum((n + 16383) >> 14 for n in lens))
    if mark:
        need += bw.bam_devmerge_markdup_hbm_need(n_rec, n_tmpl)
    if qc:
        need += bw.qc_hbm_need(len(lens), sum(lens), sum((n + 255) >> 8 for n in lens), 0)
    return need


def _budget_for_a_split_after_run_0(lens, sd, n_reads, n_tmpl, longest, pb, wp, **stages):
    """Half-way between what the runs held at the end take when only run 0 is resident (the call must succeed) and what runs 0 and 1
    would take resident (run 1 must not fit): the runs' shares of bytes, records and templates are those of their reads."""
    raw, n_rec, n_runs = sd.dev.raw_bytes, sd.dev.n_records, sd.dev.n_runs
    f0, f1 = PER_BATCH / n_reads, min(1.0, 2 * PER_BATCH / n_reads)
    at_end = _need(lens, int(f0 * raw), raw - int(f0 * raw), longest, n_rec, n_tmpl, n_runs, pb, wp, **stages)
    two_resident = _need(lens, int(f1 * raw), wp * pb * BLOCK, 0, int(f1 * n_rec), int(f1 * n_tmpl), 2, pb, wp, **stages)
    assert two_resident - at_end > 100000, "the input leaves no room between the two"
    return (at_end + two_resident) // 2


@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("n_ctx", [1, 3])
def test_stream_driver_spills_after_the_first_run(small_index, stream_case, tmp_path, n_ctx, pe):
    w = stream_case["want"][pe]
    d = tmp_path / "spill"
    d.mkdir()
    what = f"n_ctx {n_ctx}, {'pe' if pe else 'se'}"
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            lens = _lens(c0)
            qc_marked = lambda ctxs, fq1, fq2, fd, fb, fq, **kw: bw.stream_run_bam_sorted_dev_qc(ctxs, fq1, fq2, fd, fb, fq, True, STREAM_QC, **kw)
            (bam0, bai0, qc0), (st0, sd0, ms0, qs0) = _stream(qc_marked, ctxs, stream_case, pe, str(tmp_path), hbm_budget=8 << 30, piece_blocks=1)
            n_runs = st0.n_batches
            assert sd0.fell_back == 0 and n_runs == (3 if pe else 2)
            longest = max(map(len, w["judge"]["records"]))
            budget = _budget_for_a_split_after_run_0(lens, sd0, st0.n_reads, 2570, longest, 1, 2)
            spill = lambda ctxs, fq1, fq2, fd, fb, fq, **kw: bw.stream_run_bam_sorted_dev_spill(ctxs, fq1, fq2, fd, fb, fq, True, STREAM_QC, **kw)
            (bam, bai, qc), (st, sd, sp, ms, qs) = _stream(spill, ctxs, stream_case, pe, str(tmp_path), hbm_budget=budget, piece_blocks=1, window_pieces=2,
                                                          host_budget=int(0.325 * sd0.dev.raw_bytes) if pe else 0, tmp_dir=str(d))   # pe: run 1 (35 % of the bytes) to a file, the shorter run 2 to memory
            assert (bam, bai, qc) == (bam0, bai0, qc0), what + ": not the files of the all-resident entry point"
            assert bam == _want_file(c0, w["marked"], str(tmp_path)), what + ": not header member + the deflate stage's members of the judge's marked records + EOF"
            n_ref, recs, offs, _ = bai_ref.split_file(bam)
            assert recs == w["judge"]["records"] and bai == bai_ref.from_file(bam) and qc == qc_ref.build(recs, lens, STREAM_QC), what
            assert (sp.first_spilled_run, sp.n_spilled_runs, sd.fell_back) == (1, n_runs - 1, 0) and sd.dev.n_runs == n_runs, what
            assert stream_case["split"].setdefault(pe, (sp.first_spilled_run, sp.n_spilled_runs)) == (sp.first_spilled_run, sp.n_spilled_runs), what + ": the split depends on n_ctx"
            assert (sp.host_bytes > 0) == pe and sp.file_bytes > 0 and 0 < sp.host_bytes + sp.file_bytes < sd.dev.raw_bytes and sp.n_windows == (sd.dev.n_blocks + 1) // 2, what
            assert os.listdir(d) == [], what
            n_kind, n_dup, n_marked = w["judge"]["stats"]
            assert (list(ms.n_templates), list(ms.n_dup_templates), ms.n_marked) == (n_kind, n_dup, n_marked) == (list(ms0.n_templates), list(ms0.n_dup_templates), ms0.n_marked), what
            assert (st.n_reads, sd.n_records, sd.dev.raw_bytes) == (st0.n_reads, w["n_rec"], len(w["marked"])), what
        finally:
            for c in ctxs[1:]:
                c.close()


def test_stream_driver_plain_form_and_a_budget_below_the_metadata(small_index, stream_case, tmp_path):
    w = stream_case["want"][True]
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0, c0.clone_on(0)]
        try:
            lens = _lens(c0)
            plain = lambda ctxs, fq1, fq2, fd, fb, fq, **kw: bw.stream_run_bam_sorted_dev(ctxs, fq1, fq2, fd, **kw)
            (bam0, _, _), (st0, sd0) = _stream(plain, ctxs, stream_case, True, str(tmp_path), hbm_budget=8 << 30, piece_blocks=1)
            assert sd0.fell_back == 0 and bam0 == _want_file(c0, w["unmarked"], str(tmp_path))
            budget = _budget_for_a_split_after_run_0(lens, sd0, st0.n_reads, 0, max(map(len, bam_ref.split_records(w["unmarked"]))), 1, 1, mark=False, bai=False, qc=False)
            spill = lambda ctxs, fq1, fq2, fd, fb, fq, **kw: bw.stream_run_bam_sorted_dev_spill(ctxs, fq1, fq2, fd, -1, -1, False, None, **kw)
            (bam, bai, qc), (st, sd, sp, ms, qs) = _stream(spill, ctxs, stream_case, True, str(tmp_path), hbm_budget=budget, piece_blocks=1, window_pieces=1, host_budget=1 << 30)
            assert bam == bam0 and bai == b"" and qc == b"" and (sp.first_spilled_run, sd.fell_back, ms.n_marked) == (1, 0, 0) and sp.file_bytes == 0
            full = lambda ctxs, fq1, fq2, fd, fb, fq, **kw: bw.stream_run_bam_sorted_dev_spill(ctxs, fq1, fq2, fd, fb, fq, True, STREAM_QC, **kw)
            with pytest.raises(bw.BwahipError, match="ECAPACITY"):                        # not even the metadata fits
                _stream(full, ctxs, stream_case, True, str(tmp_path), hbm_budget=1, host_budget=1 << 30)
            assert os.path.getsize(tmp_path / "o.bam") == 0, "something was written before the refusal"
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                _stream(full, ctxs, stream_case, True, str(tmp_path), hbm_budget=8 << 30, host_budget=-1)
        finally:
            ctxs[1].close()
