"""The BAI index built on the device (csrc/k_bai.hip): the stage alone on the synthetic set (Context.kat_bai), inside the device merger's
finish (DevMerger.finish_bai) and behind the two stream entry points.  The judges are tests/bai_ref.py -- the canonical bytes restated in
Python, and a reader by reg2bins and the linear index -- and the device-free builder (tests/test_bai_cpu.py judges that one).  Byte for
byte, no tolerance."""
import os
import random
import struct

import numpy as np
import pytest

import bai_cases as cases
import bai_ref
import bam_sort_ref as sref
import bgzf_ref
from bai_cases import M, rec
from common import bw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(built):
    out = []
    for whole in (False, True):
        c = cases.synthetic(whole)
        c["want"] = bai_ref.build(c["records"], c["offsets"], c["n_ref"])
        cases.assert_families(c, c["want"])
        out.append(c)
    return out


def _host(c, tmp_path):
    out = str(tmp_path / "host.bai")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.BaiBuilder(c["n_ref"], c["base"]) as b:
            b.add_records(c["buf"], c["rec_off"])
            b.add_members(c["lens"])
            b.finish(fd)
    finally:
        os.close(fd)
    return open(out, "rb").read()


def _kat(ctx, c):
    return ctx.kat_bai(c["buf"], c["rec_off"], c["lens"], c["base"], c["n_ref"])


# ---------------------------------------------------------------------------------------------------------------- 1. the stage alone
def test_stage_equals_the_judge_and_the_host_builder(ctx, sets, tmp_path):
    for c in sets:
        got = _kat(ctx, c)
        assert got == c["want"], f"total {c['total']}: not the canonical index"
        assert got == _host(c, tmp_path)
        assert bai_ref.check_semantics(got, c["records"], c["offsets"], c["n_ref"]) > 1000


def test_stage_no_record_one_record_and_offsets_that_do_not_start_at_zero(ctx, sets, tmp_path):
    c = cases.make_case([])
    assert _kat(ctx, c) == bai_ref.build([], c["offsets"], c["n_ref"]) == _host(c, tmp_path)
    for one in (rec(3, 77, [(10, M)]), rec(-1, -1, [], flag=4), rec(0, 16383, [(2, M)], size=2 * 65280)):
        c = cases.make_case([one])
        assert _kat(ctx, c) == bai_ref.build([one], c["offsets"], c["n_ref"]) == _host(c, tmp_path)
    c = sets[0]
    shifted = ctx.kat_bai(bytes(13) + c["buf"], c["rec_off"] + 13, c["lens"], c["base"], c["n_ref"])   # records at odd addresses
    assert shifted == c["want"]
    many_refs = cases.make_case(c["records"], seed=12, n_ref=70000)   # more references than one workgroup's threads, nearly all empty
    assert _kat(ctx, many_refs) == bai_ref.build(c["records"], many_refs["offsets"], 70000)


def test_stage_refusals(ctx):
    """The bad record first, then at least 300 KB of ordinary records: even a kernel that read beyond a record would stay inside the
    allocation.  An error code is expected and nothing else."""
    tail = cases.ordinary(300000, pos0=6000)
    assert sum(map(len, tail)) >= 300000
    raw = lambda n, ref=0, pos=5000: struct.pack("<iiiBBHHH", n - 4, ref, pos, 1, 0, 0, 0, 0) + bytes(n - 20)
    bad_size = bytearray(rec(0, 5000, [(10, M)]))
    bad_size[0] += 1
    long_cigar = bytearray(rec(0, 5000, [(10, M)]))
    struct.pack_into("<H", long_cigar, 16, 60000)
    long_name = bytearray(rec(0, 5000, [(10, M)]))
    long_name[12] = 255
    for bad in (raw(20), raw(35), bytes(bad_size), bytes(long_cigar), bytes(long_name), rec(cases.N_REF, 5000, [(10, M)]), rec(0, -1, [(10, M)])):
        c = cases.make_case([bad] + tail)
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            _kat(ctx, c)
    for recs, code in (([rec(0, 7000)] + tail, "EINVAL"),                                  # not in coordinate order
                       ([rec(1, 10)] + tail, "EINVAL"),
                       (tail + [rec(-1, -1, flag=4), rec(0, 1 << 20)], "EINVAL"),
                       (tail + [rec(0, (1 << 29) - 99, [(100, M)])], "ECAPACITY"),          # e = 2^29 + 1
                       ([rec(0, 10, [((1 << 28) - 1, M), ((1 << 28) - 1, M), (2, M)])] + tail, "ECAPACITY"),
                       (tail + [rec(0, (1 << 29) - 99, [(100, M)]), rec(0, 5)], "ECAPACITY"),   # the first offending record decides
                       (tail + [rec(0, 5), rec(0, (1 << 29) - 99, [(100, M)])], "EINVAL")):
        c = cases.make_case(recs)
        with pytest.raises(bai_ref.Refused, match=code):
            bai_ref.build(recs, c["offsets"], c["n_ref"])
        with pytest.raises(bw.BwahipError, match=code):
            _kat(ctx, c)
    c = cases.make_case(tail)
    with pytest.raises(bw.BwahipError, match="EINVAL"):                                    # members that are not those of the records
        ctx.kat_bai(c["buf"], c["rec_off"], c["lens"][:-1], c["base"], c["n_ref"])
    assert _kat(ctx, c) == bai_ref.build(tail, c["offsets"], c["n_ref"])                   # the context still works


def test_contig_table_beyond_bai(built):
    """A contig of more than 2^29 bases: the stream entry points ask bwahip_bai_check_contigs before anything starts."""
    anns = (bw.Ann * 2)()
    bns = bw.Bns()
    bns.n_seqs, bns.anns = 2, anns
    anns[0].len, anns[1].len = 1 << 29, 1000
    bw.bai_check_contigs(bns)
    anns[1].len = (1 << 29) + 1
    with pytest.raises(bw.BwahipError, match="ECAPACITY"):
        bw.bai_check_contigs(bns)


# ---------------------------------------------------------------------------------------------------------------- 2. inside the merger's finish
def _bam_header(n_ref):
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for k in range(n_ref):
        name = b"c%d\0" % k
        out += struct.pack("<i", len(name)) + name + struct.pack("<i", 1 << 29)
    return out


@pytest.fixture(scope="module")
def merge_case(ctx, sets, tmp_path_factory):
    """The synthetic records shuffled, the header's member, and what finish (without index) writes for them -- made once."""
    d = tmp_path_factory.mktemp("bai_merge")
    c = sets[0]
    recs = list(c["records"])
    random.Random(21).shuffle(recs)
    hdr_path = str(d / "hdr.bgzf")
    fd = os.open(hdr_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    bw.bgzf_write(fd, _bam_header(c["n_ref"]), 1, 1)
    os.close(fd)
    hdr = open(hdr_path, "rb").read()
    key_of = lambda r: sref.packed_key(r, cases.N_REF, 2 ** 31 - 1)
    out = str(d / "plain.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    with bw.DevMerger(ctx, 2) as m:
        m.add(0, *sref.run_arrays(sref.stable_sort(recs), key_of))
        m.finish(fd)
    os.close(fd)
    members = open(out, "rb").read()
    assert bgzf_ref.inflate(members) == b"".join(sref.stable_sort(recs))
    want = bai_ref.from_file(hdr + members + bgzf_ref.EOF_BLOCK)
    n_ref, in_file, offs, base = bai_ref.split_file(hdr + members + bgzf_ref.EOF_BLOCK)
    assert n_ref == c["n_ref"] and base == len(hdr) and bai_ref.check_semantics(want, in_file, offs, n_ref) > 1000
    return dict(recs=recs, hdr=hdr, members=members, want=want, key_of=key_of, n_ref=c["n_ref"])


@pytest.mark.parametrize("n_runs", [1, 2, 7])
def test_finish_bai_for_every_piece_size_and_add_order(ctx, merge_case, tmp_path, n_runs):
    mc = merge_case
    rng = random.Random(n_runs)
    runs = sref.make_runs(mc["recs"], n_runs, rng, empty=3 if n_runs == 7 else None)
    assert n_runs != 7 or any(not r for r in runs)
    shuffled = list(range(n_runs))
    rng.shuffle(shuffled)
    out, bai = str(tmp_path / "members.bin"), str(tmp_path / "out.bai")
    for order in (list(range(n_runs)), list(range(n_runs))[::-1], shuffled):
        for pb in (1, 2, 3, 0):
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            fb = os.open(bai, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                with bw.DevMerger(ctx, pb) as m:
                    for k in order:
                        m.add(k, *sref.run_arrays(runs[k], mc["key_of"]))
                    st, bs = m.finish_bai(fd, fb, len(mc["hdr"]), mc["n_ref"])
            finally:
                os.close(fd)
                os.close(fb)
            what = f"{n_runs} runs added as {order}, piece_blocks {pb}"
            assert open(out, "rb").read() == mc["members"], what + ": not finish's members"
            got = open(bai, "rb").read()
            assert got == mc["want"], what + ": not the canonical index of header + members + EOF"
            assert (st.n_records, st.n_runs, st.bgzf_bytes) == (len(mc["recs"]), n_runs, len(mc["members"])), what
            assert bs.bai_bytes == len(got) and bs.n_no_coor == 3 and bs.n_chunks > 5 and bs.n_windows > 32768 and bs.hbm_bytes > 0, what


def test_finish_bai_edges(ctx, merge_case, tmp_path):
    mc = merge_case
    with bw.DevMerger(ctx, 1) as m:                                                        # nothing to merge: an index without records
        bai = str(tmp_path / "empty.bai")
        fb = os.open(bai, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        m.add(0, b"", np.zeros(0, dtype=np.uint64), np.zeros(1, dtype=np.int64))
        st, bs = m.finish_bai(-1, fb, 100, 4)
        os.close(fb)
        assert open(bai, "rb").read() == bai_ref.build([], [100], 4) and st.n_blocks == 0
    runs = sref.make_runs(mc["recs"], 3, random.Random(2))
    with bw.DevMerger(ctx, 3) as m:                                                        # both outputs dropped; then refused records leave the merger usable
        for k in (2, 0, 1):
            m.add(k, *sref.run_arrays(runs[k], mc["key_of"]))
        st, bs = m.finish_bai(-1, -1, len(mc["hdr"]), mc["n_ref"])
        assert bs.bai_bytes == len(mc["want"]) and st.bgzf_bytes == len(mc["members"])
        with pytest.raises(bw.BwahipError, match="EINVAL"):                                 # refID 3 >= n_ref 3
            m.finish_bai(-1, -1, len(mc["hdr"]), 3)
        fb = os.open(str(tmp_path / "again.bai"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        m.finish_bai(-1, fb, len(mc["hdr"]), mc["n_ref"])
        os.close(fb)
        assert open(str(tmp_path / "again.bai"), "rb").read() == mc["want"]


# ---------------------------------------------------------------------------------------------------------------- 3. the stream driver
K = 600 * 150
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"


@pytest.fixture(scope="module")
def stream_case(small_index, tmp_path_factory):
    d = tmp_path_factory.mktemp("bai_stream")
    fq1, fq2 = str(d / "s_1.fq"), str(d / "s_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 1800, 150, 10000, 2000, 500, 173)
    return dict(fq1=fq1, fq2=fq2, files={})


def _run(fn, ctxs, case, pe, tmp_path, with_bai, **kw):
    opt = bw.default_opt()
    opt.n_threads = 4
    out, bai = str(tmp_path / "o.bam"), str(tmp_path / "o.bai")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    fb = os.open(bai, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) if with_bai else -1
    try:
        extra = dict(bai_fd=fb) if with_bai else {}
        st, so = fn(ctxs, case["fq1"], case["fq2"] if pe else None, fd, hdr_line=HDR, opt=opt, chunk_bases=K, reader_threads=2, **extra, **kw)
    finally:
        os.close(fd)
        if with_bai:
            os.close(fb)
    return open(out, "rb").read(), (open(bai, "rb").read() if with_bai else None), st, so


def _judge(bam, bai, what):
    assert bai == bai_ref.from_file(bam), what + ": not the canonical index of the file"
    n_ref, recs, offs, _ = bai_ref.split_file(bam)
    assert bai_ref.check_semantics(bai, recs, offs, n_ref) > len(recs) // 2, what


@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("n_ctx", [1, 3])
def test_stream_driver_writes_the_file_and_its_index(small_index, stream_case, tmp_path, n_ctx, pe):
    n_batches = 3 if pe else 2
    spill = tmp_path / "spill"
    spill.mkdir()
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            what = f"n_ctx {n_ctx}, {'pe' if pe else 'se'}"
            # merged on the host
            plain, _, _, _ = _run(bw.stream_run_bam_sorted, ctxs, stream_case, pe, tmp_path, False, level=1, tmp_dir=str(spill), mem_budget=1 << 30)
            bam, bai, st, so = _run(bw.stream_run_bam_sorted_bai, ctxs, stream_case, pe, tmp_path, True, level=1, tmp_dir=str(spill), mem_budget=1 << 30)
            assert bam == plain and st.n_batches == n_batches, what + ": host-merged file differs from the entry point without index"
            _judge(bam, bai, what + ", host")
            # merged on the device
            plain_dev, _, _, sd0 = _run(bw.stream_run_bam_sorted_dev, ctxs, stream_case, pe, tmp_path, False, hbm_budget=8 << 30)
            bam, bai, st, sd = _run(bw.stream_run_bam_sorted_dev_bai, ctxs, stream_case, pe, tmp_path, True, hbm_budget=8 << 30)
            assert bam == plain_dev and sd.fell_back == 0 and sd.n_runs == n_batches and sd.dev.n_records == sd0.dev.n_records, what + ": device-merged file differs"
            _judge(bam, bai, what + ", device")
            # a budget for one and a half batches: the fall-back begins at run 1, and the index comes from the host path
            frac = 1.5 / n_batches
            raw, n_rec = int(frac * sd.dev.raw_bytes), int(frac * sd.dev.n_records)
            bns = bw.lib().bwahip_bns(c0._h).contents
            windows = sum((bns.anns[i].len + 16383) >> 14 for i in range(bns.n_seqs))
            budget = bw.bam_devmerge_hbm_need(raw, n_rec, 2, 1024) + bw.bam_devmerge_bai_hbm_need(n_rec, (raw + 65279) // 65280, bns.n_seqs, windows)
            bam, bai, st, sd = _run(bw.stream_run_bam_sorted_dev_bai, ctxs, stream_case, pe, tmp_path, True, hbm_budget=budget, tmp_dir=str(spill), level=1)
            assert sd.fell_back == 1 and sd.fell_back_at_run == 1 and bam == plain, what + ": the fall-back's file is not the host path's"
            _judge(bam, bai, what + ", fall-back")
            assert os.listdir(spill) == []
        finally:
            for c in ctxs[1:]:
                c.close()


def test_stream_driver_dropped_outputs(small_index, stream_case, tmp_path):
    with bw.Context(small_index["prefix"]) as c0:
        opt = bw.default_opt()
        opt.n_threads = 4
        a, b = stream_case["fq1"], stream_case["fq2"]
        for fn, kw in ((bw.stream_run_bam_sorted_bai, dict(level=1)), (bw.stream_run_bam_sorted_dev_bai, {})):
            st, so = fn([c0], a, b, -1, -1, HDR, opt=opt, chunk_bases=K, **kw)                # both built and dropped
            assert st.n_batches == 3 and so.n_records >= 1800
            bai = str(tmp_path / "only.bai")                                                 # the file dropped, the index kept
            fb = os.open(bai, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            fn([c0], a, b, -1, fb, HDR, opt=opt, chunk_bases=K, **kw)
            os.close(fb)
            bam, want, _, _ = _run(fn, [c0], stream_case, True, tmp_path, True, **kw)
            assert open(bai, "rb").read() == want == bai_ref.from_file(bam)
