"""The merge of sorted runs on the device (csrc/k_bammerge.hip) and the stream driver that keeps its runs in HBM.  The judge of content is
Python: tests/bam_sort_ref.py's stable sort of the records and gzip / tests/bgzf_ref.py on what came out.  The judge of the member bytes
is Context.kat_bgzf -- the deflate stage alone -- over the Python-sorted concatenation: blocks are cut every 65 280 bytes whatever the
pieces, so the merger's members must be those bytes for every piece size, every cut into runs and every order of adding them.  Byte for
byte, no tolerance."""
import gzip
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bam_ref
import bam_sort_ref as sref
import bgzf_ref
import common
from common import bw

pytestmark = pytest.mark.gpu

BLOCK = 65280
# the synthetic index the keys of the synthetic records are packed for: positions take 32 bits, so refID sits above bit 32
N_SEQS, LONGEST = 5, 2 ** 31 - 1


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
    assert len(head) == 20
    # bytes that deflate (a small alphabet) and bytes that do not, so that dynamic and stored members both occur
    body = bytes(rng.choices(b"ACGT", k=length - 20)) if length < 60000 else rng.randbytes(length - 20)
    return head + body


def _merge(ctx, runs, order, piece_blocks, tmp_path, key_of=_key):
    """runs: list of record lists (run k = runs[k]); order: the run numbers in the order they are added."""
    out = str(tmp_path / "members.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, piece_blocks) as m:
            for k in order:
                m.add(k, *sref.run_arrays(runs[k], key_of))
            st = m.finish(fd)
    finally:
        os.close(fd)
    return open(out, "rb").read(), st


# ---------------------------------------------------------------------------------------------------------------- 1. the merger alone
SPECIAL = (20, 31, 32, 33, 36, 300, 65279, 65280, 65281, 70000, 140000)


@pytest.fixture(scope="module")
def synthetic(ctx):
    """Records in input order, their Python sort, and the deflate stage's members of the sorted bytes (the expectation, made once)."""
    rng = random.Random(2024)
    recs = []
    # in sorted order: 65 280 bytes first (it ends on the first cut, the next record begins there), then 452 small bytes, then 140 000
    # (from 65 732 to 205 732: it covers the piece [130 560, 195 840) and spills into both neighbours), then the rest
    recs.append(_rec(65280, 0, 0, False, rng))
    for k, n in enumerate((20, 31, 32, 33, 36, 300)):
        recs.append(_rec(n, 0, 10 + k, k % 2 == 1, rng))
    recs.append(_rec(140000, 0, 100, False, rng))
    for k, n in enumerate((65279, 65281, 70000)):
        recs.append(_rec(n, 1, 5 + k, False, rng))
    # many small ones around them, with tie groups (equal refID, pos, strand) whose members differ in content
    for k in range(900):
        recs.append(_rec(rng.choice((20, 21, 35, 47, 48, 49, 64, 150, 333, 400)), rng.choice((1, 2, 3, -1)), rng.randrange(0, 40) if k % 3 else 7, rng.random() < 0.5, rng))
    assert sorted(set(SPECIAL)) == sorted(set(SPECIAL) & {len(r) for r in recs})
    rng.shuffle(recs)
    want = sref.stable_sort(recs)
    off = np.concatenate(([0], np.cumsum([len(r) for r in want])))
    starts, ends = set(off[:-1].tolist()), set(off[1:].tolist())
    assert BLOCK in starts and BLOCK in ends                                           # begins / ends exactly on a cut (piece_blocks = 1)
    assert any(a < c * BLOCK < b for a, b in zip(off[:-1], off[1:]) for c in (3, 4, 5))  # straddles a cut
    assert any(a < 2 * BLOCK and b > 3 * BLOCK for a, b in zip(off[:-1], off[1:]))       # covers a whole piece and spills into both neighbours
    want_bytes = b"".join(want)
    members, n_blocks, _ = ctx.kat_bgzf(want_bytes)
    assert bgzf_ref.inflate(members) == want_bytes and n_blocks == (len(want_bytes) + BLOCK - 1) // BLOCK
    return dict(recs=recs, want=want_bytes, members=members, n_blocks=n_blocks)


@pytest.mark.parametrize("n_runs", [1, 2, 7])
def test_merger_equals_python_sort_for_every_piece_size_and_add_order(ctx, synthetic, tmp_path, n_runs):
    rng = random.Random(n_runs)
    runs = sref.make_runs(synthetic["recs"], n_runs, rng, empty=3 if n_runs == 7 else None)
    assert sum(len(r) for r in runs) == len(synthetic["recs"]) and (n_runs != 7 or any(not r for r in runs))
    shuffled = list(range(n_runs))
    rng.shuffle(shuffled)
    for order in (list(range(n_runs)), list(range(n_runs))[::-1], shuffled):
        for pb in (1, 2, 3, 0):
            got, st = _merge(ctx, runs, order, pb, tmp_path)
            what = f"{n_runs} runs added as {order}, piece_blocks {pb}"
            assert bgzf_ref.inflate(got) == synthetic["want"], what
            assert got == synthetic["members"], what + ": not the deflate stage's members of the sorted records"
            assert (st.n_records, st.n_runs, st.raw_bytes, st.n_blocks, st.bgzf_bytes) == (len(synthetic["recs"]), n_runs, len(synthetic["want"]), synthetic["n_blocks"], len(got)), what
            assert 0 < st.n_stored < st.n_blocks and st.hbm_bytes > st.raw_bytes + 16 * st.n_records and st.finish_s > 0, what


def test_piece_blocks_knob(ctx, synthetic, tmp_path):
    runs = sref.make_runs(synthetic["recs"], 3, random.Random(3))
    try:
        ctx.tune(sorted_piece_blocks=2)
        got, _ = _merge(ctx, runs, [2, 0, 1], 0, tmp_path)
        assert got == synthetic["members"]
        for bad in (0, -1, 4097):
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                ctx.tune(sorted_piece_blocks=bad)
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            bw.DevMerger(ctx, 4097)
    finally:
        ctx.tune(sorted_piece_blocks=1024)


# ---------------------------------------------------------------------------------------------------------------- 2. edges
def test_nothing_to_merge_writes_nothing(ctx, tmp_path):
    got, st = _merge(ctx, [], [], 1, tmp_path)
    assert got == b"" and (st.n_records, st.n_runs, st.raw_bytes, st.n_blocks, st.bgzf_bytes) == (0, 0, 0, 0, 0)
    got, st = _merge(ctx, [[], [], []], [1, 0, 2], 0, tmp_path)
    assert got == b"" and (st.n_records, st.n_runs, st.raw_bytes, st.n_blocks) == (0, 3, 0, 0)


def test_one_record_of_one_byte(ctx, tmp_path):
    out = str(tmp_path / "one.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 1) as m:
            m.add(4, b"\x5a", np.array([9], dtype=np.uint64), np.array([0, 1], dtype=np.int64))
            st = m.finish(fd)
    finally:
        os.close(fd)
    got = open(out, "rb").read()
    assert bgzf_ref.inflate(got) == b"\x5a" and got == ctx.kat_bgzf(b"\x5a")[0] and (st.n_records, st.n_blocks, st.raw_bytes) == (1, 1, 1)


@pytest.mark.parametrize("pb,total", [(1, BLOCK), (2, 2 * BLOCK), (3, 3 * BLOCK), (2, BLOCK)])
def test_total_is_a_whole_number_of_pieces(ctx, tmp_path, pb, total):
    rng = random.Random(total + pb)
    lens = [1000] * (total // 1000) + [total % 1000]
    recs = [_rec(n, rng.randrange(0, 3), rng.randrange(0, 1000), False, rng) for n in lens]
    assert sum(map(len, recs)) == total
    want = b"".join(sref.stable_sort(recs))
    got, st = _merge(ctx, sref.make_runs(recs, 4, rng), [3, 1, 0, 2], pb, tmp_path)
    assert bgzf_ref.inflate(got) == want and got == ctx.kat_bgzf(want)[0] and st.n_blocks == total // BLOCK


def test_equal_keys_come_out_by_run_number_then_position(ctx, tmp_path):
    rng = random.Random(5)
    runs = [[_rec(rng.randrange(20, 200), 2, 77, False, rng) for _ in range(rng.randrange(1, 40))] for _ in range(5)]
    assert len({bytes(r) for run in runs for r in run}) == sum(map(len, runs))          # equal keys, different bytes
    got, _ = _merge(ctx, runs, [4, 3, 2, 1, 0], 1, tmp_path)
    assert bgzf_ref.inflate(got) == b"".join(r for run in runs for r in run)


def test_keys_that_differ_only_above_bit_32(ctx, tmp_path):
    rng = random.Random(6)
    recs = [_rec(40 + k % 7, ref, 123, True, rng) for k, ref in enumerate(rng.choices((0, 1, 2, 3, 4, -1), k=600))]
    keys = {_key(r) for r in recs}
    assert len(keys) == 6 and len({k & 0x1ffffffff for k in keys}) == 1                 # bits 0 .. 32 are the same in all keys
    want = b"".join(sref.stable_sort(recs))
    got, _ = _merge(ctx, sref.make_runs(recs, 3, rng), [1, 2, 0], 1, tmp_path)
    assert bgzf_ref.inflate(got) == want and got == ctx.kat_bgzf(want)[0]


def test_refused_adds_leave_the_merger_usable(ctx, synthetic, tmp_path):
    runs = sref.make_runs(synthetic["recs"], 3, random.Random(8))
    out = str(tmp_path / "m.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 2) as m:
            m.add(0, *sref.run_arrays(runs[0], _key))
            m.add(2, *sref.run_arrays(runs[2], _key))
            with pytest.raises(bw.BwahipError, match="EINVAL"):                          # a run number given twice
                m.add(2, *sref.run_arrays(runs[1], _key))
            rec, keys, off = sref.run_arrays(runs[1], _key)
            bad = off.copy()
            bad[-1] -= 1
            with pytest.raises(bw.BwahipError, match="EINVAL"):                          # offsets that do not end at the run's length
                m.add(1, rec, keys, bad)
            bad = off.copy()
            bad[1], bad[2] = off[2], off[1]
            with pytest.raises(bw.BwahipError, match="EINVAL"):                          # offsets that decrease
                m.add(1, rec, keys, bad)
            m.add(1, rec, keys, off)
            st = m.finish(fd)
            assert st.n_runs == 3 and st.n_records == len(synthetic["recs"])
    finally:
        os.close(fd)
    assert open(out, "rb").read() == synthetic["members"]


# ---------------------------------------------------------------------------------------------------------------- 3. real runs
K = 600 * 150
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"


def _oracle_sam(prefix, fqs, extra=()):
    out = subprocess.run([common.ORACLE, "mem", "-t", "8", *extra, prefix, *fqs], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    return b"".join(l + b"\n" for l in out.split(b"\n") if l and not l.startswith(b"@"))


@pytest.fixture(scope="module")
def stream_case(small_index, tmp_path_factory):
    """The 4300 reads in pairs of test_gpu_bam_sorted.py's stream case, made again with its seed, and the oracle's records with -K sorted
    by Python: 8 batches paired, 4 single-end (the first file alone)."""
    d = tmp_path_factory.mktemp("devmerge_stream")
    fq1, fq2 = str(d / "s_1.fq"), str(d / "s_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 4300, 150, 10000, 2000, 500, 171)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = {}
    for pe in (True, False):
        recs = bam_ref.split_records(bam_ref.sam_to_bam_records(_oracle_sam(small_index["prefix"], [fq1, fq2] if pe else [fq1], ["-K", str(K)]), contigs))
        want[pe] = (len(recs), b"".join(sref.stable_sort(recs)))
    return dict(fq1=fq1, fq2=fq2, want=want, members={}, host_file={}, files={}, at={})


def test_real_batches_through_the_merger(ctx, stream_case, tmp_path):
    n_rec, want = stream_case["want"][True]
    opt = bw.default_opt()
    opt.n_threads = 4
    opt.flag |= 0x2
    out = str(tmp_path / "real.bin")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.DevMerger(ctx, 1) as m, bw.FastqReader(stream_case["fq1"], stream_case["fq2"]) as rd:
            batches, done = [], 0
            while True:
                arr, n = rd.next(K)
                if n == 0:
                    break
                batches.append(ctx.process_seqs_bam_sorted_array(arr, n, opt, done))
                done += n
            assert len(batches) == 8 and done == 4300
            for k in (5, 0, 7, 2, 1, 6, 3, 4):
                m.add(k, *batches[k])
            st = m.finish(fd)
    finally:
        os.close(fd)
    got = open(out, "rb").read()
    assert bgzf_ref.inflate(got) == want
    assert got == stream_case["members"].setdefault(True, ctx.kat_bgzf(want)[0])
    assert (st.n_records, st.n_runs, st.raw_bytes, st.n_blocks) == (n_rec, 8, len(want), (len(want) + BLOCK - 1) // BLOCK)


# ---------------------------------------------------------------------------------------------------------------- 4. the stream driver
def _run_dev(ctxs, case, pe, path, **kw):
    opt = bw.default_opt()
    opt.n_threads = 4
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        st, sd = bw.stream_run_bam_sorted_dev(ctxs, case["fq1"], case["fq2"] if pe else None, fd, HDR, opt, chunk_bases=K, reader_threads=2, **kw)
    finally:
        os.close(fd)
    return open(path, "rb").read(), st, sd


@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("n_ctx", [1, 2, 3])
def test_stream_driver_files_to_sorted_bam_on_the_device(small_index, stream_case, tmp_path, n_ctx, pe):
    n_rec, want_recs = stream_case["want"][pe]
    n_batches, n_reads = (8, 4300) if pe else (4, 2150)
    spill = tmp_path / "spill"
    spill.mkdir()
    out = str(tmp_path / "out.bam")
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0] + [c0.clone_on(0) for _ in range(n_ctx - 1)]
        try:
            header = bw.bam_header_sorted(c0, HDR)
            if pe not in stream_case["members"]:
                stream_case["members"][pe] = c0.kat_bgzf(want_recs)[0]
            hdr_member = str(tmp_path / "hdr.bin")
            fd = os.open(hdr_member, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            bw.bgzf_write(fd, header, 1, 1)
            os.close(fd)
            want_file = open(hdr_member, "rb").read() + stream_case["members"][pe] + bgzf_ref.EOF_BLOCK
            if pe not in stream_case["host_file"]:                   # the host path's file at level 1: what every fall-back must write
                opt = bw.default_opt()
                opt.n_threads = 4
                fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                try:
                    bw.stream_run_bam_sorted(ctxs, stream_case["fq1"], stream_case["fq2"] if pe else None, fd, HDR, 1, opt, chunk_bases=K, reader_threads=2, tmp_dir=str(spill), mem_budget=1 << 30)
                finally:
                    os.close(fd)
                stream_case["host_file"][pe] = open(out, "rb").read()
                assert gzip.decompress(stream_case["host_file"][pe]) == header + want_recs
            # a budget that holds everything
            for pb in (1, 0):
                what = f"n_ctx {n_ctx}, piece_blocks {pb}, {'pe' if pe else 'se'}"
                got, st, sd = _run_dev(ctxs, stream_case, pe, out, hbm_budget=8 << 30, piece_blocks=pb, tmp_dir=str(tmp_path / "nowhere"))   # tmp_dir is not looked at
                assert gzip.decompress(got) == header + want_recs, what
                assert got == want_file, what + ": not header member + the deflate stage's members of the sorted records + EOF"
                assert sd.fell_back == 0 and sd.spilled_bytes == 0, what
                assert (sd.n_records, sd.n_runs, sd.dev.n_records, sd.dev.n_runs, sd.dev.raw_bytes) == (n_rec, n_batches, n_rec, n_batches, len(want_recs)), what
                assert sd.dev.n_blocks == (len(want_recs) + BLOCK - 1) // BLOCK and sd.dev.bgzf_bytes == len(stream_case["members"][pe]), what
                assert st.n_batches == n_batches and st.n_reads == n_reads and st.sam_bytes == len(want_recs) and sd.sort_ms > 0 and sd.merge_s > 0, what
            # a budget that holds nothing
            got, st, sd = _run_dev(ctxs, stream_case, pe, out, hbm_budget=1, tmp_dir=str(spill), mem_budget=0, level=1)
            assert sd.fell_back == 1 and sd.fell_back_at_run == 0 and got == stream_case["host_file"][pe]
            assert (sd.n_records, sd.n_runs, sd.dev.n_records, sd.dev.n_blocks) == (n_rec, n_batches, 0, 0) and sd.spilled_bytes > 0 and st.n_reads == n_reads
            assert os.listdir(spill) == []
            # a budget for two and a half of the full batches (600 of the 4300 reads, or of the 2150 single-end ones, each)
            frac = 2.5 * 600 / (4300 if pe else 2150)
            budget = bw.bam_devmerge_hbm_need(int(frac * len(want_recs)), int(frac * n_rec), 3, 1024)
            got, st, sd = _run_dev(ctxs, stream_case, pe, out, hbm_budget=budget, tmp_dir=str(spill), level=1)
            assert sd.fell_back == 1 and 0 < sd.fell_back_at_run < n_batches and got == stream_case["host_file"][pe]
            assert stream_case["at"].setdefault(pe, sd.fell_back_at_run) == sd.fell_back_at_run, "the run the fall-back begins at depends on the number of contexts"
            assert (sd.n_records, sd.n_runs) == (n_rec, n_batches) and os.listdir(spill) == []
        finally:
            for c in ctxs[1:]:
                c.close()


def test_stream_driver_dropped_output_and_refused_header(small_index, stream_case, tmp_path):
    n_rec, want_recs = stream_case["want"][True]
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = [c0, c0.clone_on(0)]
        try:
            opt = bw.default_opt()
            opt.n_threads = 4
            a, b = stream_case["fq1"], stream_case["fq2"]
            st, sd = bw.stream_run_bam_sorted_dev(ctxs, a, b, -1, None, opt, chunk_bases=K, max_reads=1000)       # produced and dropped; the default budget
            assert st.n_reads == 1200 and st.n_batches == 2 and sd.n_runs == 2 and sd.n_records >= 1200 and sd.fell_back == 0 and sd.dev.bgzf_bytes > 0
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                bw.stream_run_bam_sorted_dev(ctxs, a, b, -1, "@HD\tVN:1.6\tSO:unsorted", opt, chunk_bases=K)
            with pytest.raises(bw.BwahipError, match="EIO"):                                                       # a tmp_dir that cannot be used, once it is used
                bw.stream_run_bam_sorted_dev(ctxs, a, b, -1, None, opt, chunk_bases=K, hbm_budget=1, tmp_dir=str(tmp_path / "nowhere"))
            got, st, sd = _run_dev(ctxs, stream_case, True, str(tmp_path / "after.bam"))                            # the contexts still work
            assert gzip.decompress(got) == bw.bam_header_sorted(c0, HDR) + want_recs and sd.fell_back == 0 and sd.n_records == n_rec
        finally:
            ctxs[1].close()
