"""The form of a batch's output is an argument of every call, and the stream driver's outputs are sinks behind one driver: nothing of
one call's form, and nothing of one run's sink, may be left in a context for the next.  Every form in turn on one context, and every
sink in turn on the same three contexts, each against what that form or sink gives on its own."""
import gzip
import os

import numpy as np
import pytest

import bam_ref
import bam_sort_ref as sref
import bgzf_ref
from common import bw
from test_gpu_stream_pipeline import K_PE, _contexts, _cuts, _oracle, _records, _write

pytestmark = pytest.mark.gpu
HDR = "@RG\tID:g1\tSM:s\n@PG\tID:bwahip"


@pytest.fixture(scope="module")
def inputs(small_index, tmp_path_factory):
    """test_gpu_stream_pipeline.py's paired 2 x 150 reads (same recipe, same seed): the first 100 pairs as one batch, the first 300 as
    three batches of -K 200 * 150 with the oracle's SAM for them."""
    d = tmp_path_factory.mktemp("out_forms")
    fq1, fq2 = str(d / "all_1.fq"), str(d / "all_2.fq")
    bw.make_reads(small_index["fa"], fq1, fq2, 1202, 150, 10000, 2000, 500, 611, 20000)
    r1, r2 = _records(fq1), _records(fq2)
    out = {}
    for pairs in (100, 300):
        a, b = str(d / f"p{pairs}_1.fq"), str(d / f"p{pairs}_2.fq")
        _write(a, r1[:pairs]); _write(b, r2[:pairs])
        out[pairs] = (a, b)
    assert _cuts([len(x[1]) for p in zip(r1[:300], r2[:300]) for x in p], K_PE, pe=True) == [200, 200, 200]
    out["sam"] = _oracle(small_index["prefix"], list(out[300]), K_PE)
    return out


def _opt():
    opt = bw.default_opt()
    opt.n_threads = 4
    opt.flag |= 0x2
    return opt


def _batch_reads(inputs):
    (n1, s1, q1), (n2, s2, q2) = bw.read_fastq(inputs[100][0]), bw.read_fastq(inputs[100][1])
    mix = lambda x, y: [v for p in zip(x, y) for v in p]
    return mix(n1, n2), mix(s1, s2), mix(q1, q2)


def _text(c, reads, opt):
    arr, keep = bw.seq_array(*reads)
    return c.process_seqs_text_array(arr, len(reads[0]), opt)


CALLS = {
    "bam_sorted": lambda c, reads, opt: c.process_seqs_bam_sorted(*reads, opt),
    "bgzf": lambda c, reads, opt: c.process_seqs_bgzf(*reads, opt),
    "text": _text,
    "bam": lambda c, reads, opt: c.process_seqs_bam(*reads, opt),
    "strings": lambda c, reads, opt: c.process_seqs(*reads, opt),
}


def _assert_same(form, got, want, what):
    if form == "bam_sorted":                                        # records, keys, offsets; n_rec is the length of the keys
        assert got[0] == want[0], what
        assert len(got[1]) == len(want[1]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
    elif form == "bgzf":                                            # members, bytes of the records, number of members
        assert got == want and gzip.decompress(got[0]) == gzip.decompress(want[0]), what
    else:
        assert got == want, what


def test_every_form_in_turn_on_one_context(small_index, inputs):
    reads = _batch_reads(inputs)
    assert len(reads[0]) == 200
    opt = _opt()
    want = {}
    for form, call in CALLS.items():                                # what a fresh context returns for that one call
        with bw.Context(small_index["prefix"]) as fresh:
            want[form] = call(fresh, reads, opt)
    assert gzip.decompress(want["bgzf"][0]) == want["bam"] and b"".join(want["strings"]) == want["text"]
    assert len(want["bam_sorted"][1]) == len(bam_ref.split_records(want["bam"])) and len(want["bam_sorted"][0]) == len(want["bam"])
    long_names = list(reads[0])
    long_names[4] = long_names[5] = b"n" * 255
    with bw.Context(small_index["prefix"]) as c:
        for k, form in enumerate(("bam_sorted", "bgzf", "text", None, "bam", "strings", "bgzf", "bam_sorted")):
            if form is None:                                        # a refused call in the middle: the one after it is still correct
                with pytest.raises(bw.BwahipError, match="EINVAL"):
                    c.process_seqs_bam(long_names, reads[1], reads[2], opt)
                continue
            _assert_same(form, CALLS[form](c, reads, opt), want[form], f"call {k} ({form})")


def _to_file(path, fn):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        r = fn(fd)
    finally:
        os.close(fd)
    return r, open(path, "rb").read()


def _records_per_batch(sam, contigs, pairs_per_batch):
    """the BAM records of the oracle's SAM, batch by batch: a pair's lines share a name, and neighbouring pairs do not"""
    batches, names = [[]], 0
    last = None
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        name = line.split(b"\t", 1)[0]
        if name != last:
            last = name
            names += 1
            if names > pairs_per_batch:
                batches.append([])
                names = 1
        batches[-1].append(line + b"\n")
    return [bam_ref.sam_to_bam_records(b"".join(b), contigs) for b in batches]


def test_every_sink_in_turn_on_the_same_contexts(small_index, inputs, tmp_path):
    a, b = inputs[300]
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    per_batch = _records_per_batch(inputs["sam"], contigs, 100)
    recs = b"".join(per_batch)
    body = b"".join(l + b"\n" for l in inputs["sam"].split(b"\n") if l and not l.startswith(b"@"))
    assert len(per_batch) == 3 and recs == bam_ref.sam_to_bam_records(body, contigs)
    split = bam_ref.split_records(recs)
    n_rec, want_sorted = len(split), b"".join(sref.stable_sort(split))
    spill = tmp_path / "spill"
    spill.mkdir()
    opt = bw.default_opt()
    opt.n_threads = 4
    kw = dict(chunk_bases=K_PE, reader_threads=2)
    with bw.Context(small_index["prefix"]) as c0:
        ctxs = _contexts(c0, 3)
        try:
            header, header_sorted = bw.bam_header(c0, HDR), bw.bam_header_sorted(c0, HDR)
            _, hdr_member = _to_file(str(tmp_path / "hdr.bin"), lambda fd: bw.bgzf_write(fd, header_sorted, 1, 1))
            out = lambda k: str(tmp_path / f"pass{k}.out")
            # 1. device-merged, with a budget so small that run 0 falls back to the host merger
            (st, sd), got1 = _to_file(out(1), lambda fd: bw.stream_run_bam_sorted_dev(ctxs, a, b, fd, HDR, opt, hbm_budget=1, tmp_dir=str(spill), level=1, **kw))
            assert gzip.decompress(got1) == header_sorted + want_sorted
            assert (st.n_reads, st.n_batches, st.sam_bytes) == (600, 3, len(recs))
            assert (sd.n_records, sd.n_runs, sd.fell_back, sd.fell_back_at_run) == (n_rec, 3, 1, 0) and os.listdir(spill) == []
            # 2. BAM with the members made on the GPU
            (st, bs), got2 = _to_file(out(2), lambda fd: bw.stream_run_bam_dev(ctxs, a, b, fd, HDR, opt, **kw))
            assert bgzf_ref.inflate(got2) == header + recs and got2.endswith(bgzf_ref.EOF_BLOCK)
            assert (st.n_reads, st.n_batches, st.sam_bytes) == (600, 3, len(recs))
            assert (bs.raw_bytes, bs.n_blocks) == (len(recs), sum(len(bgzf_ref.blocks_of(r)) for r in per_batch))
            # 3. SAM text
            st, got3 = _to_file(out(3), lambda fd: bw.stream_run(ctxs, a, b, fd, opt, **kw))
            assert got3 == inputs["sam"]
            assert (st.n_reads, st.n_batches, st.sam_bytes) == (600, 3, len(inputs["sam"]))
            # 4. host-merged
            (st, so), got4 = _to_file(out(4), lambda fd: bw.stream_run_bam_sorted(ctxs, a, b, fd, HDR, 1, opt, tmp_dir=str(spill), **kw))
            assert gzip.decompress(got4) == header_sorted + want_sorted and got4.endswith(bgzf_ref.EOF_BLOCK)
            assert (st.n_reads, st.n_batches, st.sam_bytes) == (600, 3, len(recs))
            assert (so.n_records, so.n_runs) == (n_rec, 3) and os.listdir(spill) == []
            assert gzip.decompress(got1) == gzip.decompress(got4) and got1 == got4, "the fall-back's file is not the host-merged one"
            # 5. BAM through the host's BGZF writer, stored
            st, got5 = _to_file(out(5), lambda fd: bw.stream_run_bam(ctxs, a, b, fd, HDR, 0, opt, **kw))
            assert gzip.decompress(got5) == header + recs and got5.endswith(bgzf_ref.EOF_BLOCK) and len(got5) > len(recs)
            assert (st.n_reads, st.n_batches, st.sam_bytes) == (600, 3, len(recs))
            # 6. device-merged with the default budget: nothing falls back, tmp_dir is not looked at
            (st, sd), got6 = _to_file(out(6), lambda fd: bw.stream_run_bam_sorted_dev(ctxs, a, b, fd, HDR, opt, tmp_dir=str(tmp_path / "nowhere"), **kw))
            assert gzip.decompress(got6) == gzip.decompress(got4)
            assert got6 == hdr_member + c0.kat_bgzf(want_sorted)[0] + bgzf_ref.EOF_BLOCK
            assert (st.n_reads, st.n_batches, st.sam_bytes) == (600, 3, len(recs))
            assert (sd.n_records, sd.n_runs, sd.fell_back, sd.fell_back_at_run) == (n_rec, 3, 0, 0) and sd.n_records == so.n_records
            assert (sd.dev.n_records, sd.dev.n_runs, sd.dev.raw_bytes) == (n_rec, 3, len(recs))
        finally:
            for c in ctxs[1:]:
                c.close()
