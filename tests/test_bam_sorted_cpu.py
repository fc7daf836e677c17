"""Coordinate-sorted BAM, the parts that need no GPU: the merger of sorted runs, the header that announces the order, the sort key, and
the merger under the sanitizers.  The expectation is tests/bam_ref.py applied to the reference-made golden SAM, reordered by Python's
stable sorted() on a key read from the record's own bytes (tests/bam_sort_ref.py) -- never the code under test."""
import ctypes as C
import gzip
import os
import random
import struct
import subprocess
import threading

import numpy as np
import pytest

import bam_ref
import bam_sort_ref as sref
import common
from common import bw

GOLDEN_CONTIGS = ["ctg1", "ctg2", "ctg3"]
GOLDEN_LENS = [40000, 16000, 4000]
CSRC = os.path.join(common.ROOT, "bwa-mem-gpu_amd", "csrc")


def _bns(names, lens):
    anns = (bw.Ann * len(names))()
    off = 0
    for i, (n, l) in enumerate(zip(names, lens)):
        anns[i].offset, anns[i].len, anns[i].name, anns[i].anno = off, l, n.encode(), b""
        off += l
    bns = bw.Bns()
    bns.l_pac, bns.n_seqs, bns.anns = off, len(names), anns
    return bns, anns


@pytest.fixture(scope="module")
def golden_records(built):
    """Records of the golden paired-end and -a single-end SAM, in input order: three contigs, unmapped reads, secondary records."""
    sam = gzip.open(os.path.join(common.GOLDEN, "pe.sam.gz")).read() + gzip.open(os.path.join(common.GOLDEN, "se_all.sam.gz")).read()
    recs = bam_ref.split_records(bam_ref.sam_to_bam_records(sam, GOLDEN_CONTIGS))
    f = [sref.fields(r) for r in recs]
    assert len({x[0] for x in f if x[0] >= 0}) >= 2 and sum(1 for x in f if x[0] < 0) >= 30 and {x[2] for x in f} == {0, 1}
    assert len(recs) > 1000
    return recs


def _key_of(rec):
    return sref.packed_key(rec, len(GOLDEN_CONTIGS), max(GOLDEN_LENS))


def _merge(runs, order, tmp, budget, level, n_threads=3):
    """The runs (run number = list position) added from three threads in the given order; returns (inflated output, stats)."""
    out = os.path.join(tmp, "merged.bgzf")
    with bw.BamMerger(tmp, budget) as m:
        errs = []

        def work(part):
            try:
                for k in part:
                    m.add(k, *sref.run_arrays(runs[k], _key_of))
            except Exception as e:                                  # noqa: BLE001 -- reported below
                errs.append(e)
        th = [threading.Thread(target=work, args=(order[t::3],)) for t in range(3)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            m.finish(fd, level, n_threads)
        finally:
            os.close(fd)
        st = m.stats()
        spilled = [f for f in os.listdir(tmp) if f.endswith(".run")]
        assert (len(spilled) > 0) == (st["spilled_bytes"] > 0)
    assert [f for f in os.listdir(tmp) if f != "merged.bgzf"] == [], "close left files behind"
    raw = open(out, "rb").read()
    os.unlink(out)
    return raw, st


@pytest.mark.parametrize("n_runs", [1, 2, 5, 17])
def test_merger_equals_the_global_stable_sort(golden_records, tmp_path, n_runs):
    rng = random.Random(100 + n_runs)
    runs = sref.make_runs(golden_records, n_runs, rng, empty=1 if n_runs > 1 else None)
    if n_runs > 1:
        assert any(len(r) == 0 for r in runs) and len({len(r) for r in runs}) > 1
    want = b"".join(sref.stable_sort(golden_records))
    total = sum(len(b"".join(r)) + 16 * len(r) + 8 for r in runs)
    order = list(range(n_runs))
    rng.shuffle(order)
    files = set()
    for budget in (0, total // 2, 1 << 30):
        for level in (0, 1):
            raw, st = _merge(runs, order, str(tmp_path), budget, level)
            assert gzip.decompress(raw) == want if raw else want == b"", f"budget {budget}, level {level}"
            assert st["n_records"] == len(golden_records) and st["n_runs"] == n_runs
            if budget == 0:
                assert st["spilled_bytes"] == sum(len(b"".join(r)) + 16 * len(r) + 8 for r in runs if r)
            elif budget == 1 << 30:
                assert st["spilled_bytes"] == 0
            elif n_runs > 2:
                assert 0 < st["spilled_bytes"] < total
            files.add((level, raw))
    assert len(files) == 2, "the file depends on the memory budget"


def test_merger_ties_follow_run_number_then_position(built, tmp_path):
    """Hand-made records that differ only in their names, all on one (refID, pos, strand), handed over as five runs added backwards."""
    recs = [bam_ref.sam_to_bam_records(f"r{k}\t0\tctg2\t77\t60\t4M\t*\t0\t0\tACGT\tIIII\n", GOLDEN_CONTIGS) for k in range(50)]
    runs = [recs[10 * k:10 * k + 10] for k in range(5)]
    with bw.BamMerger(str(tmp_path), 0) as m:
        for k in (4, 2, 0, 3, 1):
            m.add(k, *sref.run_arrays(runs[k], _key_of))
        out = str(tmp_path / "t.bgzf")
        fd = os.open(out, os.O_WRONLY | os.O_CREAT, 0o644)
        m.finish(fd, 1, 2)
        os.close(fd)
    assert gzip.decompress(open(out, "rb").read()) == b"".join(recs)


def test_merger_refuses_what_it_must(golden_records, tmp_path):
    run = sref.run_arrays(sref.stable_sort(golden_records[:200]), _key_of)
    with bw.BamMerger(str(tmp_path), 1 << 30) as m:
        m.add(3, *run)
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            m.add(3, *run)                                          # a run number given twice
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            m.add(4, run[0], run[1], run[2][:-1] - 1)               # offsets that do not span the bytes
        assert m.stats()["n_runs"] == 1
    for bad in (str(tmp_path / "does_not_exist"), __file__):       # no directory files can be made in
        with pytest.raises(bw.BwahipError, match="EIO"):
            bw.BamMerger(bad, 0)
    if os.geteuid() != 0:                                           # (root writes everywhere)
        ro = tmp_path / "ro"
        ro.mkdir()
        ro.chmod(0o555)
        with pytest.raises(bw.BwahipError, match="EIO"):
            bw.BamMerger(str(ro), 0)
    # no run, and only an empty run: no record block at all
    for runs in ([], [0]):
        with bw.BamMerger(str(tmp_path), 0) as m:
            for k in runs:
                m.add(k, b"", np.zeros(0, np.uint64), np.zeros(1, np.int64))
            out = str(tmp_path / "e.bgzf")
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            m.finish(fd, 1, 1)
            os.close(fd)
            assert os.path.getsize(out) == 0 and m.stats()["n_records"] == 0
            os.unlink(out)
    assert sorted(os.listdir(tmp_path)) == (["ro"] if os.geteuid() != 0 else [])


def test_merger_spill_write_failure_is_eio_and_leaves_no_file(golden_records, tmp_path):
    """A spill that cannot be written in full (file size limit) is BWAHIP_EIO, in a child process so that the limit stays there."""
    code = f"""
import os, resource, signal, sys
sys.path.insert(0, {os.path.join(common.ROOT, 'tests')!r})
import numpy as np
import common
from common import bw
signal.signal(signal.SIGXFSZ, signal.SIG_IGN)
resource.setrlimit(resource.RLIMIT_FSIZE, (4096, 4096))
n = 4000
rec = b"x" * (40 * n)
m = bw.BamMerger({str(tmp_path)!r}, 0)
try:
    m.add(0, rec, np.arange(n, dtype=np.uint64), np.arange(n + 1, dtype=np.int64) * 40)
    print("no error")
except bw.BwahipError as e:
    print("error", e)
left = os.listdir({str(tmp_path)!r})
m.close()
print(left, os.listdir({str(tmp_path)!r}))
"""
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "error" in r.stdout and "EIO" in r.stdout and r.stdout.strip().endswith("[] []"), r.stdout


# ------------------------------------------------------------------------------------------------------------------- header
def test_sorted_header(built):
    bns, _keep = _bns(GOLDEN_CONTIGS, GOLDEN_LENS)
    for hdr in (None, "@RG\tID:grp7\tSM:sample", "@SQ\tSN:ctg1\tLN:40000\tM5:x\n@SQ\tSN:ctg2\tLN:16000\n@SQ\tSN:ctg3\tLN:4000\n@PG\tID:bwa"):
        plain, srt = bw.bam_header(bns, hdr), bw.bam_header_sorted(bns, hdr)
        assert srt[:4] == b"BAM\1"
        (l_plain,), (l_text,) = struct.unpack_from("<i", plain, 4), struct.unpack_from("<i", srt, 4)
        assert l_text == l_plain + len(sref.HD) and len(srt) == len(plain) + len(sref.HD)
        text = srt[8:8 + l_text]
        assert text.startswith(sref.HD.encode()) and text.split(b"\n")[0] == b"@HD\tVN:1.6\tSO:coordinate"
        assert text[len(sref.HD):] == plain[8:8 + l_plain]                      # the rest of the text: exactly bwahip_bam_header's
        assert srt[8 + l_text:] == plain[8 + l_plain:]                          # and its reference table
    for own in ("@HD\tVN:1.6", "@HD\tVN:1.5\tSO:unsorted\n@PG\tID:x", "@PG\tID:x\n@HD\tVN:1.6"):
        out, ln = C.c_void_p(), C.c_int64()
        assert bw.lib().bwahip_bam_header_sorted(C.byref(bns), own.encode(), C.byref(out), C.byref(ln)) == -1
    bw.bam_header_sorted(bns, "@CO\tnot an @HD line")                          # "@HD" inside a line is nobody's header line


# ------------------------------------------------------------------------------------------------------------------- key
def test_sort_key_is_monotone_and_documented(built):
    names, lens = ["a", "b", "c", "d"], [1000, 65535, 7, 2 ** 20]
    bns, _keep = _bns(names, lens)
    n, longest = len(names), max(lens)
    corners = []                                                                 # (refID, pos, reverse) in the order of the contract
    for rid in range(n):
        for pos in sorted({0, 1, 2, lens[rid] // 2, lens[rid] - 2, lens[rid] - 1}):
            if pos >= 0:
                corners += [(rid, pos, 0), (rid, pos, 1)]
    corners += [(-1, -1, 0), (-1, -1, 1)]
    assert corners[0] == (0, 0, 0) and (n - 1, lens[-1] - 1, 1) in corners
    keys = [bw.bam_sort_key(bns, *c) for c in corners]
    assert all(a < b for a, b in zip(keys, keys[1:])), "the key is not strictly monotone in (refID unsigned, pos, strand)"
    assert sorted(corners, key=lambda c: (c[0] & 0xffffffff, c[1], c[2])) == corners
    pos_bits = (longest + 1).bit_length()
    for (rid, pos, rev), k in zip(corners, keys):
        assert k == ((n if rid < 0 else rid) << (pos_bits + 1) | (pos + 1) << 1 | rev)
    bits = bw.bam_sort_key_bits(bns)
    assert bits == 1 + pos_bits + n.bit_length() and max(keys) < 1 << bits
    # an unmapped read placed at its mate's position sorts with the mate: the key has no "unmapped" bit
    assert bw.bam_sort_key(bns, 1, 500, 0) < bw.bam_sort_key(bns, 1, 500, 1) < bw.bam_sort_key(bns, 1, 501, 0)


def test_sort_key_fits_64_bits_for_any_index(built):
    """n_seqs and contig lengths are int32: the widest key is 1 + 32 + 31 bits.  The corner -- 2^31 - 2 contigs, the longest of 2^31 - 1
    bases -- goes through the library's width and packing code by the two numbers alone (a contig table of that size would take 80 GB);
    a table of 2^20 contigs checks that the table form computes the same."""
    N, L = 2 ** 31 - 2, 2 ** 31 - 1
    assert bw.bam_sort_key_bits_for(N, L) == 64
    assert bw.bam_sort_key_bits_for(N + 1, L) == 64                              # the most an int32 holds
    corner = [bw.bam_sort_key_for(N, L, *c) for c in ((0, 0, 0), (0, 0, 1), (0, L - 1, 1), (1, 0, 0), (N - 1, 0, 0), (N - 1, L - 1, 0), (N - 1, L - 1, 1), (-1, -1, 0), (-1, -1, 1))]
    assert all(a < b for a, b in zip(corner, corner[1:])) and corner[-1] == (N << 33 | 1) < 1 << 64
    assert corner[-3] == ((N - 1) << 33 | L << 1 | 1) and corner[0] == 2
    n = 1 << 20
    anns = (bw.Ann * n)()
    anns[n - 1].len = 2 ** 31 - 1
    bns = bw.Bns()
    bns.n_seqs, bns.anns = n, anns
    assert bw.bam_sort_key_bits(bns) == 1 + 32 + 21 == bw.bam_sort_key_bits_for(n, 2 ** 31 - 1)
    assert bw.bam_sort_key(bns, n - 1, 5, 1) == bw.bam_sort_key_for(n, 2 ** 31 - 1, n - 1, 5, 1)
    top = bw.bam_sort_key(bns, -1, -1, 1)
    assert top == (n << 33 | 1) and bw.bam_sort_key(bns, n - 1, 2 ** 31 - 2, 1) == ((n - 1) << 33 | (2 ** 31 - 1) << 1 | 1) < top
    bns.n_seqs = 0                                                              # no contig: every record has refID -1, pos -1 -- strand and one position bit
    assert bw.bam_sort_key_bits(bns) == 2 and bw.bam_sort_key(bns, -1, -1, 1) == 1
    for n_small, want in ((1, 1), (2, 2), (3, 2), (4, 3), (255, 8), (256, 9)):
        bns.n_seqs = n_small
        for i in range(n_small):
            anns[i].len = 99
        assert bw.bam_sort_key_bits(bns) == 1 + (100).bit_length() + want


# ------------------------------------------------------------------------------------------------------------------- sanitizers
def test_merger_under_asan_ubsan(golden_records, tmp_path):
    """csrc/bam_sort_host.cpp + csrc/bam_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (tests/san_bam_sort_driver.cpp): the
    scenario of the merger test -- 17 uneven runs, one empty, added in shuffled order from three threads, for three budgets and two
    levels; a duplicate run number and a missing directory -- must end without a report and give the global stable sort."""
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17"]
    exe = str(tmp_path / "san_bam_sort")
    r = subprocess.run(["g++", *san, "-o", exe, os.path.join(common.ROOT, "tests", "san_bam_sort_driver.cpp"), os.path.join(CSRC, "bam_sort_host.cpp"),
                        os.path.join(CSRC, "bam_host.cpp"), "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = random.Random(17)
    runs = sref.make_runs(golden_records, 17, rng, empty=1)
    order = list(range(17))
    rng.shuffle(order)
    inp = str(tmp_path / "runs.bin")
    with open(inp, "wb") as f:                                     # n_runs, then per run (in the order they are to be added): run_no, n_rec, len, keys, offsets, bytes
        f.write(struct.pack("<q", len(order)))
        for k in order:
            rec, keys, off = sref.run_arrays(runs[k], _key_of)
            f.write(struct.pack("<qqq", k, len(keys), len(rec)) + keys.tobytes() + off.tobytes() + rec)
    want = b"".join(sref.stable_sort(golden_records))
    total = sum(len(b"".join(x)) + 16 * len(x) + 8 for x in runs)
    spill = tmp_path / "spill"
    spill.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for budget in (0, total // 2, 1 << 30):
        for level in (0, 1):
            out = str(tmp_path / "san.bgzf")
            r = subprocess.run([exe, inp, str(spill), str(budget), str(level), out], capture_output=True, env=env)
            err = r.stderr.decode(errors="replace")
            assert r.returncode == 0 and "runtime error" not in err and "AddressSanitizer" not in err, err[-3000:]
            assert gzip.decompress(open(out, "rb").read()) == want
            assert os.listdir(spill) == []
