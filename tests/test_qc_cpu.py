"""The QC summary of coordinate-sorted BAM, the parts that need no GPU: the device-free builder (csrc/qc_host.cpp), the host merger that
feeds it, bwahip_qc_hbm_need, and the builder under the sanitizers through a stand-alone program.  The judge is tests/qc_ref.py -- plain
Python written from the rule in include/bwahip.h.  Byte for byte, no tolerance."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bam_sort_ref as sref
import bgzf_ref
import common
import qc_cases as cases
import qc_ref as ref
from common import bw
from qc_cases import M, rec

CSRC = os.path.join(common.ROOT, "bwa-mem-gpu_amd", "csrc")
OPTS = [(), (4, -1, 0), (8, -1, 0), (29, -1, 0), (0, 0, 0), (0, -1, 30), (5, 0x10, 4)]


@pytest.fixture(scope="module")
def case(built):
    c = cases.record_set()
    cases.assert_families(c)
    c["want"] = {o: ref.build(c["records"], c["ref_len"], o) for o in OPTS}
    return c


def _feed(c, how, opt, tmp_path, seed=0):
    out = str(tmp_path / "x.bqc")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.QcBuilder(c["ref_len"], opt) as b:
            off, buf, n = c["off"], c["buf"], len(c["off"]) - 1
            if how == "at once":
                b.add_records(buf, off)
            elif how == "one by one":
                for i in range(n):
                    b.add_records(buf[off[i]:off[i + 1]], [0, off[i + 1] - off[i]])
            else:                                                   # slices of uneven size in shuffled order, the offsets not starting at 0
                rng, i, parts = random.Random(seed), 0, []
                while i < n:
                    j = min(n, i + rng.randrange(1, 300))
                    parts.append((i, j))
                    i = j
                rng.shuffle(parts)
                for i, j in parts:
                    b.add_records(buf[:off[j]], off[i:j + 1])
            b.finish(fd)
    finally:
        os.close(fd)
    return open(out, "rb").read()


@pytest.mark.parametrize("how", ["at once", "one by one", "slices"])
def test_builder_equals_the_judge_for_every_cut(case, tmp_path, how):
    for opt in (OPTS if how != "one by one" else OPTS[:2]):
        got = _feed(case, how, opt, tmp_path, seed=len(opt))
        assert got == case["want"][opt], f"{how}, options {opt}: {ref.first_difference(got, case['want'][opt])}"


def test_the_judge_reads_what_it_writes_and_the_options_matter(case):
    w = case["want"]
    s = ref.parse(w[()])
    assert s == ref.summary(case["records"], case["ref_len"]) and s["opt"] == (14, 1796, 0) and ref.serialise(s) == w[()]
    assert len(w[()]) == 12580 + 48 * len(case["ref_len"]) + 8 * sum((n + 16383) >> 14 for n in case["ref_len"])
    assert len({w[o] for o in OPTS}) == len(OPTS)
    assert all(len(r["windows"]) == 1 and r["windows"][0] == r["depth_sum"] for r in ref.parse(w[(29, -1, 0)])["refs"])
    covered = lambda o: sum(r["depth_sum"] for r in ref.parse(w[o])["refs"])
    assert covered((0, 0, 0)) > covered(()) > covered((0, -1, 30))
    assert sum(s["depth_hist"]) == sum(case["ref_len"]) and s["depth_hist"][254] >= 5 and s["depth_hist"][255] >= 15   # 255: depth 255, 256 and 306


def test_no_record_one_record_and_a_shift(built, tmp_path):
    lens = cases.REF_LEN
    for opt in ((), (4, 0, 0)):
        c = cases.make_case([])
        want = ref.build([], lens, opt)
        s = ref.parse(want)
        assert s["depth_hist"] == [sum(lens)] + [0] * 255 and not any(map(any, s["count"])) and not any(any(r["windows"]) for r in s["refs"])
        assert _feed(c, "at once", opt, tmp_path) == want
    for one in (rec(b"a", 3, 7, [(10, M)]), rec(b"b", -1, -1, [], 0x4), rec(b"c", 16, 2040, [(100, M)], 0x400)):
        for shift in (0, 13):
            c = cases.make_case([one], shift=shift)
            assert _feed(c, "at once", (), tmp_path) == ref.build([one], lens)
    with bw.QcBuilder([], ()) as b:                                  # no reference at all: every record must be without one
        b.add_records(rec(b"b", -1, -1, [], 0x4), [0, len(rec(b"b", -1, -1, [], 0x4))])
    with bw.QcBuilder([0, 5], (4, -1, 0)) as b:                       # a reference of no bases has no window
        b.finish(-1)


def test_refusals(case, tmp_path):
    good = case["records"][:50]
    for what, (bad, refused) in cases.bad_records().items():
        for recs in ([bad] + good, good + [bad]):
            c = cases.make_case(recs)
            if refused:
                with pytest.raises(ref.BadRecord):
                    ref.build(recs, c["ref_len"])
                for how in ("at once", "one by one"):
                    with pytest.raises(bw.BwahipError, match="EINVAL"):
                        _feed(c, how, (), tmp_path)
                    assert os.path.getsize(str(tmp_path / "x.bqc")) == 0, what
            else:
                assert _feed(c, "at once", (), tmp_path) == ref.build(recs, c["ref_len"]), what
    for opt in ((3, -1, 0), (30, -1, 0), (-1, -1, 0), (0, 65536, 0), (0, -1, -1), (0, -1, 256)):
        with pytest.raises(ValueError):
            ref.resolve(*opt)
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            bw.QcBuilder(cases.REF_LEN, opt)
    for lens in ([5, -1], [1 << 31]):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            bw.QcBuilder(lens, ())
    with bw.QcBuilder(cases.REF_LEN, ()) as b:                        # after a refusal every later call says the same
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            b.add_records(bytes(20), [0, 20])
        for call in (lambda: b.add_records(good[0], [0, len(good[0])]), lambda: b.finish(-1)):
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                call()


def test_host_merger_feeds_the_builder(case, tmp_path):
    key_of = lambda r: sref.packed_key(r, len(cases.REF_LEN), 2 ** 31 - 1)
    rng = random.Random(9)
    runs = sref.make_runs(case["records"], 5, rng, empty=2)
    want_recs = sref.stable_sort(case["records"])
    spill = tmp_path / "spill"
    spill.mkdir()
    files, opt = [], (8, -1, 0)
    for listen in (False, True):
        out, qc = str(tmp_path / f"m{listen}.bgzf"), str(tmp_path / "m.bqc")
        fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        with bw.BamMerger(str(spill), 100000) as m:
            for k in (3, 0, 4, 1, 2):
                m.add(k, *sref.run_arrays(runs[k], key_of))
            if listen:
                fq = os.open(qc, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                with bw.QcBuilder(case["ref_len"], opt) as b:
                    m.set_qc(b)
                    m.finish(fd, 1, 3)
                    b.finish(fq)
                    m.set_qc(None)
                os.close(fq)
            else:
                m.finish(fd, 1, 3)
        os.close(fd)
        files.append(open(out, "rb").read())
    assert files[0] == files[1] and bgzf_ref.inflate(files[1]) == b"".join(want_recs)
    got = open(qc, "rb").read()
    assert got == case["want"][opt], ref.first_difference(got, case["want"][opt])


def test_abi_mirrors_and_hbm_need(built):
    L = bw.lib()
    for name in ("bwahip_qc_builder_open", "bwahip_qc_builder_add_records", "bwahip_qc_builder_finish", "bwahip_qc_builder_close", "bwahip_bam_merger_set_qc", "bwahip_kat_qc",
                 "bwahip_bam_devmerger_set_qc", "bwahip_qc_hbm_need", "bwahip_stream_run_bam_sorted_dev_qc"):
        assert hasattr(L, name), name
    assert C.sizeof(bw.QcOpt) == 12 and C.sizeof(bw.QcStats) == 48
    hdr = open(os.path.join(common.ROOT, "include", "bwahip.h")).read()
    assert "typedef struct { int window_shift, exclude_flags, min_mapq; } bwahip_qc_opt_t;" in hdr
    need = bw.qc_hbm_need
    # by hand from the header's terms: S = sum_len + 2048 n_ref; 4 S + 16 (S / 2048 + n_ref + 1) + 8 (1570 + 3 n_ref + windows) + 24 (n_ref + 1) + 4096; an eighth of slack
    assert need(0, 0, 0, 0) == 16696 + 16696 // 8                                          # 16 + 12 560 + 24 + 4096
    S = 3_100_000_000 + 2048 * 25
    w = 4 * S + 16 * (S // 2048 + 26) + 8 * (1570 + 75 + 189_220) + 24 * 26 + 4096
    assert need(25, 3_100_000_000, 189_220, 4_000_000) == w + w // 8 and need(25, 3_100_000_000, 189_220, 0) == w + w // 8   # nothing per record
    assert all(need(*a) == -1 for a in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)))


def _fnv(data):
    h = 1469598103934665603
    for x in data:
        h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
    return h


def test_builder_under_asan_ubsan(case, tmp_path):
    """csrc/qc_host.cpp under AddressSanitizer and UndefinedBehaviorSanitizer through the stand-alone tests/san_qc_driver.cpp (plain g++,
    run as a child process): the case set in three feeding modes must end without a report and print the digest of the judge's bytes;
    records cut short -- each in an allocation of its own size -- must end as refusals, without a report."""
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17"]
    exe = str(tmp_path / "san_qc")
    r = subprocess.run(["g++", *san, "-o", exe, os.path.join(common.ROOT, "tests", "san_qc_driver.cpp"), os.path.join(CSRC, "qc_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for opt in ((), (5, 0x10, 4), (0, -1, 30)):
        o = opt or (0, -1, 0)
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bqc")
        lens = np.asarray(case["ref_len"], dtype=np.int64)
        with open(inp, "wb") as f:
            f.write(struct.pack("<i", len(lens)) + lens.tobytes() + struct.pack("<iiiq", *o, len(case["records"])) + case["off"].tobytes() + case["buf"])
        r = subprocess.run([exe, inp, out], capture_output=True, env=env)
        err = r.stderr.decode(errors="replace")
        assert "runtime error" not in err and "AddressSanitizer" not in err and "LeakSanitizer" not in err, err[-3000:]
        assert r.returncode == 0, err[-3000:]
        want = case["want"][opt]
        digest, size, n_cut = r.stdout.split()
        assert (int(digest, 16), int(size)) == (_fnv(want), len(want)) and int(n_cut) >= 1500
        assert open(out, "rb").read() == want
