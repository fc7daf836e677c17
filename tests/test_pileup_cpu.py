"""The pileup of candidate variant sites, the parts that need no GPU: the device-free builder (csrc/pileup_host.cpp), bwahip_pileup_hbm_need,
and the builder under the sanitizers through a stand-alone program.  The judge is tests/pileup_ref.py -- plain Python written from the rule
in include/bwahip.h.  Byte for byte, no tolerance."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import common
import pileup_cases as cases
import pileup_ref as ref
from common import bw
from pileup_cases import BIG, M, QUIET, rec

CSRC = os.path.join(common.ROOT, "bwa-mem-gpu_amd", "csrc")
OPTS = [(), (0, cases.MIN_BASEQ, -1, 1), (cases.MIN_MAPQ, 0, -1, 3), (0, cases.MIN_BASEQ, 0, 2), (20, 19, 0x400, 2)]


@pytest.fixture(scope="module")
def case(built):
    c = cases.record_set()
    cases.assert_families(c)
    c["want"] = {o: ref.build(c["records"], c["ref_len"], c["pac"], o) for o in OPTS}
    return c


def _feed(c, how, opt, tmp_path, seed=0):
    out = str(tmp_path / "x.bpu")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.PileupBuilder(c["ref_len"], c["pac"], opt) as b:
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


def test_builder_does_not_mind_the_order(case, tmp_path):
    recs = list(case["records"])
    random.Random(5).shuffle(recs)
    for opt in OPTS[:2]:
        assert _feed(cases.make_case(recs, case["refs"], shift=13), "at once", opt, tmp_path) == case["want"][opt]


def test_the_judge_reads_what_it_writes_and_the_options_matter(case):
    w = case["want"]
    s = ref.parse(w[()])
    assert s == ref.pileup(case["records"], case["ref_len"], case["pac"]) and s["opt"] == (0, 0, 1796, 2) and ref.serialise(s) == w[()]
    assert len(w[()]) == 64 + 28 * len(s["sites"]) + 20 * sum(len(x["alleles"]) for x in s["sites"])
    assert len({w[o] for o in OPTS}) == len(OPTS)
    n_sites = lambda o: len(ref.parse(w[o])["sites"])
    assert n_sites((0, cases.MIN_BASEQ, -1, 1)) > n_sites(()) > n_sites((cases.MIN_MAPQ, 0, -1, 3)) > 0
    keys = [(x["ref"], x["pos"]) for x in s["sites"]]
    assert keys == sorted(set(keys)) and all(x["alleles"] == sorted(x["alleles"], key=lambda a: (a["kind"], a["len"], a["bases"])) for x in s["sites"])


def test_no_record_and_no_observation(built, tmp_path):
    refs = cases.reference()
    lens, pac = cases.REF_LEN, ref.pack_reference(refs)
    for opt in ((), (0, 0, 0, 1)):
        want = ref.build([], lens, pac, opt)
        assert len(want) == 64 and _feed(cases.make_case([], refs), "at once", opt, tmp_path) == want
    quiet = [rec(b"a", BIG, 100, [(50, M)], cases.read_over(refs, BIG, 100, [(50, M)])), rec(b"b", -1, -1, [], [1, 2, 4], flag=0x4),
             rec(b"c", QUIET, 7, [(4, cases.S), (9, M)], [15] * 4 + cases.read_over(refs, QUIET, 7, [(9, M)]), flag=0x10)]
    for shift in (0, 13):
        c = cases.make_case(quiet, refs, shift=shift)
        want = ref.build(quiet, lens, pac, (0, 0, -1, 1))
        assert len(want) == 64 and ref.parse(want)["n_obs"] == [0, 0, 0] and _feed(c, "at once", (0, 0, -1, 1), tmp_path) == want
    none = rec(b"b", -1, -1, [], [], flag=0x4)
    with bw.PileupBuilder([], None, ()) as b:                        # no reference at all: every record must be without one
        b.add_records(none, [0, len(none)])
        b.finish(-1)
    with bw.PileupBuilder([0, 5], bytes(2), (0, 0, -1, 1)) as b:      # a reference of no bases
        one = rec(b"x", 1, 0, [(5, M)], [8] * 5)
        b.add_records(one, [0, len(one)])
        b.finish(-1)


def test_refusals(case, tmp_path):
    good = case["records"][:50]
    for what, (bad, refused) in cases.bad_records().items():
        for recs in ([bad] + good, good + [bad]):
            c = cases.make_case(recs, case["refs"])
            if refused:
                with pytest.raises(ref.BadRecord):
                    ref.build(recs, c["ref_len"], c["pac"])
                for how in ("at once", "one by one"):
                    with pytest.raises(bw.BwahipError, match="EINVAL"):
                        _feed(c, how, (), tmp_path)
                    assert os.path.getsize(str(tmp_path / "x.bpu")) == 0, what
            else:
                assert _feed(c, "at once", (), tmp_path) == ref.build(recs, c["ref_len"], c["pac"]), what
    for opt in ((-1, 0, -1, 0), (256, 0, -1, 0), (0, -1, -1, 0), (0, 94, -1, 0), (0, 0, 65536, 0), (0, 0, -1, -1), (0, 0, -1, 65536)):
        with pytest.raises(ValueError):
            ref.resolve(*opt)
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            bw.PileupBuilder(cases.REF_LEN, case["pac"], opt)
    for lens in ([5, -1], [1 << 31]):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            bw.PileupBuilder(lens, case["pac"], ())
    with pytest.raises(bw.BwahipError, match="ECAPACITY"):            # 2^40 bases: a position no longer fits the key (refused before the reference is read)
        bw.PileupBuilder([(1 << 31) - 1] * 513, case["pac"], ())
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        bw.PileupBuilder(cases.REF_LEN, None, ())
    with bw.PileupBuilder(cases.REF_LEN, case["pac"], ()) as b:       # after a refusal every later call says the same
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            b.add_records(bytes(20), [0, 20])
        for call in (lambda: b.add_records(good[0], [0, len(good[0])]), lambda: b.finish(-1)):
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                call()


def test_abi_mirrors_and_hbm_need(built):
    L = bw.lib()
    for name in ("bwahip_pileup_builder_open", "bwahip_pileup_builder_add_records", "bwahip_pileup_builder_finish", "bwahip_pileup_builder_close", "bwahip_kat_pileup",
                 "bwahip_bam_devmerger_set_pileup", "bwahip_pileup_hbm_need", "bwahip_stream_run_bam_sorted_dev_pileup"):
        assert hasattr(L, name), name
    assert C.sizeof(bw.PileupOpt) == 16 and C.sizeof(bw.PileupStats) == 88
    hdr = open(os.path.join(common.ROOT, "include", "bwahip.h")).read()
    assert "typedef struct { int min_mapq, min_baseq, exclude_flags, min_alt; } bwahip_pileup_opt_t;" in hdr
    need = bw.pileup_hbm_need
    # by hand from the header's terms: 12 bytes per record and 4 096; an eighth of slack
    assert need(0) == 4096 + 512 and need(4_000_000) == 48_004_096 + 48_004_096 // 8 and need(-1) == -1


def _fnv(data):
    h = 1469598103934665603
    for x in data:
        h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
    return h


def test_builder_under_asan_ubsan(case, tmp_path):
    """csrc/pileup_host.cpp under AddressSanitizer and UndefinedBehaviorSanitizer through the stand-alone tests/san_pileup_driver.cpp (plain
    g++, run as a child process): the case set in three feeding modes must end without a report and print the digest of the judge's bytes;
    records cut short -- each in an allocation of its own size -- must end as refusals or count as they are, without a report."""
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17"]
    exe = str(tmp_path / "san_pileup")
    r = subprocess.run(["g++", *san, "-o", exe, os.path.join(common.ROOT, "tests", "san_pileup_driver.cpp"), os.path.join(CSRC, "pileup_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for opt in ((), (0, cases.MIN_BASEQ, -1, 1), (20, 19, 0x400, 2)):
        o = opt or (0, 0, -1, 0)
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bpu")
        lens = np.asarray(case["ref_len"], dtype=np.int64)
        with open(inp, "wb") as f:
            f.write(struct.pack("<i", len(lens)) + lens.tobytes() + case["pac"] + struct.pack("<iiiiq", *o, len(case["records"])) + case["off"].tobytes() + case["buf"])
        r = subprocess.run([exe, inp, out], capture_output=True, env=env)
        err = r.stderr.decode(errors="replace")
        assert "runtime error" not in err and "AddressSanitizer" not in err and "LeakSanitizer" not in err, err[-3000:]
        assert r.returncode == 0, err[-3000:]
        want = case["want"][opt]
        digest, size, n_cut = r.stdout.split()
        assert (int(digest, 16), int(size)) == (_fnv(want), len(want)) and int(n_cut) >= 1500
        assert open(out, "rb").read() == want
