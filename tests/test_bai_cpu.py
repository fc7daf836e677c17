"""The BAI index beside a coordinate-sorted BAM file, the parts that need no GPU: the device-free builder (csrc/bai_host.cpp), the host
merger that feeds it, bwahip_bgzf_write_lens, and the builder under the sanitizers.  The judges are tests/bai_ref.py: (a) the canonical
bytes restated in Python from the specification and include/bwahip.h, (b) a reader by reg2bins and the linear index, which holds for any
valid index.  Byte for byte, no tolerance."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bai_cases as cases
import bai_ref
import bam_sort_ref as sref
import bgzf_ref
import common
from bai_cases import D, M, N, S, rec
from common import bw

CSRC = os.path.join(common.ROOT, "bwa-mem-gpu_amd", "csrc")


@pytest.fixture(scope="module")
def sets(built):
    """The synthetic set, ending inside a block and on a block cut, with the judge's bytes (made once)."""
    out = []
    for whole in (False, True):
        c = cases.synthetic(whole)
        c["want"] = bai_ref.build(c["records"], c["offsets"], c["n_ref"])
        cases.assert_families(c, c["want"])
        out.append(c)
    return out


def _feed(c, how, tmp_path, seed=0):
    """The builder's bytes for case c, records and members fed as `how` says."""
    out = str(tmp_path / "x.bai")
    fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with bw.BaiBuilder(c["n_ref"], c["base"]) as b:
            off, lens, buf = c["rec_off"], c["lens"], c["buf"]
            if how == "records first":
                b.add_records(buf, off)
                b.add_members(lens)
            elif how == "members first":
                b.add_members(lens)
                b.add_records(buf, off)
            elif how == "one by one":
                rng, fed = random.Random(seed), 0
                for i in range(len(off) - 1):
                    b.add_records(buf[off[i]:off[i + 1]], [0, off[i + 1] - off[i]])
                    k = rng.choice((0, 0, 0, 1, 2))
                    b.add_members(lens[fed:fed + k])
                    fed = min(len(lens), fed + k)
                b.add_members(lens[fed:])
            else:                                                   # slices of uneven size, the offsets not starting at 0
                rng, i, fed = random.Random(seed), 0, 0
                n = len(off) - 1
                while i < n:
                    j = min(n, i + rng.randrange(1, 40))
                    b.add_records(buf[:off[j]], off[i:j + 1])
                    k = rng.randrange(0, 3)
                    b.add_members(lens[fed:fed + k])
                    fed = min(len(lens), fed + k)
                    i = j
                b.add_members(lens[fed:])
            b.finish(fd)
    finally:
        os.close(fd)
    return open(out, "rb").read()


@pytest.mark.parametrize("how", ["records first", "members first", "one by one", "slices"])
def test_builder_writes_the_canonical_index(sets, tmp_path, how):
    for c in sets:
        got = _feed(c, how, tmp_path, seed=5)
        assert got == c["want"], f"{how}, total {c['total']}"


def test_semantics_every_overlapping_record_lies_in_a_returned_chunk(sets, tmp_path):
    for c in sets:
        got = _feed(c, "records first", tmp_path)
        regions = bai_ref.regions_of(c["records"], c["n_ref"]) + [(1, 0, 1 << 29), (4, 5, 6), (0, (1 << 29) - 1, 1 << 29)]
        assert bai_ref.check_semantics(got, c["records"], c["offsets"], c["n_ref"], regions) > 10000
        # the judge can fail: an index that lost a chunk is caught
        idx = bai_ref.parse(got)
        beg, end = idx["refs"][0]["bins"][4681][1]
        broken = got.replace(struct.pack("<QQ", beg, end), struct.pack("<QQ", beg, beg + 1), 1)
        with pytest.raises(AssertionError):
            bai_ref.check_semantics(broken, c["records"], c["offsets"], c["n_ref"], regions)


def test_no_record_and_one_record(built, tmp_path):
    c = cases.make_case([])
    want = bai_ref.build([], c["offsets"], c["n_ref"])
    assert want == b"BAI\1" + struct.pack("<i", 5) + bytes(8 * 5) + bytes(8)
    for how in ("records first", "members first"):
        assert _feed(c, how, tmp_path) == want
    for one in (rec(3, 77, [(10, M)]), rec(-1, -1, [], flag=4), rec(0, 16383, [(2, M)], size=BLOCK_ALIGNED)):
        c = cases.make_case([one])
        want = bai_ref.build([one], c["offsets"], c["n_ref"])
        for how in ("records first", "members first", "one by one"):
            assert _feed(c, how, tmp_path) == want
        assert bai_ref.check_semantics(want, [one], c["offsets"], c["n_ref"]) >= 0


BLOCK_ALIGNED = 2 * 65280


def _refused(records, code, tmp_path, n_ref=cases.N_REF, lens=None):
    c = cases.make_case(records, n_ref=n_ref)
    if lens is not None:
        c["lens"] = np.asarray(lens, dtype=np.int32)
    else:
        with pytest.raises(bai_ref.Refused, match=code):           # the judge refuses the same
            bai_ref.build(records, c["offsets"], n_ref)
    out = str(tmp_path / "x.bai")
    for how in ("records first", "members first", "one by one"):
        with pytest.raises(bw.BwahipError, match=code):
            _feed(c, how, tmp_path)
        assert os.path.getsize(out) == 0, "bytes of an index that was refused"


def test_refusals(built, tmp_path):
    good = cases.ordinary(3000)
    raw = lambda n, ref=0, pos=5000: struct.pack("<iiiBBHHH", n - 4, ref, pos, 1, 0, 0, 0, 0) + bytes(n - 20)
    bad_size = bytearray(rec(0, 5000, [(10, M)]))
    bad_size[0] += 1
    long_cigar = bytearray(rec(0, 5000, [(10, M)]))
    struct.pack_into("<H", long_cigar, 16, 2)                       # two operations announced, room for one
    long_name = bytearray(rec(0, 5000, [(10, M)]))
    long_name[12] = 200
    for bad in (raw(20), raw(35), bytes(bad_size), bytes(long_cigar), bytes(long_name), rec(cases.N_REF, 5000, [(10, M)]), rec(0x7fffffff, 0), rec(0, -1, [(10, M)])):
        _refused(good[:3] + [bad] + good[3:], "EINVAL", tmp_path)
        _refused([bad] + good, "EINVAL", tmp_path)
    _refused([rec(0, 10), rec(0, 9)], "EINVAL", tmp_path)            # not in coordinate order: pos
    _refused([rec(1, 10), rec(0, 11)], "EINVAL", tmp_path)           # refID
    _refused([rec(-1, -1, flag=4), rec(0, 11)], "EINVAL", tmp_path)  # refID as unsigned: -1 comes last
    _refused(good + [rec(0, (1 << 29) - 99, [(100, M)])], "ECAPACITY", tmp_path)      # e = 2^29 + 1
    _refused(good + [rec(0, 1 << 29, [(1, M)])], "ECAPACITY", tmp_path)
    _refused(good + [rec(0, 100000, [(1 << 27, N), (1 << 27, D), (1 << 27, N), (1 << 27, N), (1 << 27, M)])], "ECAPACITY", tmp_path)   # rlen beyond int32's half
    _refused([rec(0, (1 << 29) - 99, [(100, M)]), raw(20)], "ECAPACITY", tmp_path)   # the first offending record decides
    _refused([raw(20), rec(0, (1 << 29) - 99, [(100, M)])], "EINVAL", tmp_path)
    c = cases.make_case(good)
    assert _feed(c, "slices", tmp_path) == bai_ref.build(good, c["offsets"], c["n_ref"])   # and e = 2^29 exactly is in the synthetic set
    _refused(good, "EINVAL", tmp_path, lens=[1000, 1000])            # members that are not those of the records
    _refused(good, "EINVAL", tmp_path, lens=[])
    _refused(good, "EINVAL", tmp_path, lens=[65537])
    _refused(good, "EINVAL", tmp_path, lens=[0])
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        bw.BaiBuilder(-1, 0)
    with bw.BaiBuilder(2, 0) as b:                                   # after a refusal every later call says the same
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            b.add_records(raw(20), [0, 20])
        for call in (lambda: b.add_members([100]), lambda: b.add_records(good[0], [0, len(good[0])]), lambda: b.finish(-1)):
            with pytest.raises(bw.BwahipError, match="EINVAL"):
                call()


def test_bin_is_computed_not_read(built, tmp_path):
    recs = [rec(0, 100, [(50, M)], bin_field=b) for b in (0, 4681, 9999, 65535)]
    c = cases.make_case(recs)
    got = _feed(c, "records first", tmp_path)
    assert got == bai_ref.build(recs, c["offsets"], c["n_ref"]) and list(bai_ref.parse(got)["refs"][0]["bins"]) == [4681]


def test_bgzf_write_lens(built, tmp_path):
    rng = random.Random(4)
    for n in (0, 1, 65279, 65280, 65281, 3 * 65280, 400000):
        data = bytes(rng.choices(b"ACGT", k=n // 2)) + rng.randbytes(n - n // 2)
        for level, threads in ((0, 1), (1, 1), (6, 3)):
            a, b = str(tmp_path / "a.bgzf"), str(tmp_path / "b.bgzf")
            fd = os.open(a, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            bw.bgzf_write(fd, data, level, threads)
            os.close(fd)
            fd = os.open(b, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            lens = bw.bgzf_write_lens(fd, data, level, threads)
            os.close(fd)
            got = open(b, "rb").read()
            assert got == open(a, "rb").read()
            assert lens.tolist() == [m["size"] for m in bgzf_ref.parse(got)] and int(lens.sum()) == len(got) and len(lens) == (n + 65279) // 65280
            assert bw.bgzf_write_lens(-1, data, level, threads).tolist() == lens.tolist()
    with pytest.raises(bw.BwahipError, match="ECAPACITY"):
        bw.bgzf_write_lens(-1, bytes(65281), 1, 1, cap=1)


def test_host_merger_feeds_the_builder(sets, tmp_path):
    c = sets[0]
    key_of = lambda r: sref.packed_key(r, cases.N_REF, 2 ** 31 - 1)
    rng = random.Random(9)
    shuffled = list(c["records"])
    rng.shuffle(shuffled)
    runs = sref.make_runs(shuffled, 5, rng, empty=2)
    want_recs = sref.stable_sort(shuffled)
    spill = tmp_path / "spill"
    spill.mkdir()
    files = []
    for with_bai in (False, True):
        out, bai = str(tmp_path / f"m{with_bai}.bgzf"), str(tmp_path / "m.bai")
        fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        with bw.BamMerger(str(spill), 100000) as m:
            for k in (3, 0, 4, 1, 2):
                m.add(k, *sref.run_arrays(runs[k], key_of))
            if with_bai:
                fb = os.open(bai, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                with bw.BaiBuilder(c["n_ref"], 777) as b:
                    m.finish_bai(fd, b, 1, 3)
                    b.finish(fb)
                os.close(fb)
            else:
                m.finish(fd, 1, 3)
        os.close(fd)
        files.append(open(out, "rb").read())
    assert files[0] == files[1] and bgzf_ref.inflate(files[1]) == b"".join(want_recs)
    offs = [777]
    for mem in bgzf_ref.parse(files[1]):
        offs.append(offs[-1] + mem["size"])
    got = open(bai, "rb").read()
    assert got == bai_ref.build(want_recs, offs, c["n_ref"])
    assert bai_ref.check_semantics(got, want_recs, offs, c["n_ref"]) > 1000


def test_abi_mirrors_and_sizes(built):
    L = bw.lib()
    for name in ("bwahip_bai_builder_open", "bwahip_bai_builder_add_records", "bwahip_bai_builder_add_members", "bwahip_bai_builder_finish", "bwahip_bai_builder_close",
                 "bwahip_bgzf_write_lens", "bwahip_bam_merger_finish_bai", "bwahip_bam_devmerger_finish_bai", "bwahip_kat_bai", "bwahip_bam_devmerge_bai_hbm_need",
                 "bwahip_bai_check_contigs", "bwahip_stream_run_bam_sorted_bai", "bwahip_stream_run_bam_sorted_dev_bai"):
        assert hasattr(L, name), name
    assert C.sizeof(bw.BaiStats) == 48 and [f[0] for f in bw.BaiStats._fields_] == ["n_chunks", "n_windows", "n_no_coor", "bai_bytes", "hbm_bytes", "index_ms"]
    hdr = open(os.path.join(common.ROOT, "include", "bwahip.h")).read()
    assert "typedef struct { int64_t n_chunks, n_windows, n_no_coor, bai_bytes, hbm_bytes; double index_ms; } bwahip_bai_stats_t;" in hdr
    need = bw.bam_devmerge_bai_hbm_need
    assert need(0, 0, 0, 0) == 8341 + 8341 // 8                                      # (29 + 52) + 12 + 56 + 8192, and the eighth of slack
    w = 81 * 1000001 + 12 * 4001 + 56 * 26 + 16 * 190000 + 8192
    assert need(1000000, 4000, 25, 190000) == w + w // 8
    assert all(need(*a) == -1 for a in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)))
    assert bw.bam_devmerge_hbm_need(10 ** 9, 10 ** 6, 10, 1024) == (lambda work: 10 ** 9 + 16 * 10 ** 6 + 80 + work + work // 8)(48 * 10 ** 6 + 1024 * (4 * 65280 + 62 + 65536 + 12) + (64 << 20))
    anns = (bw.Ann * 3)()
    bns = bw.Bns()
    bns.n_seqs, bns.anns = 3, anns
    anns[0].len, anns[1].len, anns[2].len = 1000, 1 << 29, 5
    bw.bai_check_contigs(bns)
    anns[1].len = (1 << 29) + 1
    with pytest.raises(bw.BwahipError, match="ECAPACITY"):
        bw.bai_check_contigs(bns)


def test_builder_under_asan_ubsan(sets, tmp_path):
    """csrc/bai_host.cpp (with bam_host.cpp and bam_sort_host.cpp, which it links against) under AddressSanitizer and
    UndefinedBehaviorSanitizer through tests/san_bai_driver.cpp: the synthetic set in every feeding mode must end without a report and
    give the judge's bytes; malformed records -- each in an allocation of its own size -- must end as refusals, without a report."""
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17"]
    exe = str(tmp_path / "san_bai")
    r = subprocess.run(["g++", *san, "-o", exe, os.path.join(common.ROOT, "tests", "san_bai_driver.cpp"), os.path.join(CSRC, "bai_host.cpp"),
                        os.path.join(CSRC, "bam_sort_host.cpp"), os.path.join(CSRC, "bam_host.cpp"), "-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(c, mode):
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bai")
        with open(inp, "wb") as f:
            f.write(struct.pack("<qqq", c["n_ref"], c["base"], len(c["records"])) + c["rec_off"].tobytes() + c["buf"] + struct.pack("<q", len(c["lens"])) + c["lens"].tobytes())
        r = subprocess.run([exe, inp, str(mode), out], capture_output=True, env=env)
        err = r.stderr.decode(errors="replace")
        assert "runtime error" not in err and "AddressSanitizer" not in err and "LeakSanitizer" not in err, err[-3000:]
        return r.returncode, (open(out, "rb").read() if r.returncode == 0 else None)

    for c in sets:
        for mode in (0, 1, 2):
            assert run(c, mode) == (0, c["want"]), mode
        z = str(tmp_path / "z.bgzf")                                 # mode 3: the lengths come from bwahip_bgzf_write_lens under the sanitizers
        fd = os.open(z, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        bw.bgzf_write(fd, c["buf"], 1, 1)
        os.close(fd)
        offs = [c["base"]]
        for mem in bgzf_ref.parse(open(z, "rb").read()):
            offs.append(offs[-1] + mem["size"])
        assert run(c, 3) == (0, bai_ref.build(c["records"], offs, c["n_ref"]))
    assert run(cases.make_case([]), 2) == (0, bai_ref.build([], [cases.BASE], cases.N_REF))
    good = cases.ordinary(2000)
    for bad in (bytes(20), struct.pack("<iii", 16, 0, 5) + bytes(8), struct.pack("<iiiBBHHH", 32, 0, 5, 255, 0, 0, 60000, 0) + bytes(16)):
        for mode in (0, 2):
            assert run(cases.make_case(good + [bad]), mode)[0] == 10 + 1      # BWAHIP_EINVAL
    assert run(cases.make_case(good + [rec(0, 1 << 29, [(1, S), (5, D)])]), 2)[0] == 10 + 5   # BWAHIP_ECAPACITY


def test_reader_selects_the_bins_of_reg2bins():
    """The reader picks a bin by its level's range instead of listing the up to 37 449 bins of a region: the two must agree."""
    rng = random.Random(1)
    for _ in range(300):
        beg = rng.randrange(0, 1 << 29)
        end = min(1 << 29, beg + rng.choice((1, 2, 100, 16384, 20000, 1 << 20, 1 << 27)))
        want = set(bai_ref.reg2bins(beg, end))
        idx = dict(refs=[dict(bins={b: [(1, 2)] for b in rng.sample(range(37449), 200) + sorted(want)[:40]}, lin=[0] * 32768, meta=None)], n_no_coor=0)
        got = bai_ref.query(idx, 0, beg, end)
        assert len(got) == len(want & set(idx["refs"][0]["bins"]))
