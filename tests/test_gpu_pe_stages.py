"""Paired-end path on the GPU (csrc/k_pair.hip) against the CPU path, stage by stage, on the libraries of tests/pe_cases.py: every
orientation, rescue windows of every class, mates of ragged length, contig ends.  Per library: what it is for is asserted on the oracle's
records first; then insert-size statistics (PESTAT), the lists after mate rescue (REGS_PE), the pairing decisions (PAIR) and the SAM text
must equal the oracle's bit for bit; then the kernels' own counters must show that the path the library is for really ran."""
import numpy as np
import pytest
import bam_ref
import common
import pe_cases as pc
from common import bw

pytestmark = pytest.mark.gpu

PE_STAGES = [bw.STAGE_PESTAT, bw.STAGE_REGS, bw.STAGE_REGS_PE, bw.STAGE_PAIR]


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib(small_index, tmp_path_factory):
    """lib(name, flags) -> the library's reads and the oracle's records and SAM for them under `flags`; made once per module."""
    genome = pc.load_genome(small_index["fa"])
    d = tmp_path_factory.mktemp("pelib")
    reads, cache = {}, {}

    def get(name, flags=()):
        if name not in reads:
            fq1, fq2, r1, r2, _ = pc.write_library(genome, name, d)
            seqs = [x for p in zip(r1, r2) for x in p]
            codes, off = bw.pack_reads(seqs)
            reads[name] = dict(fq1=fq1, fq2=fq2, seqs=seqs, names=[b"p%d" % (i >> 1) for i in range(len(seqs))], quals=[b"I" * len(s) for s in seqs],
                               codes=codes, off=off, lens=[len(s) for s in seqs])
        key = (name, tuple(flags))
        if key not in cache:
            L = dict(reads[name])
            L["ps"], L["reads"] = pc.oracle_pe_stages(small_index["prefix"], L["fq1"], L["fq2"], str(d / "o.bin"), ["-t", "8", *flags])
            L["sam"] = pc.oracle_sam(small_index["prefix"], L["fq1"], L["fq2"], ["-t", "8", *flags])
            cache[key] = L
        return cache[key]
    return get


def _mask_regs_pe(rec):
    """Two words of a region that nothing reads after this stage:
    `secondary`: mem_matesw sets it to -1 on the regions it adds (bwamem_pair.c:188) and leaves the others as they were; the next thing
    that happens to the list, mem_mark_primary_se, overwrites it on every region before anything reads it (bwamem.c:534:
    a[i].secondary = a[i].secondary_all = -1).  The device keeps no such field before its mark-primary kernel.
    `n_comp`: its only reader in the reference is mem_sort_dedup_patch itself (bwamem.c:468), after the same call has set it to 1 on
    every region (bwamem.c:449, skipped for a list of one by the return at :448); what the last call of mem_matesw leaves behind is
    read by nothing.  The device's incr_insert, which stands in for such a call, does not reproduce the leftover (1 on a region that
    is alone in its list, 0 on regions of a list it found already clean)."""
    a = rec.copy()
    a[1 + 13::19] = 0
    a[1 + 16::19] = 0
    return a


def _opt(flags=()):
    opt, pes0 = common.opt_from_cli(list(flags))
    opt.n_threads = 8
    opt.flag |= 0x2
    return opt, pes0


def _assert_stages(ctx, L, what, flags=(), pes0=None):
    """PESTAT, REGS_PE, PAIR of the GPU path == the oracle's; returns the device's per-read records."""
    opt, pes0_cli = _opt(flags)
    ps, got = pc.split_pe(ctx.run_pe_stages(L["codes"], L["off"], PE_STAGES, opt, pes0=pes0 if pes0 is not None else pes0_cli))
    assert np.array_equal(ps, L["ps"]), f"{what}: PESTAT\n got  {pc.pestat_dicts(ps)}\n want {pc.pestat_dicts(L['ps'])}"
    want = L["reads"]
    common.assert_stage_equal(got, want, bw.STAGE_REGS, f"{what}: regions before rescue")
    gm = [{bw.STAGE_REGS_PE: _mask_regs_pe(g[bw.STAGE_REGS_PE])} for g in got]
    wm = [{bw.STAGE_REGS_PE: _mask_regs_pe(w[bw.STAGE_REGS_PE])} for w in want]
    common.assert_stage_equal(gm, wm, bw.STAGE_REGS_PE, f"{what}: REGS_PE")
    common.assert_stage_equal(got, want, bw.STAGE_PAIR, f"{what}: PAIR")
    return got


def _sam(ctx, L, flags=(), pes0=None, n_processed=0, lo=0, hi=None):
    opt, pes0_cli = _opt(flags)
    hi = len(L["seqs"]) if hi is None else hi
    return b"".join(ctx.process_seqs(L["names"][lo:hi], L["seqs"][lo:hi], L["quals"][lo:hi], opt, n_processed=n_processed, pes0=pes0 if pes0 is not None else pes0_cli))


# per library: the counters of bwahip_last_pe_paths that must be above zero
PATHS = {
    "rf": ["try_rf"], "ff_rr": ["try_ff", "try_rr"], "mixed4": ["try_ff", "try_fr", "try_rf", "try_rr"],
    "minor_dir": ["try_ff", "try_fr"],
    "mid_insert": ["inline_lds"], "wide_insert": ["inline_slab"],
    "ragged": ["ahead_byte", "ahead_word", "both_kernels"],
    "edges": ["off_contig"],
}


@pytest.mark.parametrize("name,flags", [(n, ()) for n in pc.LIBRARIES] + [("ragged", ("-A", "2"))])
def test_library_matches_oracle_stage_by_stage(ctx, lib, name, flags):
    L = lib(name, flags)
    pc.preconditions(name, L["ps"], L["reads"], L["lens"])
    what = f"{name} {' '.join(flags)}".strip()
    _assert_stages(ctx, L, what, flags)
    paths = ctx.last_pe_paths()
    print(what, paths)
    assert _sam(ctx, L, flags) == L["sam"], f"{what}: SAM"
    for k in PATHS[name]:
        assert paths[k] > 0, f"{what}: path {k} did not run: {paths}"
    live = [not p["failed"] for p in pc.pestat_dicts(L["ps"])]
    for d, k in enumerate(("try_ff", "try_fr", "try_rf", "try_rr")):
        assert live[d] or paths[k] == 0, f"{what}: rescue attempted in a failed orientation: {paths}"
    if name == "mid_insert":                                    # 150-base mates: the byte kernel, every window beyond the ahead kernels' 1024 bases
        assert paths["inline_slab"] == 0 and paths["ahead_word"] == 0
    assert paths["incr_insert"] + paths["general_dedup"] > 0


REPEAT_FLAGS = ("-I", "330,40")                                  # given insert sizes: pairs inside a repeat family give mem_pestat nothing to learn from


@pytest.fixture(scope="module")
def repeat_family(built, tmp_path_factory):
    """40 FR pairs from a 400-base unit with 1000 copies (2 % diverged, one every 700 bases at most) in a 1 Mbp genome of its own -- the recipe
    of test_gpu_sam.py::test_reads_inside_a_large_repeat_family, at the smallest size (found with bwa_oracle alone) at which the oracle's lists
    show both kinds of pair the rescue kernels tell apart: every third fragment reaches the unique flank, the others lie wholly inside the unit."""
    d = tmp_path_factory.mktemp("repfam")
    rng = np.random.default_rng(2)
    n_copies, length = 1000, 1000000
    g = rng.integers(0, 4, length, dtype=np.uint8)
    unit = rng.integers(0, 4, 400, dtype=np.uint8)
    starts = np.sort(rng.choice(np.arange(1000, length - 1400, 700), n_copies, replace=False))
    for s in starts:
        c = unit.copy()
        m = rng.random(400) < 0.02
        c[m] = (c[m] + rng.integers(1, 4, int(m.sum()))) % 4
        g[s:s + 400] = c
    txt = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[g])
    fa, prefix = str(d / "rep.fa"), str(d / "rep")
    with open(fa, "wb") as f:
        f.write(b">rep\n")
        for i in range(0, length, 60):
            f.write(txt[i:i + 60] + b"\n")
    bw.make_index(fa, prefix)
    r1, r2 = [], []
    for i in range(40):
        s = int(starts[rng.integers(0, n_copies)])
        if i % 3 == 0:                                              # fragment inside the repeat unit and its unique flank: rescue has something to add
            a = s + int(rng.integers(0, 200)); frag = txt[a:a + 420]
        else:                                                       # fragment wholly inside the unit: every copy matches
            a = s + int(rng.integers(0, 60)); frag = txt[a:a + 330]
        r1.append(frag[:150]); r2.append(pc.rc(frag[-150:]))
    fq1, fq2 = str(d / "h_1.fq"), str(d / "h_2.fq")
    pc.write_fastq(fq1, r1); pc.write_fastq(fq2, r2)
    seqs = [x for p in zip(r1, r2) for x in p]
    codes, off = bw.pack_reads(seqs)
    L = dict(prefix=prefix, seqs=seqs, names=[b"p%d" % (i >> 1) for i in range(len(seqs))], quals=[b"I" * len(s) for s in seqs], codes=codes, off=off)
    L["ps"], L["reads"] = pc.oracle_pe_stages(prefix, fq1, fq2, str(d / "o.bin"), ["-t", "8", *REPEAT_FLAGS])
    L["sam"] = pc.oracle_sam(prefix, fq1, fq2, ["-t", "8", *REPEAT_FLAGS])
    return L


def test_repeat_family_lists_with_and_without_incr_insert(repeat_family):
    """Lists beyond the 224 regions held in LDS and lists of dozens of regions, most of them changed by rescue: with the knob incr_insert at 1
    (as shipped) and at 0 (every orientation ends in the full sort-and-dedup) statistics, lists, pairing and SAM are the oracle's, and the
    counters show that the incremental path, the general path, the global-memory instantiation of k_matesw and the wavefront copy all ran."""
    L = repeat_family
    n_pe = [int(r[bw.STAGE_REGS_PE][0]) for r in L["reads"]]
    assert max(n_pe) > 224, "no end with a list beyond the LDS list"
    assert any(33 <= n_pe[i] + n_pe[i + 1] <= 224 for i in range(0, len(n_pe), 2)), "no pair for the wavefront copy with its lists in LDS"
    assert len(pc.rescued_reads(L["reads"])) >= 8, "rescue changed too few lists"
    assert any(int(r[bw.STAGE_REGS_PE][0]) - int(r[bw.STAGE_REGS][0]) >= 20 for r in L["reads"]), "no list that rescue grew by many regions"
    paths = {}
    with bw.Context(L["prefix"]) as c:
        try:
            for knob in (1, 0):
                c.tune(incr_insert=knob)
                _assert_stages(c, L, f"repeat family, incr_insert {knob}", REPEAT_FLAGS)
                paths[knob] = c.last_pe_paths()
                print("incr_insert", knob, paths[knob])
                assert _sam(c, L, REPEAT_FLAGS) == L["sam"], f"repeat family, incr_insert {knob}: SAM"
        finally:
            c.tune(incr_insert=1)
    p1, p0 = paths[1], paths[0]
    assert p1["incr_insert"] > 0 and p1["general_dedup"] > 0 and p1["big_pairs"] > 0 and p1["copy_big_pairs"] > 0, p1
    assert p0["incr_insert"] == 0 and p0["general_dedup"] > p1["general_dedup"], (p0, p1)
    assert p0["big_pairs"] == p1["big_pairs"] and p0["copy_big_pairs"] == p1["copy_big_pairs"]


def test_mixed4_with_host_pairing_gives_the_same_sam(ctx, lib):
    L = lib("mixed4")
    try:
        ctx.tune(gpu_pair=0)
        host = _sam(ctx, L)
    finally:
        ctx.tune(gpu_pair=1)
    assert host == L["sam"]


def test_mixed4_in_two_batches_with_carried_statistics(ctx, lib):
    """The batch cut in two, n_processed carried over, pes0 = the whole batch's statistics with all four orientations live (which -I
    cannot express): lists, decisions and SAM of the two halves together are the single batch's."""
    L = lib("mixed4")
    assert not any(p["failed"] for p in pc.pestat_dicts(L["ps"]))
    pes0 = pc.pes0_from(L["ps"])
    n = len(L["seqs"])
    cut = (n // 2 + 37) & ~1
    got, sam = [], b""
    for lo, hi in ((0, cut), (cut, n)):
        codes, off = L["codes"][L["off"][lo]:L["off"][hi]], L["off"][lo:hi + 1] - L["off"][lo]
        ps, part = pc.split_pe(ctx.run_pe_stages(codes, off, PE_STAGES, _opt()[0], n_processed=lo, pes0=pes0))
        assert np.array_equal(ps, L["ps"])
        got += part
        sam += _sam(ctx, L, pes0=pes0, n_processed=lo, lo=lo, hi=hi)
    want = L["reads"]
    gm = [{bw.STAGE_REGS_PE: _mask_regs_pe(g[bw.STAGE_REGS_PE])} for g in got]
    wm = [{bw.STAGE_REGS_PE: _mask_regs_pe(w[bw.STAGE_REGS_PE])} for w in want]
    common.assert_stage_equal(gm, wm, bw.STAGE_REGS_PE, "two batches: REGS_PE")
    common.assert_stage_equal(got, want, bw.STAGE_PAIR, "two batches: PAIR")
    assert sam == L["sam"]


@pytest.mark.parametrize("flags", [("-S",), ("-P",), ("-m", "5"), ("-U", "5")])
def test_mixed4_options_at_stage_level(ctx, lib, flags):
    L = lib("mixed4", flags)
    got = _assert_stages(ctx, L, f"mixed4 {' '.join(flags)}", flags)
    if flags == ("-S",):                                        # no rescue: the lists are the single-end ones
        assert all(np.array_equal(g[bw.STAGE_REGS_PE], g[bw.STAGE_REGS]) for g in got)
        assert ctx.last_pe_paths()["try_fr"] == 0
    if flags == ("-P",):
        assert all(int(g[bw.STAGE_PAIR][0]) == 0 and not g[bw.STAGE_PAIR][5:].any() for g in got)
    if flags == ("-m", "5") or flags == ("-U", "5"):             # the option must have changed something, or the case shows nothing
        base = lib("mixed4")["reads"]
        assert any(not np.array_equal(a[bw.STAGE_REGS_PE], b[bw.STAGE_REGS_PE]) or not np.array_equal(a[bw.STAGE_PAIR], b[bw.STAGE_PAIR]) for a, b in zip(L["reads"], base))
    assert _sam(ctx, L, flags) == L["sam"]


@pytest.mark.parametrize("name", ["rf", "wide_insert"])
def test_bam_records_of_other_orientations_and_long_templates(ctx, lib, small_index, name):
    """Flag bits of mates on the same strand or facing outwards and template lengths of thousands of bases, through the BAM encoder."""
    L = lib(name)
    opt, _ = _opt()
    got = ctx.process_seqs_bam(L["names"], L["seqs"], L["quals"], opt)
    contigs = bam_ref.contig_names_of(small_index["prefix"])
    want = bam_ref.sam_to_bam_records(L["sam"], contigs)
    if got != want:
        g, w = bam_ref.split_records(got), bam_ref.split_records(want)
        bad = [i for i, (a, b) in enumerate(zip(g, w)) if a != b]
        raise AssertionError(f"{name}: {len(g)} records vs {len(w)}; first differing {bad[:1]}: got {bam_ref.bam_record_to_sam(g[bad[0]], contigs) if bad else None}")
