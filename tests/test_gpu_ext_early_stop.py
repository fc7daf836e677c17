"""GPU tests of the early stop of ksw_extend2 ("ksw_extend2: rows that cannot matter"): every device form ends its row loop once
no later row can change score, qle, tle, gtle, gscore or max_off.  Through the known-answer entry (dp_kat.device_extend: the plain form
beside the windowed driver, at 3 and 11 columns per lane, both strides) with liboracle.so as the judge, bit-exact; the entry's path mask
says whether the rule ended the loop (KAT_EXT_STOPPED).  Families: calls in which rows past the query's end decide gtle / gscore; the
benchmark's flank shape (the rule must be alive); calls that must never stop; the forms wave_extend_fit chooses between; and the golden
SAM with the knob at 0 (the loops of the parent)."""
import gzip
import os
import numpy as np
import pytest
import common
import dp_kat
from dp_kat import Case, scmat, rand_query
from common import bw

pytestmark = pytest.mark.gpu
CPLS = [3, 11]
GAP61 = (6, 1, 6, 1)
WINDOWED = bw.KAT_EXT_ROWS1 | bw.KAT_EXT_ROWS2 | bw.KAT_EXT_ROWS3 | bw.KAT_EXT_ROWS4
PLAIN = bw.KAT_EXT_SHORT | bw.KAT_EXT_WIDE | bw.KAT_EXT_BEYOND16


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def ora():
    return dp_kat.Oracle()


def _diff(got, want, cases, what):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{what}: {len(bad)} of {len(want)} differ; first {bad[0]}: {cases[bad[0]]}\n got  {got[bad[0]]}\n want {want[bad[0]]}"


def _run(ctx, ora, cases, cpl, what):
    """device == oracle on either stride; the path masks (forward, reversed)"""
    got, masks = dp_kat.device_extend(ctx, cases, cpl, 0)
    _diff(got, [ora.extend(c) for c in cases], cases, f"{what} cpl={cpl} forward")
    got_r, masks_r = dp_kat.device_extend(ctx, cases, cpl, 1)
    _diff(got_r, [ora.extend(c.reversed()) for c in cases], cases, f"{what} cpl={cpl} reversed")
    return masks, masks_r


def _stopped(masks):
    return (masks & bw.KAT_EXT_STOPPED) != 0


def _run_twins(ctx, ora, cases, cpl, what):
    """The cases and their reversed twins, each on either stride (all four equal the oracle).  Returns the masks of the cases read forward and
    of the twins read backwards: the same alignment problem through stride +1 and through stride -1, as the right and the left extension run it."""
    n = len(cases)
    masks, masks_r = _run(ctx, ora, cases + [c.reversed() for c in cases], cpl, what)
    return masks[:n], masks_r[n:]


# ---------------------------------------------------------------------------------------------------------------- later rows matter
def later_rows_cases(cpl):
    """One deletion (1 to 40 bases the query lacks) inside the last 30 query bases, high h0, 60 target bases more than the query has: the
    path through the gap reaches the query's end in a row past qlen, so gtle / gscore are decided there.  And tandem repeats (period 1 to
    6) against a longer repeat of the same unit: every later row ties or nearly ties the end-to-end score."""
    rng = np.random.default_rng(7100 + cpl)
    maxq = min(64 * cpl - 1, 250)
    out = []
    for _ in range(700):
        qlen = int(rng.integers(20, maxq + 1))
        q = rand_query(rng, qlen)
        p, g = qlen - int(rng.integers(1, 31)), int(rng.integers(1, 41))
        t = np.concatenate([q[:p], rand_query(rng, g), q[p:]])
        t = np.concatenate([t, rand_query(rng, qlen + 60)])[:qlen + 60]
        out.append(Case("ext", q, t, 100, GAP61, scmat(1, 4), int(rng.integers(100, 400)), int(rng.choice([0, 100])), int(rng.choice([0, 5])), fam="late deletion"))
    for _ in range(300):
        qlen, per = int(rng.integers(20, maxq + 1)), int(rng.integers(1, 7))
        unit = rand_query(rng, per)
        tlen = qlen + int(rng.integers(10, 120))
        q, t = np.resize(unit, qlen).copy(), np.resize(unit, tlen).copy()
        for s in (q, t):
            hit = rng.random(len(s)) < rng.choice([0.0, 0.01])
            s[hit] = rng.integers(0, 4, int(hit.sum()))
        out.append(Case("ext", q, t, int(rng.choice([20, 100])), dp_kat.GAPS[rng.integers(0, 2)], scmat(*dp_kat.MATRICES[rng.integers(0, 2)]),
                        int(rng.integers(20, 300)), int(rng.choice([0, 100])), int(rng.choice([0, 5])), fam="tandem"))
    return out


def later_rows_floors(ora, cases):
    """(calls whose gtle lies past qlen, calls whose gtle differs from the answer on the target cut to qlen rows) by the oracle alone"""
    want = [ora.extend(c) for c in cases]
    cut = [ora.extend(Case("ext", c.q, c.t[:c.qlen], c.w, c.gaps, c.mat, c.h0, c.zdrop, c.bonus)) for c in cases]
    return sum(a[3] > c.qlen for a, c in zip(want, cases)), sum(a[3] != b[3] for a, b in zip(want, cut))


@pytest.mark.parametrize("cpl", CPLS)
def test_later_rows_matter(ctx, ora, cpl):
    cases = later_rows_cases(cpl)
    past, moved = later_rows_floors(ora, cases)
    masks, masks_r = _run(ctx, ora, cases, cpl, "later rows")
    print(f"\nlater rows cpl {cpl}: {len(cases)} calls, gtle > qlen in {past}, gtle moved by rows past qlen in {moved}, stopped {int(_stopped(masks).sum())} + {int(_stopped(masks_r).sum())}")
    assert past >= 50 and moved >= 20                                     # (not vacuous: judged by the oracle alone)


# ---------------------------------------------------------------------------------------------------------------- benchmark shape
def bench_case(rng, qlen, h0=None):
    """A flank of the benchmark's reads: 1/-4, 6/1, w 100, z-drop 100, bonus 5, tlen = qlen + cal_max_gap(qlen), 1 % substitutions, the
    first base a mismatch (the seed ended there)."""
    q = rand_query(rng, qlen)
    max_gap = min(max(qlen - 6 + 1, 1), 200)
    t = np.concatenate([q, rand_query(rng, max_gap)])
    sub = rng.random(qlen) < 0.01
    sub[0] = True
    t[:qlen][sub] = (t[:qlen][sub] + 1 + rng.integers(0, 3, int(sub.sum()))) & 3
    return Case("ext", q, t, 100, GAP61, scmat(1, 4), int(rng.integers(19, 148)) if h0 is None else h0, 100, 5, fam="bench")


@pytest.mark.parametrize("cpl", CPLS)
def test_benchmark_shape_stops(ctx, ora, cpl):
    rng = np.random.default_rng(7200 + cpl)
    cases = [bench_case(rng, int(rng.integers(3, 103))) for _ in range(1500)]
    masks, masks_r = _run_twins(ctx, ora, cases, cpl, "benchmark shape")
    n, n_r = int(_stopped(masks).sum()), int(_stopped(masks_r).sum())
    print(f"\nbenchmark shape cpl {cpl}: {len(cases)} calls, stopped {n} on stride +1, {n_r} on stride -1")
    assert n >= len(cases) // 2 and n_r >= len(cases) // 2                # (the CPU model: 98 to 100 %; the floor keeps the rule from being dead)


# ---------------------------------------------------------------------------------------------------------------- must not stop
def no_gscore_cases(cpl):
    """Candidates for gscore = -1: a target shorter than the query under a band that cannot reach the last column from it, and a band too
    narrow to get there at all."""
    rng = np.random.default_rng(7300 + cpl)
    maxq = min(64 * cpl - 1, 400)
    out = []
    for _ in range(400):
        qlen = int(rng.integers(30, maxq + 1))
        w = int(rng.choice([0, 1, 2, 5, 20]))
        tlen = max(1, qlen - w - 2 - int(rng.integers(0, 20)))
        q = rand_query(rng, qlen)
        out.append(Case("ext", q, dp_kat.mutate(rng, q, tlen, 0.02), w, GAP61, scmat(1, 4), int(rng.integers(20, 300)), int(rng.choice([0, 100])), 5, fam="tlen < qlen"))
    for _ in range(400):
        qlen = int(rng.integers(30, maxq + 1))
        q = rand_query(rng, qlen)
        g = int(rng.integers(8, 25))                                      # an insertion the band of 5 cannot follow: the row maximum dies out before the last column
        p = int(rng.integers(5, qlen - 20))
        t = np.concatenate([q[:p], q[p + g:], rand_query(rng, 80)])
        out.append(Case("ext", q, t, 5, GAP61, scmat(1, 4), int(rng.integers(10, 40)), 100, 5, fam="narrow band"))
    return out


@pytest.mark.parametrize("cpl", CPLS)
def test_no_gscore_never_stops(ctx, ora, cpl):
    cand = no_gscore_cases(cpl)
    cases = [c for c in cand if ora.extend(c)[4] == -1]
    assert len(cases) >= 300 and sum(c.fam == "narrow band" for c in cases) >= 50 and sum(c.fam == "tlen < qlen" for c in cases) >= 50
    masks, masks_r = _run(ctx, ora, cases, cpl, "gscore -1")
    rev = np.array([ora.extend(c.reversed())[4] == -1 for c in cases])
    assert not _stopped(masks).any()
    assert not _stopped(masks_r)[rev].any()


@pytest.mark.parametrize("cpl", CPLS)
def test_knob_off(ctx, ora, cpl):
    """ext_early_stop = 0: the parent's loops -- no call reports a stop, the results still equal the oracle's."""
    rng = np.random.default_rng(7400 + cpl)
    cases = later_rows_cases(cpl)[::4] + [bench_case(rng, int(rng.integers(3, 103))) for _ in range(300)]
    ctx.tune(ext_early_stop=0)
    try:
        masks, masks_r = _run(ctx, ora, cases, cpl, "knob 0")
    finally:
        ctx.tune(ext_early_stop=1)
    assert not _stopped(masks).any() and not _stopped(masks_r).any()
    masks, _ = _run(ctx, ora, cases, cpl, "knob back at 1")
    assert _stopped(masks).sum() >= 150                                   # (and it is the knob that made the difference)


# ---------------------------------------------------------------------------------------------------------------- the other forms
def form_cases(cpl):
    """name -> (cases, path bits: every call must report one of them, and no plain form where they are the windowed ones).  The flank lengths at which wave_extend_fit changes form; the two sides of what 16
    bits hold (50/-60: the windowed form at 32759, the plain one at 32760); a band that can outgrow the widest window (plain form)."""
    rng = np.random.default_rng(7500 + cpl)
    maxq = 64 * cpl - 1
    fam = {}
    for qlen in (63, 64, 65, 191, 192):
        if qlen <= maxq:
            fam[f"flank {qlen}"] = ([bench_case(rng, qlen, h0=int(rng.integers(19, 148))) for _ in range(12)], bw.KAT_EXT_SHORT if qlen < 64 else WINDOWED)
    for k, bit in ((32759, WINDOWED), (32760, bw.KAT_EXT_BEYOND16)):
        cs = []
        for _ in range(12):
            qlen = int(rng.integers(64, min(maxq, 600) + 1))
            q = rand_query(rng, qlen)
            cs.append(Case("ext", q, np.concatenate([dp_kat.mutate(rng, q, qlen, 0.01, max_gap=3), rand_query(rng, 120)]), 100, GAP61, scmat(50, 60), k - 50 * qlen,
                           int(rng.choice([0, 1000])), 5, fam=f"16bit {k}"))
        fam[f"h0 + qlen * mx = {k}"] = (cs, bit)
    if cpl == 11:                                                         # (2w + 2 beyond 255 columns needs a flank of 256 bases and more)
        q = rand_query(np.random.default_rng(300), 300)
        t = np.concatenate([q[:60], q[160:], rand_query(np.random.default_rng(301), 160)])   # as test_gpu_dp_kat's BAND_BEYOND_WINDOW cases, with rows past the query's end
        fam["band beyond window"] = ([Case("ext", q, t, 200, GAP61, scmat(1, 4), 400, 0, 0, fam="skip100_of_300")], bw.KAT_EXT_WIDE)
    return fam


@pytest.mark.parametrize("cpl", CPLS)
def test_other_forms(ctx, ora, cpl):
    for name, (cases, bit) in form_cases(cpl).items():
        masks, masks_r = _run_twins(ctx, ora, cases, cpl, name)
        both = np.concatenate([masks, masks_r])
        print(f"\n{name} cpl {cpl}: {len(cases)} calls, stopped {int(_stopped(both).sum())} of {len(both)}")
        assert ((both & bit) != 0).all() and (bit != WINDOWED or ((both & PLAIN) == 0).all()), (name, [int(m) for m in both])
        assert _stopped(masks).any() and _stopped(masks_r).any(), name   # the rule is alive in this form, on either stride


# ---------------------------------------------------------------------------------------------------------------- SAM with the knob at 0
def _first_diff(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return f"SAM differs at line {i} of {len(w)}:\n got  {a[:300]}\n want {b[:300]}"
    return f"SAM line counts differ: {len(g)} vs {len(w)}"


def test_golden_sam_with_knob_off(built, tmp_path):
    """The reference-made SAM of tests/golden (SE -a and PE) with ext_early_stop = 0; test_gpu_sam.py covers the default."""
    G = common.GOLDEN
    fa = str(tmp_path / "g60k.fa")
    open(fa, "wb").write(gzip.open(os.path.join(G, "g60k.fa.gz")).read())
    bw.make_index(fa, str(tmp_path / "g60k"))
    open(str(tmp_path / "g60k.alt"), "wb").write(open(os.path.join(G, "g60k.alt"), "rb").read())
    for n in ("se.fq", "pe_1.fq", "pe_2.fq"):
        open(str(tmp_path / n), "wb").write(gzip.open(os.path.join(G, n + ".gz")).read())
    with bw.Context(str(tmp_path / "g60k")) as c:
        c.tune(ext_early_stop=0)
        names, seqs, quals = bw.read_fastq(str(tmp_path / "se.fq"))
        opt = bw.default_opt()
        opt.n_threads = 4
        opt.flag |= 0x8                                                   # -a
        got = b"".join(c.process_seqs(names, seqs, quals, opt))
        want = gzip.open(os.path.join(G, "se_all.sam.gz")).read()
        assert got == want, _first_diff(got, want)
        n1, s1, q1 = bw.read_fastq(str(tmp_path / "pe_1.fq"))
        n2, s2, q2 = bw.read_fastq(str(tmp_path / "pe_2.fq"))
        opt = bw.default_opt()
        opt.n_threads = 4
        opt.flag |= 0x2
        got = b"".join(c.process_seqs([x for p in zip(n1, n2) for x in p], [x for p in zip(s1, s2) for x in p],
                                      [x for p in zip(q1, q2) for x in p], opt))
        want = gzip.open(os.path.join(G, "pe.sam.gz")).read()
        assert got == want, _first_diff(got, want)
