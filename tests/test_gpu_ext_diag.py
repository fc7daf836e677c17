"""GPU tests of the diagonal rule of ksw_extend2 ("ksw_extend2: flanks the diagonal answers"): the extension kernels answer a flank
of ACGT bases with at most K mismatches from the main diagonal, without a DP row.  Through the known-answer entry that makes the call as the
product does (bwahip_kat_ksw_extend2_diag), at 3 and 11 columns per lane and on either stride: the six results equal liboracle.so's, and the
entry's DIAG bit equals the predicate of tests/ext_diag_model.c exactly -- the calls that qualify and the near misses that must fall through
to the DP forms.  With ext_diag = 0 no call reports DIAG.  Then the golden SAM with the knob at 0 and at 1, and the work counters."""
import gzip
import os
import numpy as np
import pytest
import common
import dp_kat
from dp_kat import Case, scmat, rand_query
from common import bw
from test_ext_diag_model import build_model, rule

pytestmark = pytest.mark.gpu
CPLS = [3, 11]
GAP61 = (6, 1, 6, 1)
LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 191, 192]


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def ora():
    return dp_kat.Oracle()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return build_model(tmp_path_factory.mktemp("edg_gpu"))


def _sub(rng, t, p):
    t[p] = (t[p] + 1 + rng.integers(0, 3)) & 3


def flank(rng, qlen, nsub, h0=None, ab=(1, 4), gaps=GAP61, zdrop=100, extra=None, fam="flank", at=None):
    """A flank of qlen bases with nsub substitutions (at the positions `at`, else anywhere) against a target of qlen + extra bases."""
    q = rand_query(rng, qlen)
    extra = int(rng.integers(0, 40)) if extra is None else extra
    t = np.concatenate([q, rand_query(rng, extra)])
    for p in (at if at is not None else rng.choice(qlen, size=min(nsub, qlen), replace=False)):
        _sub(rng, t, int(p))
    return Case("ext", q, t, int(rng.choice([0, 5, 100])), gaps, scmat(*ab), int(rng.integers(19, 148)) if h0 is None else h0, zdrop, 5, fam=fam)


def cases_for(cpl):
    """The calls that qualify and the near misses, at every length the test is asked for that fits cpl columns per lane."""
    rng = np.random.default_rng(8100 + cpl)
    out = []
    for qlen in [n for n in LENGTHS if n + 1 <= 64 * cpl]:
        for _ in range(6):
            out.append(flank(rng, qlen, 0, fam="exact"))
            out.append(flank(rng, qlen, 1, fam="one mismatch"))
            out.append(flank(rng, qlen, 1, at=[0], fam="mismatch first"))
            out.append(flank(rng, qlen, 1, at=[qlen - 1], fam="mismatch last"))
            if qlen > 1:
                out.append(flank(rng, qlen, 2, fam="K + 1 mismatches"))
            out.append(flank(rng, qlen, 2, ab=(1, 1), gaps=(16, 1, 16, 1), fam="K = 8, two mismatches"))
            out.append(flank(rng, qlen, 1, extra=0, fam="tlen = qlen"))
            if qlen > 1:
                c = flank(rng, qlen, 0, fam="short target")
                out.append(Case("ext", c.q, c.t[:qlen - 1], c.w, c.gaps, c.mat, c.h0, c.zdrop, c.bonus, fam=c.fam))
            out.append(flank(rng, qlen, 1, at=[int(rng.integers(0, min(qlen, 2)))], h0=int(rng.integers(1, 3)), fam="dying diagonal"))   # h0 + 1 - 4 < 1 at the latest
            out.append(flank(rng, qlen, 1, zdrop=int(rng.integers(1, 4)), fam="small z-drop"))
            out.append(flank(rng, qlen, 1, gaps=(1, 1, 1, 1), fam="cheap gaps"))
            out.append(flank(rng, qlen, 1, ab=(2, 3), gaps=(4, 2, 7, 1), fam="K = 1 by the deletion"))
            c = flank(rng, qlen, int(rng.integers(0, 2)), fam="N")
            s = c.q if rng.random() < 0.5 else c.t
            s[int(rng.integers(0, qlen))] = 4
            out.append(c)
    maxq = min(64 * cpl - 1, 250)
    for _ in range(120):                                                  # tandem repeats (period 1 to 6) with one substitution, against a longer repeat of the unit
        qlen, per = int(rng.integers(2, maxq + 1)), int(rng.integers(1, 7))
        unit = rand_query(rng, per)
        q, t = np.resize(unit, qlen).copy(), np.resize(unit, qlen + int(rng.integers(0, 120))).copy()
        _sub(rng, t, int(rng.integers(0, qlen)))
        out.append(Case("ext", q, t, int(rng.choice([20, 100])), GAP61, scmat(1, 4), int(rng.integers(20, 300)), int(rng.choice([0, 100])), int(rng.choice([0, 5])), fam="tandem"))
    return out


def device(ctx, cases, cpl, reverse):
    params = [[c.qlen, c.tlen, c.w, c.h0, c.zdrop, c.bonus, *c.gaps, reverse, cpl] for c in cases]
    out = ctx.kat_ksw_extend2(params, *dp_kat.pack(cases), diag=True)
    return [[int(x) for x in out[i, :6]] for i in range(len(cases))], out[:, 6].copy()


def _check(ctx, ora, model, cases, cpl, knob):
    """results == oracle on either stride; the DIAG bit == the model's predicate (knob 1) or never set (knob 0).  Returns the calls answered."""
    answered = 0
    for reverse in (0, 1):
        seen = [c.reversed() for c in cases] if reverse else cases        # what the call aligns: both sequences read backwards
        got, masks = device(ctx, cases, cpl, reverse)
        want = [ora.extend(c) for c in seen]
        bad = [i for i in range(len(cases)) if got[i] != want[i]]
        assert not bad, f"cpl {cpl} reverse {reverse} knob {knob}: {len(bad)} of {len(cases)} differ; first {seen[bad[0]]}\n got  {got[bad[0]]}\n want {want[bad[0]]}"
        holds = np.array([rule(model, c) is not None for c in seen])
        diag = (masks & bw.KAT_EXT_DIAG) != 0
        if knob:
            off = np.flatnonzero(diag != holds)
            assert not len(off), f"cpl {cpl} reverse {reverse}: DIAG bit differs from the predicate in {len(off)} calls; first {seen[off[0]]}: bit {diag[off[0]]}"
            assert (masks[diag] == bw.KAT_EXT_DIAG).all()                 # an answered call went through no DP form
            assert (masks[~diag] != 0).all()
        else:
            assert not diag.any()
        answered += int(diag.sum())
    return answered


@pytest.mark.parametrize("cpl", CPLS)
def test_diag_bit_is_the_predicate(ctx, ora, model, cpl):
    cases = cases_for(cpl)
    held = {}
    for c in cases:
        held.setdefault(c.fam, []).append(rule(model, c) is not None)
    print(f"\ncpl {cpl}: {len(cases)} calls; predicate by family: " + ", ".join(f"{k} {sum(v)}/{len(v)}" for k, v in held.items()))
    for fam in ("K + 1 mismatches", "short target", "dying diagonal", "small z-drop", "cheap gaps", "N"):
        assert not any(held[fam]), fam                                    # the near misses are near misses (by the model alone)
    for fam in ("exact", "mismatch first", "mismatch last", "K = 8, two mismatches", "tlen = qlen", "K = 1 by the deletion", "tandem"):
        assert sum(held[fam]) >= len(held[fam]) // 2, fam
    n = _check(ctx, ora, model, cases, cpl, 1)
    assert n >= len(cases) // 3                                           # (seven of the thirteen families qualify when read forward)


@pytest.mark.parametrize("cpl", CPLS)
def test_knob_off(ctx, ora, model, cpl):
    """ext_diag = 0: no call reports DIAG, the results are the same; back at 1 the rule answers again."""
    cases = cases_for(cpl)[::3]
    ctx.tune(ext_diag=0)
    try:
        assert _check(ctx, ora, model, cases, cpl, 0) == 0
    finally:
        ctx.tune(ext_diag=1)
    assert _check(ctx, ora, model, cases, cpl, 1) >= len(cases) // 3


# ---------------------------------------------------------------------------------------------------------------- SAM with the knob at 0 and at 1
def _first_diff(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return f"SAM differs at line {i} of {len(w)}:\n got  {a[:300]}\n want {b[:300]}"
    return f"SAM line counts differ: {len(g)} vs {len(w)}"


def test_golden_sam_with_knob_off_and_on(built, tmp_path):
    """The reference-made SAM of tests/golden (SE -a and PE) with ext_diag = 0 and = 1, byte for byte; the counters of the calls."""
    G = common.GOLDEN
    fa = str(tmp_path / "g60k.fa")
    open(fa, "wb").write(gzip.open(os.path.join(G, "g60k.fa.gz")).read())
    bw.make_index(fa, str(tmp_path / "g60k"))
    open(str(tmp_path / "g60k.alt"), "wb").write(open(os.path.join(G, "g60k.alt"), "rb").read())
    for n in ("se.fq", "pe_1.fq", "pe_2.fq"):
        open(str(tmp_path / n), "wb").write(gzip.open(os.path.join(G, n + ".gz")).read())
    names, seqs, quals = bw.read_fastq(str(tmp_path / "se.fq"))
    n1, s1, q1 = bw.read_fastq(str(tmp_path / "pe_1.fq"))
    n2, s2, q2 = bw.read_fastq(str(tmp_path / "pe_2.fq"))
    want_se = gzip.open(os.path.join(G, "se_all.sam.gz")).read()
    want_pe = gzip.open(os.path.join(G, "pe.sam.gz")).read()
    with bw.Context(str(tmp_path / "g60k")) as c:
        for knob in (0, 1):
            c.tune(ext_diag=knob)
            opt = bw.default_opt()
            opt.n_threads = 4
            opt.flag |= 0x8                                               # -a
            got = b"".join(c.process_seqs(names, seqs, quals, opt))
            assert got == want_se, f"ext_diag {knob}: " + _first_diff(got, want_se)
            cnt_se = c.counters()
            opt = bw.default_opt()
            opt.n_threads = 4
            opt.flag |= 0x2
            got = b"".join(c.process_seqs([x for p in zip(n1, n2) for x in p], [x for p in zip(s1, s2) for x in p],
                                          [x for p in zip(q1, q2) for x in p], opt))
            assert got == want_pe, f"ext_diag {knob}: " + _first_diff(got, want_pe)
            cnt_pe = c.counters()
            print(f"\next_diag {knob}: SE ext_calls {cnt_se['ext_calls']} ext_diag {cnt_se['ext_diag']}; PE ext_calls {cnt_pe['ext_calls']} ext_diag {cnt_pe['ext_diag']}")
            for cnt in (cnt_se, cnt_pe):
                assert cnt["ext_calls"] > 0
                if knob:
                    assert 0 < cnt["ext_diag"] <= cnt["ext_calls"]
                else:
                    assert cnt["ext_diag"] == 0
