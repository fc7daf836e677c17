"""Known answers for mem_sort_dedup_patch on the device: k_dedup_fast, k_dedup with the list in LDS (at most 32 regions) and in global memory
(wavefront sort or one-lane introsort, reach test evaluated 64 entries ahead, ballot compactions, mem_patch_reg with its global alignment)
and the slab form of k_extend_big, fed region lists directly through bwahip_kat_dedup -- the extension stage's own buffers and the
launches that follow k_extend -- against ora_kat_dedup (`bwa_oracle katdedup`), which tests/test_dedup_cases_cpu.py pins to the
reference's own mem_sort_dedup_patch, and against the reference-made tests/golden/kat_dedup.npz.  All 19 words of every region are
compared; the function is integers plus float and double comparisons in the reference's types: nothing is tolerated."""
import os

import numpy as np
import pytest

import common
import dedup_cases as dc
from common import bw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prefix(built, tmp_path_factory):
    return dc.make_index(str(tmp_path_factory.mktemp("dedup_g60k")))


@pytest.fixture(scope="module")
def ctx(prefix):
    c = bw.Context(prefix)
    yield c
    c.close()


@pytest.fixture(scope="module")
def judged(prefix, tmp_path_factory):
    """The oracle's answers, computed once per set and shared."""
    d, memo = str(tmp_path_factory.mktemp("dedup_ora")), {}

    def get(name):
        if name not in memo:
            memo[name] = dc.run_checker(common.ORACLE, name, prefix, d, "ora")
        return memo[name]
    return get


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(common.GOLDEN, "kat_dedup.npz"))


def tuned(ctx, knobs):
    for k, v in {**dict(rank_sort_min=2, ext_lds_window=1 << 30), **knobs}.items():
        ctx.tune(**{k: v})


def differing(got, want, cases):
    return [cases[i].name for i in range(len(want)) if not np.array_equal(got[i], want[i][0])]


def check(ctx, name, want, form, diag=True, cases=None):
    cases = dc.cases_of(name) if cases is None else cases
    got, dg, handed = ctx.kat_dedup(*dc.pack(cases)[:4], opt=dc.opt_of(name), heavy=dc.pack(cases)[4], form=form, diag=diag)
    bad = differing(got, want, cases)
    assert not bad, f"{name} form {form} diag {diag}: {len(bad)} of {len(cases)} lists differ from the oracle, first {bad[:5]}"
    return got, dg, handed


@pytest.mark.parametrize("name", list(dc.SETS))
def test_set_equals_oracle_golden_and_model(ctx, judged, gold, name):
    """Per set: the product's launches (k_dedup_fast first) and k_dedup alone both give the oracle's lists word for word and the reference's
    digests -- with the instantiations that write diagnostics and with the product's own --; every diag word is the one the model
    predicts: who finished the list, why k_dedup_fast refused it, which sort ran on one lane, and the judge's counts of alignments and
    merges; the reads handed over are the ones whose patch window exceeds the set's ext_lds_window."""
    s = dc.SETS[name]
    cases, want = dc.cases_of(name), judged(name)
    assert str(gold[f"{name}.inputs"]) == dc.input_digest(name), "the case generator drifted: regenerate tests/golden/kat_dedup.npz"
    tuned(ctx, s.knobs)
    try:
        for form in (bw.KAT_DEDUP_PRODUCT, bw.KAT_DEDUP_FULL):
            got, dg, handed = check(ctx, name, want, form)
            assert np.array_equal(dc.digests(got), gold[f"{name}.sha"]), f"{name} form {form}: differs from the reference's lists"
            pred = np.array([dc.predict(name, c, st, form) for c, (_, st) in zip(cases, want)], dtype=np.int32)
            bad = [(c.name, hex(int(a)), hex(int(b))) for c, a, b in zip(cases, dg, pred) if a != b]
            assert not bad, f"{name} form {form}: {len(bad)} diag words differ from the model (name, got, predicted), first {bad[:5]}"
            assert handed == int(np.count_nonzero(pred & bw.KAT_DEDUP_HANDED))
            got2, dg2, handed2 = check(ctx, name, want, form, diag=False)
            # (the product's instantiations write no diagnostics: a word is 0 unless the slab kernel, which always writes, took the read over)
            assert handed2 == handed and np.array_equal(dg2, np.where(pred & bw.KAT_DEDUP_HANDED, pred & ~(3 << bw.KAT_DEDUP_WHY_SHIFT), 0))
    finally:
        tuned(ctx, {})


@pytest.mark.parametrize("name", [n for n, s in dc.SETS.items() if s.slab])
def test_slab_form_equals_oracle(ctx, judged, name):
    """k_extend_big's dedup body -- list in global memory whatever its length, window in the slab -- on whole sets."""
    cases, want = dc.cases_of(name), judged(name)
    _, dg, handed = check(ctx, name, want, bw.KAT_DEDUP_SLAB)
    pred = np.array([dc.predict(name, c, st, bw.KAT_DEDUP_SLAB) for c, (_, st) in zip(cases, want)], dtype=np.int32)
    assert handed == 0 and np.array_equal(dg, pred)


def test_hand_over_reports_the_reads_above_the_window(ctx, judged):
    """ext_lds_window 150 and 400: the patch windows one base above hand the read over (short list and list of 42, which k_dedup has
    sorted in place by then) and the slab kernel answers from the original list; at and below the window k_dedup finishes the read."""
    for w in (150, 400):
        name = f"handover_{w}"
        cases, want = dc.cases_of(name), judged(name)
        tuned(ctx, dc.SETS[name].knobs)
        try:
            _, dg, handed = check(ctx, name, want, bw.KAT_DEDUP_PRODUCT)
        finally:
            tuned(ctx, {})
        over = [c.name for c, d in zip(cases, dg) if d & bw.KAT_DEDUP_HANDED]
        assert handed == 2 and over == [f"win{w}+1", f"win{w}+1_n42"], over


def test_launch_shapes(ctx, judged):
    """The same lists on either list and at read 0, 1 and last; rank_sort_min 2 and 2^30 (every sort on one lane)."""
    want_f, want_p = judged("fast"), judged("patch")
    cases = dc.cases_of("fast")[:9] + dc.cases_of("patch")[:9]
    want = want_f[:9] + want_p[:9]
    opt = dc.opt_of("fast")
    for heavy in (np.zeros(18, np.uint8), np.ones(18, np.uint8), np.arange(18, dtype=np.uint8) % 2):
        for rsm in (2, 1 << 30):
            ctx.tune(rank_sort_min=rsm)
            try:
                for rot in (0, 1, 17):
                    order = [(k + rot) % 18 for k in range(18)]
                    cs = [cases[k] for k in order]
                    got, dg, _ = ctx.kat_dedup(*dc.pack(cs)[:4], opt=opt, heavy=heavy, form=bw.KAT_DEDUP_PRODUCT)
                    bad = differing(got, [want[k] for k in order], cs)
                    assert not bad, (rsm, rot, bad[:5])
                    if rsm > 2:
                        assert all(d & bw.KAT_DEDUP_FAST or (d & bw.KAT_DEDUP_LANE1 and d & bw.KAT_DEDUP_LANE2) for d in dg)
            finally:
                ctx.tune(rank_sort_min=2)


def test_one_batch_mixes_every_taker(ctx, judged):
    """The set `mixed` (judged list by list in test_set_equals_oracle_golden_and_model) really has k_dedup_fast, k_dedup in LDS and k_dedup
    in global memory finish lists of one batch."""
    cases = dc.cases_of("mixed")
    _, dg, _ = check(ctx, "mixed", judged("mixed"), bw.KAT_DEDUP_PRODUCT)
    assert {int(d) & 15 for d in dg} == {bw.KAT_DEDUP_FAST, bw.KAT_DEDUP_STAGED, bw.KAT_DEDUP_GLOBAL}


def test_more_reads_than_either_grid(ctx, judged):
    """4 097 reads of two regions on the heavy reads' list (k_dedup's grid there is 4 096) and 32 769 on the bulk's (k_dedup_fast's and
    k_dedup's grid is 32 768): the stride loops take a second turn.  The lists are the two-region lists of the set `fast` -- one the fast
    form finishes, a tie in re, a patch candidate that merges, one that fails the ratio -- repeated in turn.  k_dedup's second turn is reached on the
    heavy list in both forms and on the bulk list in form `full`, k_dedup_fast's in form `product` (the list k_dedup_fast passes on
    holds three reads in four, fewer than that launch's grid); each read must come back as the oracle's answer for its list."""
    src = [i for i, c in enumerate(dc.cases_of("fast")) if len(c.regs) == 2 and len(c.seq) == 150]
    assert len(src) >= 4
    cs, want = [dc.cases_of("fast")[i] for i in src], [judged("fast")[i] for i in src]
    n = 4097 + 32769
    pick = np.arange(n) % len(cs)
    codes = np.stack([c.seq for c in cs])[pick].ravel()
    regs = np.stack([c.regs for c in cs])[pick].reshape(-1, 19)
    heavy = (np.arange(n) < 4097).astype(np.uint8)
    for form in (bw.KAT_DEDUP_PRODUCT, bw.KAT_DEDUP_FULL):
        got, dg, handed = ctx.kat_dedup(codes, np.arange(n + 1) * 150, np.arange(n + 1) * 2, regs, opt=dc.opt_of("fast"), heavy=heavy, form=form)
        bad = [i for i in range(n) if not np.array_equal(got[i], want[pick[i]][0])]
        assert not bad and handed == 0, (form, len(bad), bad[:5])
        pred = np.array([dc.predict("fast", c, w[1], form) for c, w in zip(cs, want)], dtype=np.int32)
        pred_h = np.array([dc.predict("fast", _as_heavy(c), w[1], form) for c, w in zip(cs, want)], dtype=np.int32)
        assert np.array_equal(dg, np.where(heavy > 0, pred_h[pick], pred[pick]))


def _as_heavy(c):
    d = dc._bare(c)
    d.heavy = True
    return d


def test_empty_batch_and_bad_input(ctx):
    """n_reads == 0 launches nothing; descending offsets, a list of fewer than 2 regions, qe < qb, re < rb, a contig outside the index, a
    region across l_pac or beyond its contig, qe beyond the read are refused."""
    got, dg, handed = ctx.kat_dedup(np.zeros(0, np.uint8), [0], [0], np.zeros((0, 19)))
    assert got == [] and len(dg) == 0 and handed == 0
    seq = np.zeros(150, np.uint8)
    a, b = dc.words(dc.reg(100, 200, 0, 100, 50), 0), dc.words(dc.reg(300, 400, 10, 110, 60), 1)
    assert len(ctx.kat_dedup(seq, [0, 150], [0, 2], [a, b])[0][0]) == 2

    def with_(col, v):
        r = list(b)
        r[col] = v
        return r
    for off, roff, regs in (([0, 150], [0, 1], [a]), ([0, 150, 100], [0, 2, 4], [a, b, a, b]), ([0, 150, 300], [0, 3, 2], [a, b, a, b]),
                            ([0, 150], [0, 2], [a, with_(dc.C_QE, 5)]), ([0, 150], [0, 2], [a, with_(dc.C_RE, 299)]), ([0, 150], [0, 2], [a, with_(dc.C_RID, 3)]),
                            ([0, 150], [0, 2], [a, with_(dc.C_RID, -1)]), ([0, 150], [0, 2], [a, with_(dc.C_RE, 60010)]), ([0, 150], [0, 2], [a, with_(dc.C_RE, 40001)]),
                            ([0, 150], [0, 2], [a, with_(dc.C_QE, 151)]), ([0, 150], [0, 2], [a, with_(dc.C_RID, 1)])):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.kat_dedup(np.zeros(max(off), np.uint8), off, roff, regs)
