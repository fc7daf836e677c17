"""The cases of tests/dedup_cases.py checked before a GPU sees them.  Every set goes through `bwa_oracle katdedup` (ora_kat_dedup:
ora_sort_dedup_patch over the index's reference, then the is_alt marking) and must equal the reference-made digests of
tests/golden/kat_dedup.npz and -- where oracle/_ref/bwaref is built -- the reference's own mem_sort_dedup_patch (`bwaref katdedup`) on every
word.  The two sides of every threshold pair must really come out differently, every case built for a count must show it, and across the
sets the judge's own counts must reach the floors below: the conditions the generator is held to, not measurements.

Counts of this generator (21 sets, 4 015 lists, 219 018 regions; the three sets run under tuning knobs left out of the counts), by the
judge and the model of who takes a list: k_dedup_fast finishes 337 lists, k_dedup in LDS 2 385, in global memory 1 014; k_dedup_fast refuses
1 136 / 588 / 48 lists for a tie in the first sort / a patch candidate / a tie in the second; mem_patch_reg refuses in 49 (strand) / 1 210
(qb) / 1 260 (qe) / 341 (re) lists; 128 353 alignments run, 19 021 merge, 109 332 fail the ratio; the first sort reaches its depth limit
in 337 lists, the second in 332; the random set alone holds 9 858 exclusions, 119 198 patch alignments and 9 750 identical-hit drops.
Identical hits reach the second sort only under mask_level_redun >= 1 (tests/dedup_cases.py says why), so the random set runs under 1.0,
where a region strictly inside another is still redundant; random_m95 is the same generator under the default."""
import os

import numpy as np
import pytest

import common
import dedup_cases as dc
from common import bw


@pytest.fixture(scope="module")
def prefix(built, tmp_path_factory):
    return dc.make_index(str(tmp_path_factory.mktemp("dedup_g60k")))


@pytest.fixture(scope="module")
def judged(prefix, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dedup_ora"))
    return {name: dc.run_checker(common.ORACLE, name, prefix, d, "ora") for name in dc.SETS}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(common.GOLDEN, "kat_dedup.npz"))


@pytest.mark.parametrize("name", list(dc.SETS))
def test_oracle_equals_golden(judged, gold, name):
    assert str(gold[f"{name}.inputs"]) == dc.input_digest(name), "the case generator drifted: regenerate tests/golden/kat_dedup.npz"
    assert np.array_equal(dc.digests([x[0] for x in judged[name]]), gold[f"{name}.sha"])
    if f"{name}.words" in gold:                                  # the small hand-made sets: the reference's records themselves
        assert np.array_equal(np.concatenate([x[0].ravel() for x in judged[name]]), gold[f"{name}.words"])


@pytest.mark.parametrize("name", list(dc.SETS))
def test_oracle_equals_reference_katdedup(judged, prefix, tmp_path, name):
    if not common.have_ref():
        pytest.skip("oracle/_ref/bwaref is not built here")
    ref = dc.run_checker(common.BWAREF, name, prefix, str(tmp_path), "ref")
    cases = dc.cases_of(name)
    bad = [cases[i].name for i in range(len(cases)) if not np.array_equal(ref[i][0], judged[name][i][0])]
    assert not bad, f"{name}: {len(bad)} of {len(cases)} lists differ from the reference, first {bad[:5]}"


@pytest.mark.parametrize("name", list(dc.SETS))
def test_cases_do_what_they_are_built_for(judged, name):
    """Both sides of a threshold pair differ in the list that comes out; a case built for a count or a refusal reason shows it (sets run
    under other options than the defaults only check the pairs)."""
    cases, out = dc.cases_of(name), judged[name]

    def behaviour(k):
        """What the function did with a list, apart from the coordinates it was given: the final length, which tagged records are left, the
        band and n_comp they carry, and the judge's counts of exclusions, alignments, merges and refusal reasons."""
        regs, st = out[k]
        return (len(regs), tuple(int(x) for x in regs[:, dc.C_SEEDLEN0]), tuple(int(x) for x in regs[:, dc.C_NCOMP]), tuple(int(x) for x in regs[:, dc.C_W]),
                tuple(int(x) for x in st[[dc.S_EXCL_P, dc.S_EXCL_Q, dc.S_ALIGN, dc.S_MERGE, dc.S_WHY]]))
    for p, (a, b) in dc.pairs_of(name).items():
        assert behaviour(a) != behaviour(b), f"{name}: pair {p} comes out the same on both sides: {behaviour(a)}"
        if not p.startswith(("gap_", "ovl_")):    # (the limits pairs differ in whether the alignment runs: the judge's count)
            assert behaviour(a)[:4] != behaviour(b)[:4], f"{name}: pair {p} differs in the judge's counts only"
    if not dc.SETS[name].pairs:
        return
    for c, (_, st) in zip(cases, out):
        e = c.expect
        if "align" in e:
            assert st[dc.S_ALIGN] == e["align"], (c.name, st)
        if "merge" in e:
            assert st[dc.S_MERGE] == e["merge"], (c.name, st)
        if "why" in e:
            assert st[dc.S_WHY] & dc.WHY[e["why"]], (c.name, st)
        if "excl" in e:
            assert st[dc.S_EXCL_P] + st[dc.S_EXCL_Q] == e["excl"], (c.name, st)
        if "n" in e:
            assert len(_) == e["n"], (c.name, len(_))
        if "w" in e:
            assert e["w"] in [int(x) for x in _[:, dc.C_W]], (c.name, _[:, dc.C_W])
        if "why_fast" in e:
            assert dc.fast_model(c.regs, dc.SETS[name].mask, dc.SETS[name].gap, 100) == e["why_fast"], c.name
        if e.get("taker") == "fast":
            assert dc.fast_model(c.regs, dc.SETS[name].mask, dc.SETS[name].gap, 100) == 0, c.name


def test_a_list_k_dedup_fast_finishes_needs_nothing_else(judged):
    """Where the model lets k_dedup_fast finish a list, the judge ran no alignment, met no tie and dropped no identical hit."""
    for name in dc.SETS:
        for c, (_, st) in zip(dc.cases_of(name), judged[name]):
            if dc.predict(name, c, st) == bw.KAT_DEDUP_FAST:
                assert st[dc.S_ALIGN] == 0 and st[dc.S_IDENT] == 0 and not st[dc.S_FLAGS] & dc.F_TIE1, (name, c.name, st)


def test_the_skip_of_excluded_entries_decides_lists():
    """k_dedup_fast must not take an excluded entry for a patch candidate: the model finishes the `behind_excluded` and `behind_collapsed`
    lists and refuses their `behind_live` twins; a model without the skip refuses the `behind_collapsed` lists, whose excluded entry
    passes the pre-tests once its qe has collapsed onto its qb."""
    s = dc.SETS["fast"]
    seen = 0
    for c in dc.cases_of("fast"):
        right, wrong = (dc.fast_model(c.regs, s.mask, s.gap, 100, skip_excluded=k) for k in (True, False))
        if c.name.startswith("behind_collapsed"):
            assert (right, wrong) == (0, 2), (c.name, right, wrong)
            seen += 1
        elif c.name.startswith("behind_excluded"):
            assert right == 0, (c.name, right)
        elif c.name.startswith("behind_live"):
            assert (right, wrong) == (2, 2), (c.name, right, wrong)
    assert seen == 6


def test_floors(judged):
    """The conditions the generator is held to, counted by the judge and the model alone."""
    taker = {bw.KAT_DEDUP_FAST: 0, bw.KAT_DEDUP_STAGED: 0, bw.KAT_DEDUP_GLOBAL: 0}
    why_fast, why, tot = {1: 0, 2: 0, 3: 0}, {k: 0 for k in dc.WHY}, np.zeros(dc.STAT_N, np.int64)
    comb = [0, 0]
    for name in dc.SETS:
        if dc.SETS[name].knobs:
            continue
        for c, (_, st) in zip(dc.cases_of(name), judged[name]):
            d = dc.predict(name, c, st)
            taker[d & 7] += 1
            w = d >> bw.KAT_DEDUP_WHY_SHIFT & 3
            if w:
                why_fast[w] += 1
            for k, b in dc.WHY.items():
                why[k] += bool(st[dc.S_WHY] & b)
            tot += st
            comb[0] += bool(st[dc.S_FLAGS] & dc.F_COMB1)
            comb[1] += bool(st[dc.S_FLAGS] & dc.F_COMB2)
    print("takers", taker, "fast refusals", why_fast, "patch refusals", why, "sums", tot, "depth limits", comb)
    assert min(taker.values()) >= 50, taker
    assert min(why_fast.values()) >= 20, why_fast
    assert min(why[k] for k in ("strand", "qb", "qe", "re")) >= 10, why
    assert tot[dc.S_ALIGN] >= 50 and tot[dc.S_MERGE] >= 20 and tot[dc.S_RATIO] >= 20, tot
    assert min(comb) >= 10, comb
    rnd = np.array([st for _, st in judged["random"]])
    assert rnd[:, dc.S_EXCL_P].sum() + rnd[:, dc.S_EXCL_Q].sum() >= 100 and rnd[:, dc.S_ALIGN].sum() >= 20
    assert rnd[:, dc.S_IDENT].sum() >= 20, rnd[:, dc.S_IDENT].sum()
    print("random: exclusions", rnd[:, dc.S_EXCL_P].sum() + rnd[:, dc.S_EXCL_Q].sum(), "alignments", rnd[:, dc.S_ALIGN].sum(), "identical hits", rnd[:, dc.S_IDENT].sum())
