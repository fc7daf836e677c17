"""The cases of tests/pair_cases.py checked before a GPU sees them.  Every set goes through `bwa_oracle katpair` (ora_kat_pair: the
restatement's mark primary, -5, mem_pair and -- ora_pe_decide, the block ora_sam_pe runs, which the paired-end SAM parity pins to the
reference -- mem_sam_pe's decisions); what the reference can give of it must equal the reference-made digests of tests/golden/kat_pair.npz
and, where oracle/_ref/bwaref is built, the reference's own mem_mark_primary_se / mem_reorder_primary5 / mem_pair (`bwaref katpair`) word by
word, the overflowing pair ids of the ties sets included.  The two sides of every threshold pair must really come out differently, and the
sets must reach what they were built for, counted from the oracle's extra words.  A disagreement here is a bug of the oracle or of a case
builder, not of a kernel."""
import os

import numpy as np
import pytest

import chain_cases as cc
import common
import pair_cases as pc

_runs = {}


@pytest.fixture(scope="module")
def alt(small_index, tmp_path_factory):
    return cc.alt_index(small_index, tmp_path_factory.mktemp("pair_alt"))


def run(exe, name, alt, workdir):
    if (exe, name) not in _runs:
        _runs[exe, name] = pc.run_checker(exe, name, alt, str(workdir), "ref" if exe == common.BWAREF else "ora")
    return _runs[exe, name]


def oracle(name, alt, workdir):
    return run(common.ORACLE, name, alt, workdir)


def extras(reads):
    return [reads[2 * p][pc.TAG_EXTRA] for p in range(len(reads) // 2)]


def test_contig_table_is_the_one_the_cases_assume(alt):
    with open(alt + ".ann") as f:
        lines = f.read().split("\n")
    assert int(lines[0].split()[0]) == pc.L_PAC and [int(lines[2 + 2 * i].split()[0]) for i in range(3)] == list(pc.CTG_OFF)
    assert [int(lines[2 + 2 * i].split()[1]) for i in range(3)] == list(pc.CTG_LEN)


@pytest.mark.parametrize("name", list(pc.SETS))
def test_oracle_equals_reference_made_golden(alt, tmp_path, name):
    """kat_pair.npz (tests/golden/make_golden.py pair): per set the sha256 of the generated inputs and, per pair, of what `bwaref katpair`
    wrote of it (pair_cases.shared_words)."""
    g = np.load(os.path.join(common.GOLDEN, "kat_pair.npz"))
    cases = pc.cases_of(name)
    assert str(g[f"{name}.inputs"]) == pc.input_digest(name), "the case generator drifted: regenerate tests/golden/kat_pair.npz"
    got = pc.digests_of_checker(oracle(name, alt, tmp_path))
    bad = [cases[i].name for i in range(len(cases)) if got[i] != g[f"{name}.sha"][i]]
    assert not bad, f"{len(bad)} pairs differ from the reference's records, first {bad[:5]}"


@pytest.mark.skipif(not common.have_ref(), reason="oracle/_ref/bwaref not built (reference absent)")
@pytest.mark.parametrize("name", list(pc.SETS))
def test_oracle_equals_reference_katpair(alt, tmp_path, name):
    """Every word the reference gives: the marked lists, mem_pair's ret, sub and n_sub, and z[] where u held anything (mem_pair leaves z
    alone otherwise: the driver's -1 must then still stand, on both sides)."""
    cases = pc.cases_of(name)
    got, want = oracle(name, alt, tmp_path), run(common.BWAREF, name, alt, tmp_path)
    bad = []
    for p, c in enumerate(cases):
        ok = all(np.array_equal(got[2 * p + e][pc.TAG_MARKED], want[2 * p + e][pc.TAG_MARKED]) for e in (0, 1))
        g, w = got[2 * p][pc.TAG_MEMPAIR], want[2 * p][pc.TAG_MEMPAIR]
        ok = ok and np.array_equal(g, w)
        if got[2 * p][pc.TAG_EXTRA][pc.X_NU] == 0:
            ok = ok and list(w) == [0, 0, 0, -1, -1]
        else:
            ok = ok and min(w[3:]) >= 0
        if not ok:
            bad.append(c.name)
    assert not bad, f"{name}: {len(bad)} of {len(cases)} pairs differ from the reference, first {bad[:5]}"


@pytest.mark.parametrize("name", [s for s in pc.SETS if pc.pairs_of(s)])
def test_threshold_pairs_fall_on_both_sides(alt, tmp_path, name):
    ora = oracle(name, alt, tmp_path)
    for pair, (kind, a, b) in pc.pairs_of(name).items():
        assert pc.outcome(ora, a, kind) != pc.outcome(ora, b, kind), f"{name}: both sides of {pair} give {pc.outcome(ora, a, kind)}"


def test_every_threshold_of_the_stage_has_a_pair():
    have = {p for s in pc.SETS for p in pc.pairs_of(s)}
    for want in [f"win.d{d}.up{u}.{e}" for d in range(4) for u in (0, 1) for e in ("low", "high")] + ["nsub.7", "nsub.10", "nsub.9", "multi.e0.j1.own1", "multi.e1.j128.own1",
                                                                                                     "multi.e0.j-1.own1", "choice.U17.up0", "choice.U50.up1", "unp.T.e0", "unp.altT.e1"]:
        assert want in have, (want, sorted(have))


def test_window_cases_pair_exactly_inside(alt, tmp_path):
    """inside [low, high] one element of u and a proper pair; one step outside none -- in each orientation, with either end upstream"""
    for d, nm in enumerate("ff fr rf rr".split()):
        ora = oracle(f"window_{nm}", alt, tmp_path)
        for p, c in enumerate(pc.cases_of(f"window_{nm}")):
            dist = int(c.name.rsplit("dist", 1)[1])
            inside = pc.WIN[0] <= dist <= pc.WIN[1]
            x, r = ora[2 * p][pc.TAG_EXTRA], ora[2 * p][pc.TAG_PAIR]
            assert x[pc.X_NV] == 2 and x[pc.X_NU] == int(inside) and r[pc.H_MODE] == int(inside) and r[pc.H_FLAG] == (3 if inside else 1), c.name
            assert r[pc.H_O] == (pc.q_of(100, 100, dist, pc.WIN) if inside else 0), c.name


def test_failed_masks_leave_the_live_orientations(alt, tmp_path):
    for m in range(16):
        ora = oracle(f"failed_{m:04b}", alt, tmp_path)
        for p, c in enumerate(pc.cases_of(f"failed_{m:04b}")):
            x = ora[2 * p][pc.TAG_EXTRA]
            assert x[pc.X_NV] == 8 and x[pc.X_NU] == 4 - bin(m).count("1"), (m, c.name)
    # the winner moves with the mask: every orientation is the best pair somewhere
    wins = set()
    for m in range(16):
        ora = oracle(f"failed_{m:04b}", alt, tmp_path)
        wins |= {(int(ora[2 * p][pc.TAG_PAIR][pc.H_HREG]), int(ora[2 * p + 1][pc.TAG_PAIR][pc.H_HREG])) for p in range(len(ora) // 2) if ora[2 * p][pc.TAG_PAIR][pc.H_MODE]}
    assert len(wins) >= 4, wins


def test_penalty_sweeps_cover_the_table_and_reach_zero(alt, tmp_path):
    for a in (1, 2, 5):
        for k, st in pc.PEN_STATS.items():
            name = f"penalty_A{a}_{k}"
            ora = oracle(name, alt, tmp_path)
            o = [int(ora[2 * p][pc.TAG_PAIR][pc.H_O]) for p in range(len(ora) // 2)]
            assert len(o) == st[1] - st[0] + 1
            assert o == [pc.q_of(60 * a, 60 * a, dist, st, a) for dist in range(st[0], st[1] + 1)], name
            mode = [int(ora[2 * p][pc.TAG_PAIR][pc.H_MODE]) for p in range(len(ora) // 2)]
            if k == "s1":                                  # the penalty exceeds the two scores: q holds at 0, nothing is paired
                assert o.count(0) > 150 and all(m == (q > 0) for m, q in zip(mode, o)) and max(o) >= 120 * a, name
            else:
                assert min(o) > 0 and len(set(o)) >= 6, name


def test_sizes_reach_every_nv_and_a_long_u(alt, tmp_path):
    ora = oracle("sizes", alt, tmp_path)
    xs = extras(ora)
    assert sorted({int(x[pc.X_NV]) for x in xs}) == sorted(pc.NV)
    assert max(int(x[pc.X_NU]) for x in xs if x[pc.X_NV] == 600) >= 1000
    for nv in pc.NV:                                       # both splits of every size hold candidate pairs, or the sort of v shows nothing
        if nv >= 63:
            assert sum(1 for x in xs if x[pc.X_NV] == nv and x[pc.X_NU] >= 2) >= 3, nv
    # equal x: the order of v falls to y
    eq = 0
    for c in pc.cases_of("sizes"):
        keys = sorted([(pc.key_x(r), 0) for r in c.a] + [(pc.key_x(r), 1) for r in c.b])
        eq += sum(1 for i in range(1, len(keys)) if keys[i][0] == keys[i - 1][0])
    assert eq >= 50, eq


def test_lanes_placements_are_reached(alt, tmp_path):
    """(k, i) of the best and of the second element of u as the oracle found them: i % 64 is the lane of k_pair that meets the element"""
    by = {c.name: x for c, x in zip(pc.cases_of("lanes"), extras(oracle("lanes", alt, tmp_path)))}
    assert all(x[pc.X_NV] == 130 for x in by.values())
    x = by["lanes.one"]
    assert x[pc.X_NU] == 1 and x[pc.X_SI] == -1
    x = by["lanes.two.other_lanes"]
    assert x[pc.X_NU] == 2 and (x[pc.X_BI], x[pc.X_SI]) == (11, 32)
    x = by["lanes.two.same_lane_64_apart"]
    assert x[pc.X_NU] == 2 and (x[pc.X_BI], x[pc.X_SI]) == (11, 75)
    x = by["lanes.two.same_i"]
    assert x[pc.X_NU] == 2 and x[pc.X_BI] == x[pc.X_SI] == 22 and (x[pc.X_BK], x[pc.X_SK]) == (20, 21)
    x = by["lanes.best_at_1"]
    assert (x[pc.X_BK], x[pc.X_BI]) == (0, 1) and x[pc.X_NU] == 3
    x = by["lanes.best_at_last"]
    assert x[pc.X_BI] == 129 and x[pc.X_NU] == 2
    x = by["lanes.second_in_holders_lane"]
    assert x[pc.X_BI] == x[pc.X_SI] and x[pc.X_NU] == 4
    x = by["lanes.second_elsewhere"]
    assert x[pc.X_BI] % 64 != x[pc.X_SI] % 64 and x[pc.X_NU] == 6
    x = by["lanes.crowded"]
    assert x[pc.X_NU] == 54


def test_ties_are_broken_by_the_pair_id(alt, tmp_path):
    """The candidates tie in q: the winner follows hash_64(uy ^ id << 8) with id an int.  From pair 2^23 on the shift leaves 32 bits; the
    winner must move with the id at least once, come back at 2^40 (the same low 32 bits as 0), and wherever bwaref is built
    test_oracle_equals_reference_katpair holds the oracle to the reference's own arithmetic at every one of these ids."""
    win = {}
    for k in pc.NP_TIES:
        ora = oracle(f"ties_{k}", alt, tmp_path)
        for p, c in enumerate(pc.cases_of(f"ties_{k}")):
            x = ora[2 * p][pc.TAG_EXTRA]
            want_nu = 5 if "top2" in c.name else 6 if "top3" in c.name else 40
            assert x[pc.X_NU] == want_nu and ora[2 * p][pc.TAG_PAIR][pc.H_O] == ora[2 * p][pc.TAG_PAIR][pc.H_SUB], c.name
            win.setdefault(c.name, {})[k] = (int(x[pc.X_BK]), int(x[pc.X_BI]), int(x[pc.X_SK]), int(x[pc.X_SI]))
    assert sum(1 for w in win.values() if len(set(w.values())) >= 2) >= 6, win
    assert all(w["0"] == w["2p40"] for w in win.values())
    assert any(w["2p23m1"] != w["2p23"] for w in win.values()) and any(w["2p31m4"] != w["2p31"] for w in win.values())


def test_nsub_counts(alt, tmp_path):
    for name in ("nsub", "nsub_ab", "nsub_del", "nsub_ins"):
        ora = oracle(name, alt, tmp_path)
        by = {c.name: ora[2 * p][pc.TAG_PAIR] for p, c in enumerate(pc.cases_of(name))}
        for n in (0, 1, 63, 64, 65, 1000):
            assert by[f"nsub.n{n}"][pc.H_NSUB] == n and by[f"nsub.n{n}"][pc.H_O] == 200, (name, n)
        tmp = int(next(iter(pc.pairs_of(name))).split(".")[1])
        assert [int(by[f"nsub.gap{tmp}{d:+d}"][pc.H_NSUB]) for d in (-1, 0, 1)] == [2, 2, 1], name


def test_logtab_reaches_the_last_entry(alt, tmp_path):
    ora = oracle("logtab", alt, tmp_path)
    assert ora[0][pc.TAG_EXTRA][pc.X_NU] == 255 * 257 and ora[0][pc.TAG_PAIR][pc.H_NSUB] + 1 == 65535 and ora[0][pc.TAG_PAIR][pc.H_MODE] == 1


def test_multi_cases_place_the_other_hit(alt, tmp_path):
    ora = oracle("multi", alt, tmp_path)
    seen = set()
    for p, c in enumerate(pc.cases_of("multi")):
        x, r = ora[2 * p][pc.TAG_EXTRA], ora[2 * p][pc.TAG_PAIR]
        _, e, j, own, t = c.name.split(".")
        e, own, at_T = int(e[1]), int(own[3]), t == "T-0"
        assert x[pc.X_NU] == 1 and x[pc.X_MULTI] == ((1 << e) if own and at_T else 0) and r[pc.H_MODE] == (0 if own and at_T else 1), c.name
        b = pc.body(ora[2 * p + e][pc.TAG_PAIR])
        kept = [i for i in range(1, len(b)) if b[i, pc.C_SEC] < 0]
        assert kept == ([len(b) - (1 if j == "j-1" else 2)] if own else []), c.name
        seen |= set(kept)
    assert seen == {1, 63, 64, 65, 128, 129}, seen


def test_choice_reaches_every_sign_and_rule(alt, tmp_path):
    signs, rules, capped, z_sec = set(), set(), 0, 0
    for U in (0, 17, 50):
        name = f"choice_U{U}"
        ora = oracle(name, alt, tmp_path)
        for p, c in enumerate(pc.cases_of(name)):
            x = ora[2 * p][pc.TAG_EXTRA]
            r = [ora[2 * p + e][pc.TAG_PAIR] for e in (0, 1)]
            assert x[pc.X_HAS_UN] == 1, c.name
            if "o_un" in c.name:
                assert x[pc.X_O_UN] == int(c.name.split("o_un")[1][:2]), c.name
                signs.add((U, int(np.sign(x[pc.X_O_UN]))))
            if "z_secondary" in c.name:
                e = int(c.name[-1])
                b = pc.body(r[e])
                if U == 0:                                 # 195 against 200 unpaired: the best regions are preferred, nothing is adopted
                    assert r[e][pc.H_HREG] == 0 and r[e][pc.H_FLAG] == 1 and b[1, pc.C_SEC] == 0 and x[pc.X_REPARENT] == 0, c.name
                    continue
                assert r[e][pc.H_HREG] == 1 and b[1, pc.C_SEC] == -2 and b[1, pc.C_SUB] == 100 and x[pc.X_REPARENT] == 1 and list(b[:, pc.C_SECALL]) == [1, -1, 1], c.name
                z_sec += 1
            for w in ("below", "inside", "beyond"):
                if f"q_pe_{w}" in c.name:
                    rules.add((w, tuple(int(q[pc.H_MAPQ]) for q in r)))
            if "csub" in c.name and U == 17:
                e, cs = int(c.name[-1]), int(c.name.split("csub")[1].split(".")[0])
                capped += int(r[e][pc.H_MAPQ]) == int(6.02 * (100 - cs) + .499) < 60 if cs else 0
    assert {(17, -1), (17, 0), (17, 1), (50, -1), (50, 0), (50, 1), (0, -1), (0, 0)} <= signs, signs
    assert z_sec == 4 and capped >= 4 and len(rules) >= 8, (z_sec, capped, rules)


def test_reparent_families(alt, tmp_path):
    for name, k in (("reparent", 0), ("reparent_k1", 1)):
        ora = oracle(name, alt, tmp_path)
        beyond = 0
        for p, c in enumerate(pc.cases_of(name)):
            e, zi = int(c.name.split(".e")[1][0]), int(c.name.rsplit("z", 1)[1])
            r, x = ora[2 * p + e][pc.TAG_PAIR], ora[2 * p][pc.TAG_EXTRA]
            b = pc.body(r)
            fam = [i for i in range(len(b)) if i != zi and (i % 2 == 1 if k else True)]
            assert r[pc.H_MODE] == 1 and r[pc.H_HREG] == zi and x[pc.X_REPARENT] == 1 and b[zi, pc.C_SECALL] == -1 and b[zi, pc.C_SEC] == -2, c.name
            assert all(b[i, pc.C_SECALL] == zi for i in fam) and b[zi, pc.C_SUB] == b[k, pc.C_SCORE], c.name
            if k:
                assert all(b[i, pc.C_SECALL] == 0 for i in range(2, len(b), 2)) and b[0, pc.C_SECALL] == -1, c.name
            beyond += len(fam) > 64 and zi > 64
        assert beyond >= 4, name


def test_alt_cases_print_and_own(alt, tmp_path):
    for name in ("alt", "alt_a"):
        ora = oracle(name, alt, tmp_path)
        for p, c in enumerate(pc.cases_of(name)):
            e = int(c.name[-1])
            r = ora[2 * p + e][pc.TAG_PAIR]
            b = pc.body(r)
            n_xa = lambda own: int(((b[:, pc.C_NEED] & pc.NEED_XA) != 0)[b[:, pc.C_OWNER] == own].sum()) if own >= 0 else 0
            what = c.name.split(".", 1)[1].rsplit(".e", 1)[0]
            if what.startswith("n_pri0"):
                assert r[pc.H_NPRI] == 0 and r[pc.H_MODE] == 0 and ora[2 * p][pc.TAG_EXTRA][pc.X_NV] == 0 and r[pc.H_HREG] == (-1 if "below_T" in what else 0), c.name
                continue
            assert r[pc.H_MODE] == 1 and r[pc.H_NPRI] < r[pc.H_N] or what == "many_xa", c.name
            printable = what in ("printable", "printable.xa", "at_T", "on_top", "xa_of_neither")
            assert (r[pc.H_ALT] == r[pc.H_NPRI]) == printable and (printable or r[pc.H_ALT] == -1 or what == "many_xa") and r[pc.H_REC] == 1 + printable, c.name
            if name == "alt":
                assert n_xa(0) == (0 if what in ("many_xa", "on_top") else 4) and n_xa(int(r[pc.H_ALT])) == (3 if what == "printable.xa" else 0), c.name
                assert ((b[:, pc.C_NEED] & pc.NEED_XA) != 0).sum() == n_xa(0) + n_xa(int(r[pc.H_ALT])), c.name
            else:
                assert not (b[:, pc.C_NEED] & pc.NEED_XA).any(), c.name


def test_unpaired_cases_choose_h(alt, tmp_path):
    for name in ("unpaired", "unpaired_P"):
        ora = oracle(name, alt, tmp_path)
        by = {c.name: (ora[2 * p][pc.TAG_PAIR], ora[2 * p + 1][pc.TAG_PAIR], ora[2 * p][pc.TAG_EXTRA]) for p, c in enumerate(pc.cases_of(name))}
        assert all(r0[pc.H_MODE] == 0 and r0[pc.H_FLAG] == 1 for k, (r0, _, _) in by.items() if name == "unpaired_P" or k != "unp.proper_candidate")
        assert by["unp.proper_candidate"][0][pc.H_MODE] == (name == "unpaired")
        assert [int(by["unp.both_empty"][e][pc.H_HREG]) for e in (0, 1)] == [-1, -1] and by["unp.empty0"][1][pc.H_HREG] == 0
        for e in (0, 1):
            assert by[f"unp.alt_T-0.e{e}"][e][pc.H_HREG] == 1 and by[f"unp.alt_T-1.e{e}"][e][pc.H_HREG] == -1
            b = pc.body(by[f"unp.alt_T-0.e{e}"][e])
            assert b[1, pc.C_NEED] == pc.NEED_REC and b[0, pc.C_NEED] == 0
        x = by["unp.proper_candidate"][2]
        assert x[pc.X_NU] == (0 if name == "unpaired_P" else 1) and by["unp.two_primaries.e0"][2][pc.X_MULTI] == (0 if name == "unpaired_P" else 1)


def test_contig_cases_break_and_mirror(alt, tmp_path):
    ora = oracle("contigs", alt, tmp_path)
    by = {c.name: (ora[2 * p][pc.TAG_PAIR], ora[2 * p][pc.TAG_EXTRA]) for p, c in enumerate(pc.cases_of("contigs"))}
    for up in (0, 1):
        assert by[f"ctg.neighbours.up{up}"][1][pc.X_NU] == 0 and by[f"ctg.neighbours.up{up}"][0][pc.H_MODE] == 0
        assert by[f"ctg.break.up{up}"][1][pc.X_NU] == 1 and by[f"ctg.break.better_beyond.up{up}"][1][pc.X_NU] == 1
        for nm in ("first_last", "last_contig", "rb_lpac-1", "rb_2lpac-1.rf", "rb_2lpac-1.rr"):
            r, x = by[f"ctg.{nm}.up{up}"]
            assert x[pc.X_NU] == 1 and r[pc.H_MODE] == 1 and r[pc.H_O] == 200, nm
        assert by[f"ctg.rb_lpac.both.up{up}"][1][pc.X_NU] == 2


def test_odd_statistics(alt, tmp_path):
    """std == 0: ns is NaN at the mean and infinite beside it, q falls to 0 and nothing is paired although u holds the candidates;
    low == high admits one distance; a window of 2^20 pairs across half a contig; all orientations failed: u stays empty"""
    ora = oracle("pes_std0", alt, tmp_path)
    assert all(ora[2 * p][pc.TAG_PAIR][pc.H_MODE] == 0 and ora[2 * p][pc.TAG_PAIR][pc.H_O] == 0 for p in range(len(ora) // 2))
    assert sum(int(ora[2 * p][pc.TAG_EXTRA][pc.X_NU] > 0) for p in range(len(ora) // 2)) == len(ora) // 2
    ora = oracle("pes_low_eq_high", alt, tmp_path)
    for p, c in enumerate(pc.cases_of("pes_low_eq_high")):
        assert (ora[2 * p][pc.TAG_EXTRA][pc.X_NU] > 0) == ("dist300" in c.name), c.name
    ora = oracle("pes_2p20", alt, tmp_path)
    assert all(ora[2 * p][pc.TAG_PAIR][pc.H_MODE] == 1 for p in range(len(ora) // 2)) and len({int(ora[2 * p][pc.TAG_PAIR][pc.H_O]) for p in range(len(ora) // 2)}) >= 3
    ora = oracle("pes_all_failed", alt, tmp_path)
    assert all(ora[2 * p][pc.TAG_EXTRA][pc.X_NU] == 0 and ora[2 * p][pc.TAG_EXTRA][pc.X_NV] >= 2 for p in range(len(ora) // 2))


@pytest.mark.parametrize("name", [s for s in pc.SETS if s.startswith("random")])
def test_random_sets_are_mixed(alt, tmp_path, name):
    ora = oracle(name, alt, tmp_path)
    mode = [int(ora[2 * p][pc.TAG_PAIR][pc.H_MODE]) for p in range(len(ora) // 2)]
    assert len(mode) == 300 and 60 <= sum(mode) <= 240, sum(mode)
