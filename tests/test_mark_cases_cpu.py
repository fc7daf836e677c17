"""The cases of tests/mark_cases.py checked before a GPU sees them.  Every set goes through `bwa_oracle katmark` (ora_kat_mark: the
restatement's mark primary, -5, mapQ, and the selection ora_reg2sam / ora_gen_alt share); its records must equal the reference-made digests
of tests/golden/kat_mark.npz and -- where oracle/_ref/bwaref is built -- the reference's own mem_mark_primary_se / mem_reorder_primary5 /
mem_approx_mapq_se (`bwaref katmark`) on every word the reference can give.  The two sides of every threshold pair must really come out
differently, and the sets must reach what they were built for, counted from the records.  A disagreement here is a bug of the oracle or of a
case builder, not of a kernel."""
import os

import numpy as np
import pytest

import common
import mark_cases as mc

_runs = {}


def run(exe, name, workdir):
    if (exe, name) not in _runs:
        _runs[exe, name] = mc.run_checker(exe, name, str(workdir), "ref" if exe == common.BWAREF else "ora")
    return _runs[exe, name]


def oracle(name, workdir):
    return run(common.ORACLE, name, workdir)


def reference_or_oracle(name, workdir):
    """The reference's records where it is built; otherwise the oracle's, which test_oracle_equals_reference_made_golden pins to them."""
    return run(common.BWAREF if common.have_ref() else common.ORACLE, name, workdir)


@pytest.mark.parametrize("name", list(mc.SETS))
def test_oracle_equals_reference_made_golden(tmp_path, name):
    """kat_mark.npz (tests/golden/make_golden.py mark): per set the sha256 of the generated inputs and, per read, of the record `bwaref
    katmark` wrote."""
    g = np.load(os.path.join(common.GOLDEN, "kat_mark.npz"))
    cases = mc.cases_of(name)
    assert str(g[f"{name}.inputs"]) == mc.input_digest(name), "the case generator drifted: regenerate tests/golden/kat_mark.npz"
    got = mc.digests(oracle(name, tmp_path))
    bad = [cases[i].name for i in range(len(cases)) if got[i] != g[f"{name}.sha"][i]]
    assert not bad, f"{len(bad)} reads differ from the reference's records, first {bad[:5]}"


@pytest.mark.skipif(not common.have_ref(), reason="oracle/_ref/bwaref not built (reference absent)")
@pytest.mark.parametrize("name", list(mc.SETS))
def test_oracle_equals_reference_katmark(tmp_path, name):
    cases = mc.cases_of(name)
    got, want = oracle(name, tmp_path), run(common.BWAREF, name, tmp_path)
    bad = [cases[i].name for i in range(len(cases)) if not np.array_equal(mc.shared(got[i]), want[i])]
    assert not bad, f"{name}: {len(bad)} of {len(cases)} reads differ from the reference, first {bad[:5]}"
    assert all(int(w[2]) == 0 and int(w[3]) == 0 and not mc.body(w)[:, [mc.C_NEED, mc.C_OWNER, mc.C_BAD]].any() for w in want)


@pytest.mark.parametrize("name", [s for s in mc.SETS if mc.pairs_of(s)])
def test_threshold_pairs_fall_on_both_sides(tmp_path, name):
    """A case at a threshold and its neighbour one step beyond must differ in what the threshold decides -- parent, sub_n, mapQ, the first
    region after -5 from the reference's records; the selection from the oracle's, the reference having none here."""
    ora, ref = oracle(name, tmp_path), reference_or_oracle(name, tmp_path)
    for pair, (kind, a, b) in mc.pairs_of(name).items():
        src = ora if kind == "need" else ref
        assert mc.outcome(src[a], kind) != mc.outcome(src[b], kind), f"{name}: both sides of {pair} give {mc.outcome(src[a], kind)}"


def test_every_threshold_of_the_stage_has_a_pair():
    have = {p.rsplit(".", 1)[0] if p.startswith(("ov.", "five.swap")) else p for s in mc.SETS for p in mc.pairs_of(s)}
    for want in ("ov.0.5", "ov.0.3", "ov.0.9", "subn.7.j0.i0", "subn.7.j1.i0", "subn.7.j1.i1", "subn.10.j0.i0", "subn.10.j1.i1", "subn.14.j1.i0", "five.swap", "sel.T", "sel.T.alone",
                 "sel.drop", "sel.xa.100", "sel.xa.101", "sel.cap", "sel.cap_alt", "mapq.identity", "mapq.coef_len"):
        assert any(h == want or h.startswith(want + ".") for h in have), (want, sorted(have))


def test_list_sizes_and_primary_counts_are_reached(tmp_path):
    """Every list-size class of k_mark (none, one, LDS, one lane block, rank sort, bitonic at and around a power of two, the longest), and
    n_pri of 0, 1, n - 1 and n in each form of the second pass -- counted from the reference's records."""
    recs = reference_or_oracle("sizes", tmp_path)
    assert sorted({int(r[0]) for r in recs}) == sorted(mc.SIZES)
    seen = set()
    for name in ("alt", "sizes", "random"):
        for r in reference_or_oracle(name, tmp_path):
            n, n_pri = int(r[0]), int(r[1])
            cls = 0 if n <= 32 else 1 if n <= 128 else 2
            for what, hit in (("0", n_pri == 0), ("1", n_pri == 1), ("n-1", n_pri == n - 1), ("n", n_pri == n)):
                if hit and n >= 3:
                    seen.add((cls, what))
    assert seen == {(c, w) for c in (0, 1, 2) for w in ("0", "1", "n-1", "n")}, seen


def test_alt_cases_set_alt_sc_and_int_max_in_every_form(tmp_path):
    seen = {}
    for r in reference_or_oracle("alt", tmp_path):
        b = mc.body(r)
        cls = 0 if len(b) <= 32 else 1 if len(b) <= 128 else 2
        d = seen.setdefault(cls, [0, 0, 0])
        d[0] += int((b[:, mc.C_ALTSC] > 0).sum())
        d[1] += int((b[:, mc.C_SEC] == mc.INT_MAX).sum())
        d[2] += int(((b[:, mc.C_SEC] >= 0) & (b[:, mc.C_SEC] != b[:, mc.C_SECALL])).sum())          # the z remap moved a parent
        assert ((b[:, mc.C_SEC] == mc.INT_MAX) <= (b[:, mc.C_ALT] == 1)).all()
    assert set(seen) == {0, 1, 2} and all(min(d) > 0 for d in seen.values()), seen


def test_a_region_that_overlaps_two_kept_ones_goes_to_the_first(tmp_path):
    """Counted on lists without ALT regions (one pass): a secondary region that overlaps two or more kept regions significantly, its
    parent the first of them in the final order."""
    found = 0
    for name in ("kept", "sizes"):
        for r in reference_or_oracle(name, tmp_path):
            b = mc.body(r)
            if not len(b) or b[:, mc.C_ALT].any():
                continue
            kept = [k for k in range(len(b)) if b[k, mc.C_SEC] < 0]
            for i in range(len(b)):
                if b[i, mc.C_SEC] < 0:
                    continue
                over = []
                for k in kept:
                    if k > i:
                        break
                    b_max, e_min = max(b[k, mc.C_QB], b[i, mc.C_QB]), min(b[k, mc.C_QE], b[i, mc.C_QE])
                    min_l = min(b[k, mc.C_QE] - b[k, mc.C_QB], b[i, mc.C_QE] - b[i, mc.C_QB])
                    if e_min > b_max and mc.sig(int(e_min - b_max), int(min_l), 0.5):
                        over.append(k)
                assert over and over[0] == b[i, mc.C_SEC]
                found += len(over) >= 2
    assert found >= 20, found


def test_kept_cases_lie_beyond_the_first_lane_block(tmp_path):
    by = {c.name: mc.body(r) for c, r in zip(mc.cases_of("kept"), reference_or_oracle("kept", tmp_path))}
    b = by["kept.first_absorbed_beyond_64"]
    assert int(np.flatnonzero(b[:, mc.C_SEC] == 0)[0]) > 65 and b[0, mc.C_SUB] == 100
    b = by["kept.next_open_beyond_64"]
    assert [k for k in range(len(b)) if b[k, mc.C_SEC] < 0][:2] == [0, 71]
    b = by["kept.forty"]
    assert int((b[:, mc.C_SEC] < 0).sum()) == 40 and sorted(np.bincount(b[b[:, mc.C_SEC] >= 0, mc.C_SECALL])[np.flatnonzero(b[:, mc.C_SEC] < 0)]) == [2] * 40
    b = by["kept.two_parents"]
    assert [int(x) for x in b[:, mc.C_SEC]] == [-1, -1, 0]


def test_five_cases_swap_in_both_forms(tmp_path):
    """-5 moves a primary from index k > 0 to the front, with secondaries pointing at 0 and at k, in lists of at most and of more than 32."""
    swapped = {}
    for c, r in zip(mc.cases_of("five"), reference_or_oracle("five", tmp_path)):
        b = mc.body(r)
        if "leftmost_at_k" in c.name or c.name.endswith("leftmost_second"):
            sc = b[:, mc.C_SCORE]
            k = int(np.flatnonzero(sc == sc.max())[0])
            assert k > 0 and b[0, mc.C_QB] == 0, c.name                                             # the best region left the front
            assert (b[:, mc.C_SEC] == 0).any() and (b[:, mc.C_SEC] == k).any(), c.name
            swapped[len(b) <= 32] = swapped.get(len(b) <= 32, 0) + 1
        if "none_above_T" in c.name or "one_primary" in c.name or "leftmost_first" in c.name:   # nothing to move
            assert b[0, mc.C_SCORE] == b[:, mc.C_SCORE].max(), c.name
    assert swapped.get(True, 0) >= 2 and swapped.get(False, 0) >= 2, swapped


@pytest.mark.parametrize("name,hits,hits_alt", [("select", 5, 200), ("select_h3,10", 3, 10)])
def test_xa_caps_from_both_sides(tmp_path, name, hits, hits_alt):
    by = {c.name: mc.body(r) for c, r in zip(mc.cases_of(name), oracle(name, tmp_path))}
    n_xa = lambda b: int(((b[:, mc.C_NEED] & 2) != 0).sum())
    assert n_xa(by[f"sel.hits{hits}"]) == hits and n_xa(by[f"sel.hits{hits + 1}"]) == 0 and n_xa(by[f"sel.hits{hits + 1}.alt"]) == hits + 1
    assert n_xa(by[f"sel.hits{hits_alt}.alt"]) == hits_alt and n_xa(by[f"sel.hits{hits_alt + 1}.alt"]) == 0 and n_xa(by[f"sel.hits{hits_alt + 1}"]) == 0
    assert n_xa(by["sel.hits300"]) == 0 and n_xa(by["sel.hits300.alt"]) == 0
    b = by["sel.seventy"]
    own = b[(b[:, mc.C_NEED] & 2) != 0, mc.C_OWNER]
    assert len(own) == 70 and len(set(own)) == 70 and n_xa(by["sel.cap.uncounted"]) == hits


def test_mapq_grid_is_not_flat(tmp_path):
    """The grid must exercise the formula, not its clamps: many distinct values strictly between 0 and 60 under both formulas."""
    for name in ("mapq", "mapq_Q0", "mapq_A2", "mapq_Q0_A2"):
        q = np.concatenate([mc.body(r)[:, mc.C_MAPQ] for r in reference_or_oracle(name, tmp_path)])
        assert len(q) > 4000 and len(set(q[(q > 0) & (q < 60)])) >= 40 and (q == 60).any() and (q == 0).any(), (name, len(q), sorted(set(q)))
