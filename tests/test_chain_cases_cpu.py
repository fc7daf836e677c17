"""The cases of tests/chain_cases.py checked before a GPU sees them.  Every set goes through `bwa_oracle katchain` (ora_kat_chain); the reason
each case was built for must hold on the oracle's chains, the B-tree of every read must fit the node budget of every kernel variant that can
take it, and the oracle's records must equal the reference-made tests/golden/kat_chain.npz on the core sets and -- where oracle/_ref/bwaref
is built -- the reference's own kbtree / test_and_merge / mem_chain_flt (`bwaref katchain`) on every set, the flood included.  A
disagreement here is a bug of the oracle or of a case builder, not of a kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import chain_cases as cc
import common
from common import bw


@pytest.fixture(scope="module")
def alt(small_index, tmp_path_factory):
    return cc.alt_index(small_index, tmp_path_factory.mktemp("chain_alt"))


_oracle = {}


def oracle(alt, name, workdir):
    if name not in _oracle:
        _oracle[name] = cc.run_checker(common.ORACLE, alt, cc.cases_of(name), cc.SETS[name][0], str(workdir), "ora")
    return _oracle[name]


def test_layout_and_contigs_are_the_index_own(alt):
    """chain_cases hard-codes the genome's layout and restates bns_intv2rid: both must be the index's (liboracle's ora_intv2rid)."""
    class Ann(C.Structure):
        _fields_ = [("offset", C.c_int64), ("len", C.c_int32), ("n_ambs", C.c_int32), ("gi", C.c_uint32), ("is_alt", C.c_int32), ("name", C.c_char_p), ("anno", C.c_char_p)]

    class Ref(C.Structure):
        _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("seed", C.c_uint32), ("anns", C.POINTER(Ann))]

    class Idx(C.Structure):
        _fields_ = [("fmi", C.c_void_p), ("ref", C.POINTER(Ref))]
    ora = C.CDLL(os.path.join(common.ROOT, "oracle", "liboracle.so"))
    ora.ora_index_load.restype = C.POINTER(Idx)
    ora.ora_index_load.argtypes = [C.c_char_p]
    ora.ora_intv2rid.argtypes = [C.POINTER(Ref), C.c_int64, C.c_int64]
    ref = ora.ora_index_load(alt.encode()).contents.ref
    r = ref.contents
    assert r.l_pac == cc.L_PAC and r.n_seqs == 3
    assert [(r.anns[i].offset, r.anns[i].len) for i in range(3)] == list(zip(cc.CTG_OFF, cc.CTG_LEN))
    assert [r.anns[i].is_alt for i in range(3)] == [0, 0, 1]
    n = 0
    for name in cc.SETS:
        if name.startswith("filter_") or name.startswith("merge_w"):
            continue                                        # the same builders as "filter" / "merge"
        for c in cc.cases_of(name):
            for rb, _, ln, rid in c.seeds[:: max(1, len(c.seeds) // 50)]:
                assert max(-1, ora.ora_intv2rid(ref, int(rb), int(rb + ln))) == rid, (c.name, rb, ln)
                n += 1
    assert n > 5000


def _chains(rd):
    return cc.chain_list(rd[bw.STAGE_CHAIN]), cc.chain_list(rd[bw.STAGE_CHAIN_FLT])


@pytest.mark.parametrize("name", cc.FAMILIES["merge"])
def test_merge_cases_take_the_intended_branch(alt, tmp_path, name):
    reads, _ = oracle(alt, name, tmp_path)
    seen = set()
    for c, rd in zip(cc.cases_of(name), reads):
        un, _ = _chains(rd)
        given = len(c.seeds) - 1                              # the seeds in front of the one under test: one chain
        n_seeds = sum(ch[6] for ch in un)
        if c.expect == "merge":
            assert (len(un), n_seeds) == (1, given + 1), c.name
        elif c.expect == "new":
            assert (len(un), n_seeds) == (2, given + 1), c.name
        elif c.expect == "swallow":
            assert (len(un), n_seeds) == (1, given), c.name
        elif c.expect == "skip":
            assert (len(un), n_seeds) == (1, given) and c.seeds[-1][3] < 0, c.name
        seen.add(c.expect)
    assert seen >= {"merge", "new", "swallow", "skip"}
    names = " ".join(c.name for c in cc.cases_of(name))
    assert all(what in names for what in ("y=0", "y=-1", "l_pac.fwd_then_rev", "l_pac.rev_then_fwd", "rid<0", "other_rid"))
    if name != "merge_G50":
        assert all(what in names for what in ("x-y=w+0", "x-y=w+1", "y-x=w+0", "y-x=w+1"))
    else:
        assert all(f"{v}-len=G{d}" in names for v in "xy" for d in ("-1", "+0"))


def test_node_budget_holds_for_every_tree_a_kernel_can_be_given():
    """bt_new / wbt_new have no capacity check; what keeps them inside their arrays is kbtree's own invariant: with t = 6 every node but
    the root holds at least 5 keys and the root at least 1, so a tree of S keys has at most (S - 1) / 5 + 1 nodes.  That is within the 72 /
    400 / 800 LDS nodes at the most seeds a class admits (the knobs cannot raise 256 / 1536 / 3200), and within the S / 4 + 4 global slots
    for every S (the slots of read r begin at (seed_base >> 2) + 4 r, so it owns at least floor(S / 4) + 4 of them)."""
    bound = lambda s: (s - 1) // 5 + 1 if s else 1
    assert bound(cc.SMALL_SEEDS) <= cc.NODE_CAP[0] and bound(cc.MID_SEEDS) <= cc.NODE_CAP[1] and bound(cc.BIG_SEEDS) <= cc.NODE_CAP[2]
    assert all(bound(s) <= s // 4 + 4 for s in range(0, 70_000))


def test_tree_cases_open_a_chain_per_seed_and_stay_within_capacity(alt, tmp_path):
    reads, stats = oracle(alt, "tree", tmp_path)
    heights = set()
    for c, rd, st in zip(cc.cases_of("tree"), reads, stats):
        un, _ = _chains(rd)
        n, ties = len(c.seeds), int(c.name.split(".")[3])
        assert len(un) == n and all(ch[6] == 1 for ch in un), c.name
        pos = [ch[0] for ch in un]
        assert pos == sorted(pos)
        assert max(np.bincount(np.unique(pos, return_inverse=True)[1])) == (ties + 1 if ties else 1), c.name
        assert st[0] <= (n - 1) // 5 + 1
        for knobs in cc.SETS["tree"][2].values():             # every variant this read is sent to
            assert st[0] <= cc.node_room(n, cc.expected_taker(n, knobs)), (c.name, knobs, st[0])
        assert st[0] <= n // 4 + 4                            # ... and the global slots, were it helped out
        heights.add(int(st[1]))
    assert heights >= {2, 3, 4, 5}, heights
    by_n = {n: max(int(st[0]) for c, st in zip(cc.cases_of("tree"), stats) if len(c.seeds) == n) for n in (256, 1536, 3200)}
    print("most nodes at 256 / 1536 / 3200 chains:", by_n)
    assert by_n[256] <= 72 and by_n[1536] <= 400 and by_n[3200] <= 800
    # the equal positions really come out in an order that depends on the tree: not always the order they went in
    moved = 0
    for c, rd in zip(cc.cases_of("tree"), reads):
        if c.name.endswith(".12"):
            un, _ = _chains(rd)
            p_tie = max(set(ch[0] for ch in un), key=[ch[0] for ch in un].count)
            out_q = [int(ch[7][0][1]) for ch in un if ch[0] == p_tie]
            in_q = [int(q) for r, q, _, _ in c.seeds if r == p_tie]
            moved += out_q != in_q
    assert moved >= 10, moved


def test_sort_area_always_fits():
    """The wave sort of k_chain_big needs n * 20 + 8 + 4 * ws_work_ints(n) bytes (+ 2048 when it shares the LDS with its tables); the area is
    the class's LDS less 512 bytes, or 32 bytes per seed of the filter's scratch.  With n <= the seeds a class admits this always fits, so
    the kernel's "area too small" hand-over to the one-lane sort cannot be reached by any input: no case is built for it, and
    test_gpu_chain_kat.py asserts that the diagnostics never report it."""
    def need(n, lds):
        is_scratch = 6 * (n // 64 + 1) + 2 * (n // 2 + 1)
        return n * 20 + 8 + 4 * (is_scratch + n + n // 4 + 4) + (2048 if lds else 0)
    for cls, s_max in ((0, cc.SMALL_SEEDS), (1, cc.MID_SEEDS), (2, cc.BIG_SEEDS)):
        assert all(need(n, True) <= cc.NODE_CAP[cls] * 192 - 512 for n in range(2, s_max + 1)), cls
    assert all(need(n, False) <= 32 * s for s in range(cc.SMALL_SEEDS + 1, 4000) for n in (s,))   # global nodes / helped out: S > 256, n <= S
    assert all(need(n, False) <= 32 * 100_000 for n in (65_535,))


def test_sort_cases_reach_the_sorts_they_are_for(alt, tmp_path):
    reads, stats = oracle(alt, "sort", tmp_path)
    deep = []
    for c, rd, st in zip(cc.cases_of("sort"), reads, stats):
        un, flt = _chains(rd)
        assert len(un) == len(c.seeds) == st[2], c.name       # one chain per seed, none below min_chain_weight
        w = [ch[3] for ch in flt]
        assert w == sorted(w, reverse=True)
        if c.name.endswith(".depth"):
            deep.append(int(st[3]))
        elif c.name.endswith(".equal") or c.name.endswith(".two"):
            assert st[3] == 0, c.name                         # (weights that rise or fall along the tree reach the limit too, without ties)
    assert sorted(set(len(c.seeds) for c in cc.cases_of("sort"))) == sorted(cc.SORT_COUNTS + (129, 600))
    assert deep and all(deep), "no case reaches the introsort's depth limit"


def _kept_of(flt, q, ln):
    """kept of the chain whose first seed is (qbeg q, len ln); None when the filter dropped it"""
    hit = [ch[4] for ch in flt if int(ch[7][0][1]) == q and int(ch[7][0][2]) == ln]
    assert len(hit) <= 1
    return hit[0] if hit else None


@pytest.mark.parametrize("name", ["filter", "filter_G50", "filter_W40"])
def test_filter_cases_sit_on_their_edges(alt, tmp_path, name):
    reads, stats = oracle(alt, name, tmp_path)
    by = {c.name: (c, rd, st) for c, rd, st in zip(cc.cases_of(name), reads, stats)}
    Q = 260
    sizes = set()
    for pad in (0, 40, 70):
        P = f"flt.p{pad}."
        k = lambda case, q, ln: _kept_of(_chains(by[P + case][1])[1], q, ln)
        if name == "filter":
            assert (k("mask.19", Q + 181, 40), k("mask.20", Q + 180, 40), k("mask.21", Q + 179, 40)) == (3, 1, 1)
            assert (k("drop.49", Q + 10, 49), k("drop.50", Q + 10, 50), k("drop.51", Q + 10, 51)) == (None, 1, 1)
            assert (k("diff.31", Q + 5, 31), k("diff.32", Q + 5, 32), k("diff.33", Q + 5, 33)) == (None, None, 1)
            assert (k("alt_over_pri", Q + 10, 40), k("pri_over_alt", Q + 10, 40), k("alt_over_alt", Q + 10, 40)) == (3, 1, 1)
            assert (k("first.kept_then_dropped", Q + 5, 80), k("first.kept_then_dropped", Q + 10, 30)) == (1, None)
            assert (k("first.two_dropped", Q + 5, 30), k("first.two_dropped", Q + 10, 29), k("first.two_dropped", Q + 310, 28)) == (1, None, 1)
        if name == "filter_G50":
            assert (k("minl.49", Q + 3, 49), k("minl.50", Q + 3, 50), k("minl.51", Q + 3, 51)) == (1, 3, 3)
        for case in ("mask.20", "extend", "multi"):
            sizes.add(int(by[P + case][2][2]))
    assert min(sizes) <= 32 and max(sizes) > 64 and any(32 < s <= 64 for s in sizes)
    if name == "filter":
        for n_kept in (63, 64, 65, 130):
            for kk in sorted({0, 63, 64, n_kept - 1}):
                if kk < n_kept:
                    c, rd, st = by[f"flt.kept{n_kept}.shadow{kk}"]
                    _, flt = _chains(rd)
                    assert st[2] == n_kept + 2 and len(flt) == n_kept + 1        # all but the second light chain
                    assert [ch[3] for ch in flt[:n_kept]] == [400 - i for i in range(n_kept)]
                    assert flt[kk][5] == n_kept and flt[n_kept][4] == 1 and all(ch[5] != n_kept for i, ch in enumerate(flt) if i != kk), (n_kept, kk)
        assert by["flt.count32"][2][2] == 32 and by["flt.count33"][2][2] == 33
        assert by["flt.survive32"][2][2] == 38 and by["flt.survive33"][2][2] == 39
    if name == "filter_W40":
        assert by["flt.survive32"][2][2] == 32 and by["flt.survive33"][2][2] == 33
        assert len(_chains(by["flt.survive33"][1])[0]) == 39


@pytest.mark.parametrize("name,n", [("filter_N1", 1), ("filter_N2", 2), ("filter_N5", 5)])
def test_max_chain_extend_cuts_inside_the_cases(alt, tmp_path, name, n):
    """-N below the number of chains with kept 1 / 2: the chain that reaches the limit is zeroed as well (bwamem.c:380-385)."""
    reads, _ = oracle(alt, name, tmp_path)
    base, _ = oracle(alt, "filter", tmp_path)
    cut = 0
    for c, rd, rb in zip(cc.cases_of(name), reads, base):
        a, b = _chains(rd)[1], _chains(rb)[1]
        assert sum(ch[4] in (1, 2) for ch in a) <= max(n - 1, 0) or len(a) == len(b), c.name
        cut += len(a) < len(b)
    assert cut >= 20, cut


def test_class_cases_reach_every_class():
    takers = {kn: [cc.expected_taker(len(c.seeds), knobs) for c in cc.cases_of("classes")] for kn, knobs in cc.CLASS_KNOBS.items()}
    assert set(takers["off"]) == {bw.CHAIN_BY_LANE}
    assert set(takers["all"]) == {bw.CHAIN_BY_LANE, 0, 1} and takers["all"].count(bw.CHAIN_BY_LANE) == 1     # (the read without seeds)
    assert set(takers["min8"]) == {bw.CHAIN_BY_LANE, 0, 1} and set(takers["shipped"]) == {bw.CHAIN_BY_LANE, 1}
    sizes = [len(c.seeds) for c in cc.cases_of("classes")]
    assert [takers["narrow"][sizes.index(s)] for s in (256, 257, 258, 259)] == [0, 1, 2, 3]


def test_random_cases_merge_open_and_tie(alt, tmp_path):
    reads, stats = oracle(alt, "random", tmp_path)
    cases = cc.cases_of("random")
    assert len(cases) == 400 and min(len(c.seeds) for c in cases) >= 1 and max(len(c.seeds) for c in cases) <= 400
    seeds = chains = merged = tied = 0
    for c, rd in zip(cases, reads):
        un, _ = _chains(rd)
        seeds += len(c.seeds); chains += len(un); merged += sum(ch[6] - 1 for ch in un)
        pos = [ch[0] for ch in un]
        tied += len(set(pos)) < len(pos)
    print(f"random: {seeds} seeds, {chains} open a chain, {merged} merge, {tied} reads with chains of equal pos")
    assert merged * 4 >= seeds and chains * 4 >= seeds and tied >= 20


def test_flood_sizes_cross_the_help_out_thresholds():
    for which, n, lo, knobs, cls in ((1, 2049, 257, cc.SETS["flood1"][2]["all"], 1), (2, 513, 258, cc.SETS["flood2"][2]["narrow_mid"], 2)):
        cases = cc.cases_of(f"flood{which}")
        assert len(cases) == n and all(lo <= len(c.seeds) <= 300 for c in cases)
        assert all(cc.expected_taker(len(c.seeds), knobs) == cls for c in cases)
    assert 2049 > 2 * 1024 and 513 > 2 * 256                  # the queue lengths beyond which k_chain_big<0, 3> helps out


@pytest.mark.parametrize("name", [s for s in cc.SETS if cc.SETS[s][3]])
def test_oracle_equals_reference_made_golden(alt, tmp_path, name):
    """kat_chain.npz (tests/golden/make_golden.py chain): per core set the sha256 of the generated inputs and, per case, of the two records
    `bwaref katchain` wrote; the records themselves for the cases of at most 64 seeds."""
    g = np.load(os.path.join(common.GOLDEN, "kat_chain.npz"))
    cases = cc.cases_of(name)
    assert str(g[f"{name}.inputs"]) == cc.input_digest(cases), "the case generator drifted: regenerate tests/golden/kat_chain.npz"
    reads, _ = oracle(alt, name, tmp_path)
    got = cc.digests(reads)
    bad = [cases[i].name for i in range(len(cases)) if not np.array_equal(got[i], g[f"{name}.sha"][i])]
    assert not bad, f"{len(bad)} cases differ from the reference's records, first {bad[:5]}"
    words, off = g[f"{name}.words"], g[f"{name}.off"]
    small = [i for i, c in enumerate(cases) if len(c.seeds) <= 64]
    assert len(off) == len(small) + 1
    for k, i in enumerate(small):
        m = cc.masked([reads[i]])[0]
        assert np.array_equal(np.concatenate([m[bw.STAGE_CHAIN], m[bw.STAGE_CHAIN_FLT]]), words[off[k]:off[k + 1]]), cases[i].name


@pytest.mark.skipif(not common.have_ref(), reason="oracle/_ref/bwaref not built (reference absent)")
@pytest.mark.parametrize("name", list(cc.SETS))
def test_oracle_equals_reference_katchain(alt, tmp_path, name):
    reads, _ = oracle(alt, name, tmp_path)
    ref, _ = cc.run_checker(common.BWAREF, alt, cc.cases_of(name), cc.SETS[name][0], str(tmp_path), "ref")
    got, want = cc.masked(reads), cc.masked(ref)
    common.assert_stage_equal(got, want, bw.STAGE_CHAIN, f"{name}: chains")
    common.assert_stage_equal(got, want, bw.STAGE_CHAIN_FLT, f"{name}: filtered chains")
