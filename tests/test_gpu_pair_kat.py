"""Known answers for the pairing stage: k_pair of csrc/k_pair.hip (the rank sort of v by shuffle up to 64 keys and the bitonic network in
the spare region array beyond, the per-lane best and second of u with their reduction across lanes, the second pass for n_sub, the
tie-breaking hash of the pair id, is_multi, score_un, q_pe and q_se, the sub adopted from a secondary z[i], the re-parenting of
secondary_all, the selection after select_records), fed pairs of region lists directly through bwahip_kat_pair -- the paired-end path's own
buffers in their tightest layout, its own marking and its own launches -- against ora_kat_pair (`bwa_oracle katpair`), which
tests/test_pair_cases_cpu.py pins to the reference's mem_mark_primary_se / mem_reorder_primary5 / mem_pair, and against the
reference-made tests/golden/kat_pair.npz.  Every word is an integer and the penalty table is made by the host's libm: nothing is
tolerated."""
import os

import numpy as np
import pytest

import chain_cases as cc
import common
import mark_cases as mc
import pair_cases as pc
from common import bw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def alt(small_index, tmp_path_factory):
    return cc.alt_index(small_index, tmp_path_factory.mktemp("pair_alt"))


@pytest.fixture(scope="module")
def ctx(alt):
    c = bw.Context(alt)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(common.GOLDEN, "kat_pair.npz"))


def answers(recs):
    return [r[bw.KAT_PAIR_TAG] for r in common.by_read(recs)]


def differing(got, want, cases):
    return sorted({cases[i // 2].name for i in range(len(want)) if not np.array_equal(got[i], want[i])})


def device(ctx, name, pairs=None):
    s = pc.SETS[name]
    off, regs = pc.pack(pc.cases_of(name))
    return answers(ctx.kat_pair(off, regs, pc.pes_of(name), opt=pc.opt_of(name), n_processed=s.n_processed, pairs=pairs))


@pytest.mark.parametrize("name", list(pc.SETS))
def test_set_equals_oracle_and_golden(ctx, alt, gold, tmp_path, name):
    """Per set every word of every read equals the oracle's, and what the reference gives of it equals the reference's digests."""
    cases = pc.cases_of(name)
    assert str(gold[f"{name}.inputs"]) == pc.input_digest(name), "the case generator drifted: regenerate tests/golden/kat_pair.npz"
    want = [r[pc.TAG_PAIR] for r in pc.run_checker(common.ORACLE, name, alt, str(tmp_path), "ora")]
    got = device(ctx, name)
    assert len(got) == len(want) == 2 * len(cases)
    bad = differing(got, want, cases)
    assert not bad, f"{name}: {len(bad)} of {len(cases)} pairs differ from the oracle, first {bad[:5]}"
    assert np.array_equal(pc.digests_of_device(got), gold[f"{name}.sha"]), f"{name}: differs from the reference's records"


@pytest.mark.parametrize("name", ["sizes", "lanes", "ties_2p31m4", "choice_U17", "reparent", "alt", "unpaired", "random_5"])
def test_two_launches_equal_one(ctx, name):
    """The paired-end path marks and pairs a batch in two launches: every pair but the listed ones, then the listed pairs.  With every
    third pair listed -- and with all, and with none -- the batch must come back exactly as from one launch."""
    cases = pc.cases_of(name)
    n_pairs = len(cases)
    one = device(ctx, name)
    for listed in (list(range(0, n_pairs, 3)), list(range(n_pairs - 1, -1, -1)), []):
        two = device(ctx, name, pairs=listed)
        bad = differing(two, one, cases)
        assert not bad, f"{name}, {len(listed)} pairs listed: {len(bad)} pairs differ, first {bad[:5]}"


def test_log_table_boundary(ctx, alt, tmp_path):
    """255 x 257 candidates of one score: n_sub + 1 = 65535 is the table's last entry and the answer is the oracle's (it is part of the set
    `logtab` above; here the count itself is looked at).  256 x 256: n_sub + 1 = 65536 lies beyond it, the kernel reports code 61 and the
    entry BWAHIP_EINTERNAL."""
    got = device(ctx, "logtab")
    assert got[0][pc.H_NSUB] == 65534 and got[0][pc.H_MODE] == 1
    c = pc.bad_logtab_case()
    off, regs = pc.pack([c])
    with pytest.raises(bw.BwahipError, match="EINTERNAL"):
        ctx.kat_pair(off, regs, pc.pes_of("logtab"))
    got = answers(ctx.kat_pair(*pc.pack([pc.logtab_case(3, 5)]), pc.pes_of("logtab")))      # the context goes on working
    assert got[0][pc.H_NSUB] == 14


def test_empty_batch_and_bad_input(ctx):
    """n_reads == 0 launches nothing; what bwahip_kat_mark refuses is refused, and so are pes == NULL, an odd batch and a live orientation
    whose window exceeds 2^26."""
    fr = pc.pes_of("lanes")
    assert ctx.kat_pair([0], np.zeros((0, 19)), fr) == []
    ok = pc.preg(5000, 0, 90)
    assert len(answers(ctx.kat_pair([0, 1, 2], [ok, ok], fr))) == 2
    assert len(answers(ctx.kat_pair([0, 0, 0], np.zeros((0, 19)), fr))) == 2

    def with_(col, v):
        r = list(ok)
        r[col] = v
        return r
    wide = pc.pes_of("lanes")
    wide[1].low, wide[1].high = 1, (1 << 26) + 2
    for off, regs, p, kw in (([0, 2, 1], [ok, ok], fr, {}), ([1, 2, 3], [ok] * 3, fr, {}), ([0, 1, 2], [with_(3, -1), ok], fr, {}), ([0, 1, 2], [with_(1, ok[0] - 1), ok], fr, {}),
                             ([0, 1, 2], [with_(4, 3), ok], fr, {}), ([0, 1, 2], [ok, with_(4, -1)], fr, {}), ([0, 1], [ok], fr, {}), ([0, 1, 2, 3], [ok] * 3, fr, dict(pairs=[0])),
                             ([0, 1, 2], [ok, ok], fr, dict(pairs=[1])), ([0, 1, 2], [ok, ok], fr, dict(pairs=[-1])), ([0, 1, 2, 3, 4], [ok] * 4, fr, dict(pairs=[1, 1])),
                             ([0, 1, 2], [ok, ok], None, {}), ([0, 1, 2], [ok, ok], wide, {})):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.kat_pair(off, regs, p, **kw)
    wide[1].failed = 1                                     # a failed orientation's window is not looked at
    assert len(answers(ctx.kat_pair([0, 1, 2], [ok, ok], wide))) == 2
    assert len(answers(ctx.kat_pair([0, 1, 2, 3, 4], [ok] * 4, fr, pairs=[1]))) == 4


def test_entry_leaves_the_marking_entry_alone(ctx):
    """bwahip_kat_mark and bwahip_kat_pair share their upload and marking: a call of one between two calls of the other changes nothing."""
    cases = mc.cases_of("alt")
    off, regs = mc.pack(cases)
    a = [r[bw.KAT_MARK_TAG] for r in common.by_read(ctx.kat_mark(off, regs))]
    p1 = device(ctx, "alt")
    b = [r[bw.KAT_MARK_TAG] for r in common.by_read(ctx.kat_mark(off, regs))]
    p2 = device(ctx, "alt")
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(p1, p2))
