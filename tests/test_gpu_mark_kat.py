"""Known answers for the stage between the region list and the output text: k_mark of csrc/k_final.hip (the rank sort and the bitonic
network, the overlap test run one kept region at a time, marking in LDS up to 32 regions and in HBM beyond, the one-region shortcut, the
second pass over the primaries of a list with ALT regions, -5), fin::select_records (record filter, XA membership and its caps) and
fin::approx_mapq_se, fed region lists directly through bwahip_kat_mark -- the finalisation's own buffers and its own launch -- against
ora_kat_mark (`bwa_oracle katmark`), which tests/test_mark_cases_cpu.py pins to the reference's mem_mark_primary_se /
mem_reorder_primary5 / mem_approx_mapq_se, and against the reference-made tests/golden/kat_mark.npz.  Every word is an integer and mapQ
reads the host-made log table: nothing is tolerated."""
import os

import numpy as np
import pytest

import chain_cases as cc
import common
import mark_cases as mc
from common import bw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(small_index, tmp_path_factory):
    c = bw.Context(cc.alt_index(small_index, tmp_path_factory.mktemp("mark_alt")))
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(common.GOLDEN, "kat_mark.npz"))


def answers(recs):
    reads = common.by_read(recs)
    return [r[bw.KAT_MARK_TAG] for r in reads]


def differing(got, want, cases):
    return [cases[i].name for i in range(len(want)) if not np.array_equal(got[i], want[i])]


@pytest.mark.parametrize("name", list(mc.SETS))
def test_set_equals_oracle_and_golden(ctx, gold, tmp_path, name):
    """Per set: with the selection (plan 1) every word of every read equals the oracle's; without (plan 0) the same with need, XA owner
    and the two counts zero; both equal the reference's digests on the reference's words."""
    s = mc.SETS[name]
    cases = mc.cases_of(name)
    assert str(gold[f"{name}.inputs"]) == mc.input_digest(name), "the case generator drifted: regenerate tests/golden/kat_mark.npz"
    want = mc.run_checker(common.ORACLE, name, str(tmp_path), "ora")
    off, regs = mc.pack(cases)
    opt = mc.opt_of(name)
    for plan in (1, 0):
        got = answers(ctx.kat_mark(off, regs, opt=opt, n_processed=s.n_processed, plan=plan))
        assert len(got) == len(want)
        bad = differing(got, want if plan else [mc.no_plan(w) for w in want], cases)
        assert not bad, f"{name} plan {plan}: {len(bad)} of {len(cases)} reads differ from the oracle, first {bad[:5]}"
        assert np.array_equal(mc.digests(got), gold[f"{name}.sha"]), f"{name} plan {plan}: differs from the reference's records"


@pytest.mark.parametrize("name", ["sizes_pe", "position_np1t_pe", "five_pe", "random_a5"])
@pytest.mark.parametrize("plan", [0, 1])
def test_two_launches_equal_one(ctx, name, plan):
    """The paired-end path marks a batch in two launches: every pair but the listed ones (one workgroup per read, the listed pairs leave at
    once), then the listed pairs (one workgroup per listed pair end).  With every third pair listed -- and with none, and with all -- the
    batch must come back exactly as from one launch."""
    s = mc.SETS[name]
    cases = mc.cases_of(name)
    off, regs = mc.pack(cases)
    opt = mc.opt_of(name)
    n_pairs = len(cases) // 2
    one = answers(ctx.kat_mark(off, regs, opt=opt, n_processed=s.n_processed, plan=plan))
    for listed in (list(range(0, n_pairs, 3)), list(range(n_pairs - 1, -1, -1)), []):
        two = answers(ctx.kat_mark(off, regs, opt=opt, n_processed=s.n_processed, plan=plan, pairs=listed))
        bad = differing(two, one, cases)
        assert not bad, f"{name} plan {plan}, {len(listed)} pairs listed: {len(bad)} reads differ, first {bad[:5]}"


def test_empty_batch_and_bad_input(ctx):
    """n_reads == 0 launches nothing; offsets that descend, qe < qb, re < rb, a contig outside the index, an odd batch with the paired
    flag or a pair list, a pair index out of range or given twice are refused."""
    assert ctx.kat_mark([0], np.zeros((0, 19))) == []
    ok = mc.reg(0, 100, 90)
    assert len(answers(ctx.kat_mark([0, 1], [ok]))) == 1

    def with_(col, v):
        r = list(ok)
        r[col] = v
        return r
    pe = bw.default_opt()
    pe.flag |= 0x2
    for off, regs, kw in (([0, 2, 1], [ok, ok], {}), ([1, 2], [ok, ok], {}), ([0, 1], [with_(3, -1)], {}), ([0, 1], [with_(1, ok[0] - 1)], {}),
                          ([0, 1], [with_(4, 3)], {}), ([0, 1], [with_(4, -1)], {}), ([0, 1], [ok], dict(opt=pe)), ([0, 1], [ok], dict(pairs=[])),
                          ([0, 1, 2], [ok, ok], dict(pairs=[1])), ([0, 1, 2], [ok, ok], dict(pairs=[-1])), ([0, 1, 2, 3, 4], [ok] * 4, dict(pairs=[1, 1])),
                          ([0, 1], [ok], dict(plan=2))):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.kat_mark(off, regs, **kw)
    assert len(answers(ctx.kat_mark([0, 1, 2], [ok, ok], opt=pe, pairs=[0]))) == 2


def test_span_beyond_the_log_table_is_reported(ctx):
    """A region whose span needs log() beyond the host-made table comes back with bad = 1 and mapQ 0 -- the output path reports an error
    for it --; its neighbour in the list is answered as usual."""
    c = mc.bad_case()
    (rec,) = answers(ctx.kat_mark([0, len(c.regs)], c.regs))
    b = mc.body(rec)
    assert [int(x) for x in b[:, mc.C_IN]] == [0, 1] and [int(x) for x in b[:, mc.C_BAD]] == [1, 0]
    assert b[0, mc.C_MAPQ] == 0 and b[1, mc.C_MAPQ] > 0
