"""Known answers for chaining and the chain filter: the kernels of csrc/k_chain.hip (one read per lane; a wavefront per read with the B-tree in
14 / 77 / 150 KB of LDS or in global memory, and its help-out loop; the sequential and the wavefront overlap filter) fed seed lists
directly through bwahip_kat_chain -- the stage chain's own buffers, sizes and launches -- against ora_kat_chain (`bwa_oracle katchain`),
which tests/test_chain_cases_cpu.py pins to the reference's kbtree / test_and_merge / mem_chain_flt, and against the reference-made
tests/golden/kat_chain.npz.  Per set of tests/chain_cases.py and per knob setting: the chains before the filter (w / kept / first masked,
as everywhere) and the filtered chains bit for bit, and the kernels' per-read diagnostics equal to the model's: who took the read, B-tree
nodes used, tree height, which sort and which filter ran."""
import os

import numpy as np
import pytest

import chain_cases as cc
import common
from common import bw
from test_gpu_stages import KNOB_DEFAULTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def alt(small_index, tmp_path_factory):
    return cc.alt_index(small_index, tmp_path_factory.mktemp("chain_alt"))


@pytest.fixture(scope="module")
def ctx(alt):
    c = bw.Context(alt)
    yield c
    c.close()


@pytest.fixture
def tuned(ctx):
    yield ctx.tune
    ctx.tune(**KNOB_DEFAULTS)


def run_set(ctx, tune, alt, name, workdir, helped_ok=False):
    """One set under each of its knob settings -> {setting: diag}, after asserting records and diagnostics."""
    flags, _, settings, core = cc.SETS[name]
    cases = cc.cases_of(name)
    want_reads, stats = cc.run_checker(common.ORACLE, alt, cases, flags, str(workdir), name)
    want = cc.masked(want_reads)
    opt, _ = common.opt_from_cli(flags)
    gold = np.load(os.path.join(common.GOLDEN, "kat_chain.npz")) if core else None
    if core:
        assert str(gold[f"{name}.inputs"]) == cc.input_digest(cases), "the case generator drifted: regenerate tests/golden/kat_chain.npz"
    out = {}
    for label, knobs in settings.items():
        tune(**KNOB_DEFAULTS)
        tune(**knobs)
        recs, diag = ctx.kat_chain(*cc.pack(cases), opt=opt)
        got_reads = common.by_read(recs)
        got = cc.masked(got_reads)
        common.assert_stage_equal(got, want, bw.STAGE_CHAIN, f"{name}[{label}]: chains")
        common.assert_stage_equal(got, want, bw.STAGE_CHAIN_FLT, f"{name}[{label}]: filtered chains")
        if core:
            assert np.array_equal(cc.digests(got_reads), gold[f"{name}.sha"]), f"{name}[{label}]: differs from the reference's records"
        for i, c in enumerate(cases):
            taker = cc.expected_taker(len(c.seeds), knobs)
            exp = cc.expected_diag(c, want_reads[i], stats[i], taker, opt.min_chain_weight)
            d = [int(x) for x in diag[i, :6]]
            if helped_ok and d[0] == bw.CHAIN_BY_HELPED and taker in (1, 2):
                exp[0] = bw.CHAIN_BY_HELPED
            assert d == exp and not diag[i, 6:].any(), f"{name}[{label}] {c.name}: diagnostics {d}, the model's {exp}"
        assert not (diag[:, 3] == bw.CHAIN_SORT_LANE_AREA).any()    # unreachable (test_chain_cases_cpu.test_sort_area_always_fits)
        out[label] = diag
    return out


@pytest.mark.parametrize("name", cc.FAMILIES["merge"])
def test_merge_rule(ctx, tuned, alt, tmp_path, name):
    """test_and_merge on either side of each inequality, contained seeds, other contig, no contig, the strand rule; also under -w 1, -w 300, -G 50."""
    run_set(ctx, tuned, alt, name, tmp_path)


def test_tree_shape(ctx, tuned, alt, tmp_path):
    """11 .. 3201 chains in four insertion orders with 0, 2 and 12 chains of equal pos: every split of leaf, internal node and root up to
    height 5, in the lane kernel, in each LDS class at its last size and in global memory at the first size beyond."""
    diags = run_set(ctx, tuned, alt, "tree", tmp_path)
    assert set(diags["shipped"][:, 0]) == {bw.CHAIN_BY_LANE, 1, 2, 3} and set(diags["all"][:, 0]) == {0, 1, 2, 3} and set(diags["off"][:, 0]) == {bw.CHAIN_BY_LANE}
    assert set(diags["all"][:, 2]) >= {2, 3, 4, 5}
    n = np.array([len(c.seeds) for c in cc.cases_of("tree")])
    for size, cls in ((256, 0), (257, 1), (1536, 1), (1537, 2), (3200, 2), (3201, 3)):
        assert set(diags["all"][n == size, 0]) == {cls}


def test_sort_by_weight(ctx, tuned, alt, tmp_path):
    """1 .. 255 chains of equal, two-valued, rising and falling weights, and sorted weights with ties: k_chain's introsort, the wavefront's
    exact sort, and its hand-over to one lane at the introsort's depth limit must each have run, with the reference's order among ties."""
    diags = run_set(ctx, tuned, alt, "sort", tmp_path)
    assert set(diags["shipped"][:, 3]) >= {bw.CHAIN_SORT_NONE, bw.CHAIN_SORT_LANE}                          # (the 600 chains: class 1 as shipped)
    assert set(diags["all"][:, 3]) == {bw.CHAIN_SORT_NONE, bw.CHAIN_SORT_WAVE, bw.CHAIN_SORT_LANE_DEPTH}
    deep = [c.name for c, d in zip(cc.cases_of("sort"), diags["all"]) if d[3] == bw.CHAIN_SORT_LANE_DEPTH]
    assert any(nm.endswith(".depth") for nm in deep), deep


@pytest.mark.parametrize("name", cc.FAMILIES["filter"])
def test_overlap_filter(ctx, tuned, alt, tmp_path, name):
    """mem_chain_flt at each threshold (mask_level, drop_ratio, 2 x min_seed_len, max_chain_gap), ALT against primary, `first`, 32 against 33
    chains, kept lists around 64 and 128 with the shadowing chain at index 0, 63, 64 and last; under -G 50, -D 0.1 / 0.9, -W 40, -N 1 / 2 / 5.
    Both filters must have run."""
    diags = run_set(ctx, tuned, alt, name, tmp_path)
    for d in diags.values():
        assert set(d[:, 4]) >= {bw.CHAIN_FLT_SEQ, bw.CHAIN_FLT_WAVE}
    if name in ("filter", "filter_W40"):
        by = {c.name: d for c, d in zip(cc.cases_of(name), diags["all"])}
        which = "count" if name == "filter" else "survive"
        assert by[f"flt.{which}32"][4] == bw.CHAIN_FLT_SEQ and by[f"flt.{which}33"][4] == bw.CHAIN_FLT_WAVE


def test_every_class_gives_the_same_chains(ctx, tuned, alt, tmp_path):
    """The same reads of 0 .. 700 seeds in the lane kernel, in class 0 / 1, and -- with the class bounds drawn in to 257 / 258 seeds -- in
    class 2 and 3: identical records (each setting is compared with the one oracle run), and the class the setting asks for."""
    diags = run_set(ctx, tuned, alt, "classes", tmp_path)
    sizes = [len(c.seeds) for c in cc.cases_of("classes")]
    assert [int(diags["narrow"][sizes.index(s), 0]) for s in (256, 257, 258, 259)] == [0, 1, 2, 3]
    assert set(diags["narrow"][:, 0]) == {bw.CHAIN_BY_LANE, 0, 1, 2, 3} and set(diags["off"][:, 0]) == {bw.CHAIN_BY_LANE}


def test_random_reads(ctx, tuned, alt, tmp_path):
    """400 seeded reads of 1 .. 400 seeds in which seeds merge, open chains and meet chains of equal pos."""
    run_set(ctx, tuned, alt, "random", tmp_path)


@pytest.mark.parametrize("name,cls,setting", [("flood1", 1, "all"), ("flood2", 2, "narrow_mid")])
def test_flood_switches_the_help_out_loop_on(ctx, tuned, alt, tmp_path, name, cls, setting):
    """More reads of one LDS class than its kernel takes in two rounds (2049 of class 1; 513 of class 2): the workgroups of the global-node
    kernel empty the queue together with the LDS kernel, running LDS-class reads on global nodes with the sort area in the filter's scratch."""
    diag = run_set(ctx, tuned, alt, name, tmp_path, helped_ok=True)[setting]
    assert set(diag[:, 0]) <= {cls, bw.CHAIN_BY_HELPED}
    helped = int((diag[:, 0] == bw.CHAIN_BY_HELPED).sum())
    print(f"{name}: {helped} of {len(diag)} reads taken by the help-out loop")
    if helped == 0:
        pytest.skip("parity holds, but scheduling gave the help-out loop no read on this run")


def test_empty_batch_and_bad_input(ctx):
    """n_reads == 0 launches nothing; offsets that descend, a seed outside its read or the reference, a contig that does not exist are refused."""
    recs, diag = ctx.kat_chain([], [0], np.zeros((0, 4)), [0], np.zeros((0, 3)))
    assert recs == [] and diag.shape == (0, bw.CHAIN_DIAG_N)
    ok = [[5000, 10, 20, 0]]
    for read_len, seed_off, seeds in (([700], [0, 1], [[5000, 690, 20, 0]]), ([700], [0, 1], [[2 * cc.L_PAC - 5, 10, 20, 0]]), ([700], [0, 1], [[5000, 10, 20, 3]]),
                                      ([700], [0, 1], [[5000, 10, 0, 0]]), ([700, 700], [0, 1, 0], ok), ([0], [0, 1], ok)):
        with pytest.raises(bw.BwahipError, match="EINVAL"):
            ctx.kat_chain(read_len, seed_off, seeds, [0] * len(seed_off), np.zeros((0, 3)))
    recs, diag = ctx.kat_chain([700], [0, 1], ok, [0, 0], np.zeros((0, 3)))
    assert int(common.by_read(recs)[0][bw.STAGE_CHAIN_FLT][0]) == 1 and diag[0, 0] == bw.CHAIN_BY_LANE
