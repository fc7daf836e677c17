"""k_smem's table jump ("k_smem: the short-string triangle skipped by table jumps"; knob smem_skip) against the oracle:
STAGE_INTV through ctx.run_stages, bit for bit, on the 1 Mbp index of the small_index fixture, whose table holds strings of up to 11
bases -- a depth of 11 falls back often there, a depth of 5 almost never.  tests/test_smem_skip_model.py pins the rule itself on the CPU.
The variants with more than one lane per read run plain under every smem_skip (k_smem.hip), which the counters show."""
import subprocess
import numpy as np
import pytest
import common
from common import bw

pytestmark = pytest.mark.gpu

DEPTHS = [0, 2, 5, 8, 11]


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    assert c.kat_kmer_table()[0] == 11
    yield c
    c.close()


@pytest.fixture
def tuned(ctx):
    yield ctx.tune
    ctx.tune(smem_skip=-1, smem_lanes=1, heavy_mult=-1)


def _short_reads(fa, path, n, seed):
    """n reads of 19 to 40 bases with 2 % N: 40-base reads cut to a seeded length"""
    bw.make_reads(fa, path + ".40", None, n, 40, 10000, 0, 20000, seed, 0)
    names, seqs, quals = bw.read_fastq(path + ".40")
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        for nm, s, q in zip(names, seqs, quals):
            ln = int(rng.integers(19, 41))
            f.write(b"@%s\n%s\n+\n%s\n" % (nm, s[:ln], q[:ln]))


@pytest.fixture(scope="module")
def read_sets(small_index, tmp_path_factory):
    """the three read sets, each with the oracle's stage records (made once, shared by every test)"""
    d = tmp_path_factory.mktemp("skip")
    fa, prefix = small_index["fa"], small_index["prefix"]
    sets = {}
    for name, make in (("se150", lambda p: bw.make_reads(fa, p, None, 2500, 150, 10000, 2000, 500, 131, 20000)),
                       ("short", lambda p: _short_reads(fa, p, 500, 132)),
                       ("se250", lambda p: bw.make_reads(fa, p, None, 1000, 250, 50000, 0, 0, 133, 0))):
        fq = str(d / f"{name}.fq")
        make(fq)
        _, seqs, _ = bw.read_fastq(fq)
        codes, off = bw.pack_reads(seqs)
        sets[name] = dict(fq=fq, codes=codes, off=off, n=len(seqs), want=common.by_read(common.oracle_stages(prefix, fq, str(d / f"{name}.bin"))))
    lens = np.diff(sets["short"]["off"])
    assert lens.min() == 19 and lens.max() == 40
    return sets


def _run(ctx, rs, what, opt=None, want=None):
    got = common.by_read(ctx.run_stages(rs["codes"], rs["off"], [bw.STAGE_INTV], opt))
    common.assert_stage_equal(got, want or rs["want"], bw.STAGE_INTV, what)
    return ctx.counters()


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", ["se150", "short", "se250"])
def test_intervals_at_every_depth(ctx, read_sets, tuned, name, depth):
    tuned(smem_skip=depth)
    cnt = _run(ctx, read_sets[name], f"intervals[{name}, smem_skip={depth}]")
    print(f"\n{name}, smem_skip {depth}: extend {cnt['extend']}, look-ups {cnt['smem_lookups']}, fallbacks {cnt['smem_fallbacks']}")
    if depth == 0:
        assert cnt["smem_lookups"] == 0 and cnt["smem_fallbacks"] == 0
    else:
        assert cnt["smem_lookups"] > 0
    if depth == 11:
        assert cnt["smem_fallbacks"] > 0
    if depth == 5:
        assert cnt["smem_fallbacks"] * 100 < cnt["smem_lookups"]


def test_default_depth_is_8_on_this_index(ctx, read_sets, tuned):
    """-1 derives the depth from the text: 4^8 <= 2 Mbp / 16 < 4^9.  The same reads must take the same turns as under smem_skip = 8."""
    tuned(smem_skip=-1)
    auto = _run(ctx, read_sets["se150"], "intervals[default]")
    tuned(smem_skip=8)
    eight = _run(ctx, read_sets["se150"], "intervals[8]")
    assert auto["smem_lookups"] == eight["smem_lookups"] > 0 and auto["extend"] == eight["extend"]
    tuned(smem_skip=0)
    plain = _run(ctx, read_sets["se150"], "intervals[0]")
    print(f"\nextend {plain['extend']} plain -> {eight['extend']} + {eight['smem_lookups']} look-ups at depth 8")
    assert eight["extend"] + eight["smem_lookups"] < plain["extend"]      # the skip saves turns (the CPU model says how many)


@pytest.mark.parametrize("depth", [8, 11])
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_every_lanes_variant(ctx, read_sets, tuned, lanes, depth):
    tuned(smem_skip=depth, smem_lanes=lanes)
    cnt = _run(ctx, read_sets["se150"], f"intervals[lanes={lanes}, smem_skip={depth}]")
    assert (cnt["smem_lookups"] > 0) == (lanes == 1)        # more than one lane per read: plain


@pytest.mark.parametrize("depth", [-1, 11])
def test_heavy_hand_off_with_look_ups_counted(ctx, read_sets, tuned, depth):
    """heavy_mult 2: most reads pass 2 x len turns -- look-ups count as turns -- and go to k_smem_heavy, abandoned calls and all"""
    tuned(smem_skip=depth, heavy_mult=2)
    for name in ("se150", "se250"):
        cnt = _run(ctx, read_sets[name], f"intervals[{name}, heavy_mult=2, smem_skip={depth}]")
        assert cnt["heavy_intv"] > 0 and cnt["smem_lookups"] > 0


def test_min_seed_len_below_the_depth(ctx, small_index, read_sets, tuned, tmp_path):
    """-k 10 under smem_skip = 11: the depth is clamped to 10, so no dormant entry can end a kept seed"""
    tuned(smem_skip=11)
    opt, _ = common.opt_from_cli(["-k", "10"])
    for name in ("se150", "short"):
        rs = read_sets[name]
        obin = str(tmp_path / f"{name}_k10.bin")
        subprocess.check_call([common.ORACLE, "stages", "-k", "10", small_index["prefix"], rs["fq"], obin])
        want = common.by_read(bw.read_record_file(obin))
        cnt = _run(ctx, rs, f"intervals[{name}, -k 10, smem_skip=11]", opt, want)
        assert cnt["smem_lookups"] > 0


def test_sam_text_same_with_and_without(ctx, small_index, tuned, tmp_path):
    fa = small_index["fa"]
    pe1, pe2 = str(tmp_path / "p_1.fq"), str(tmp_path / "p_2.fq")
    bw.make_reads(fa, pe1, pe2, 800, 150, 10000, 2000, 500, 134, 20000)
    opt = bw.default_opt()
    opt.flag |= 0x2
    sams = {}
    for depth in (-1, 0):
        tuned(smem_skip=depth)
        with bw.FastqReader(pe1, pe2) as rd:
            arr, n = rd.next(10 ** 9)
            assert n == 800
            sams[depth] = ctx.process_seqs_text_array(arr, n, opt)
    assert len(sams[0]) > 800 * 100 and sams[-1] == sams[0]


def test_empty_batch_and_bad_value(ctx, tuned):
    tuned(smem_skip=11)
    assert ctx.run_stages(np.zeros(0, np.uint8), np.zeros(1, np.int64), [bw.STAGE_INTV]) == []
    for bad in (1, -2):
        with pytest.raises(bw.BwahipError):
            ctx.tune(smem_skip=bad)
