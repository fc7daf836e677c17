"""The early stop of ksw_extend2 ("ksw_extend2: rows that cannot matter") pinned without a GPU: tests/ext_early_stop_model.c
restates the reference's row loop with the rule, and must give the six results of liboracle.so's ora_ksw_extend2 -- score, qle, tle,
gtle, gscore, max_off -- on every case: seeded cases drawn as dp_kat.rand_case draws them (in C, so that a hundred thousand take
seconds), tandem-repeat queries, the benchmark's flank shape, and cases from dp_kat.rand_case itself.  Bit-exact: no tolerances."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import common
import dp_kat

HERE = os.path.dirname(os.path.abspath(__file__))
STATS = ["cases", "diff", "stopped", "prefilter_miss", "rows_full", "rows_rule", "first_diff", "gscore_neg_stopped", "evals"]
FAM_RANDOM, FAM_TANDEM, FAM_BENCH = 0, 1, 2


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ees") / "libees_model.so")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "ext_early_stop_model.c")], check=True)
    lib = C.CDLL(so)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    lib.ees_compare.restype = C.c_long
    lib.ees_compare.argtypes = [vp, C.c_uint64, C.c_long, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_long)]
    lib.ees_extend2.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 9 + [ip] * 8
    return lib


@pytest.fixture(scope="module")
def ora():
    return dp_kat.Oracle()


def _compare(model, ora, seed, n, family, every=1, want_rows=0, threads=4):
    """n cases in `threads` runs of their own seed; the summed counts"""
    fn = C.cast(ora.lib.ora_ksw_extend2, C.c_void_p)

    def one(k):
        st = (C.c_long * len(STATS))()
        model.ees_compare(fn, seed * 1000 + k, n // threads, family, every, want_rows, st)
        return dict(zip(STATS, st))
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, range(threads)))
    tot = {k: sum(p[k] for p in parts) for k in STATS}
    tot["first_diff"] = [(k, p["first_diff"]) for k, p in enumerate(parts) if p["first_diff"] >= 0]
    return tot


def test_random_cases_equal_the_oracle(model, ora):
    """88 000 cases over the matrices, gap sets, bands, z-drops, end bonuses and lengths of dp_kat (N's included, qlen up to 700) and
    12 000 tandem-repeat queries (period 1 to 6) against a longer repeat of the same unit."""
    rnd = _compare(model, ora, 11, 88000, FAM_RANDOM)
    tan = _compare(model, ora, 12, 12000, FAM_TANDEM)
    print(f"\nrandom {rnd}\ntandem {tan}")
    assert rnd["cases"] + tan["cases"] >= 100000
    for st in (rnd, tan):
        assert st["diff"] == 0, st
        assert st["prefilter_miss"] == 0, st                            # the kernels' scalar pre-filter never keeps out a test that would hold
        assert st["gscore_neg_stopped"] == 0, st
    assert rnd["stopped"] >= rnd["cases"] // 10 and tan["stopped"] >= tan["cases"] // 2   # (the rule is alive in both families)


@pytest.mark.parametrize("every", [1, 4, 8])
def test_benchmark_shape(model, ora, every):
    """The flanks of the benchmark's reads (3 to 102 bases, 1/-4, 6/1, w 100, z-drop 100, bonus 5, h0 19 to 147, tlen = qlen + max_gap,
    1 % substitutions, first base a mismatch): same results, nearly every call stops, about half the rows are left.  Tested after every
    row, every 4th and every 8th: testing less often is the same rule."""
    st = _compare(model, ora, 13, 20000, FAM_BENCH, every, want_rows=1)
    ratio = st["rows_rule"] / st["rows_full"]
    print(f"\nbenchmark shape, every {every}: {st}; rows {ratio:.3f} of the full loop, {st['evals'] / st['cases']:.2f} vector tests per call")
    assert st["diff"] == 0 and st["prefilter_miss"] == 0, st
    assert st["stopped"] >= 0.9 * st["cases"]
    assert ratio < 0.6
    if every == 1:
        assert st["evals"] <= 1.1 * st["cases"]                         # with the scalar pre-filter the vector part runs about once per call


def test_rand_case_of_dp_kat(model, ora):
    """Cases from dp_kat.rand_case itself (the generator the device tests use), one call each."""
    rng = np.random.default_rng(4242)
    stopped = 0
    for k in range(3000):
        c = dp_kat.rand_case(rng, "ext")
        o = [C.c_int() for _ in range(8)]
        sc = model.ees_extend2(c.qlen, c.q.ctypes.data, c.tlen, c.t.ctypes.data, 5, c.mat.ctypes.data, *c.gaps, c.w, c.bonus, c.zdrop, c.h0, 1,
                               *[C.byref(x) for x in o])
        assert [sc] + [x.value for x in o[:5]] == ora.extend(c), (k, c)
        assert not o[5].value & 2, (k, c)
        stopped += o[5].value & 1
    assert stopped >= 300
