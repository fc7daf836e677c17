"""The diagonal rule of ksw_extend2 ("ksw_extend2: flanks the diagonal answers") pinned without a GPU: tests/ext_diag_model.c
states it as a predicate plus the six results it writes down -- score, qle, tle, gtle, gscore, max_off -- and liboracle.so's
ora_ksw_extend2 is the judge wherever the predicate holds.  Seeded cases drawn in C (a quarter of a million take seconds): the grids of
dp_kat, tandem repeats, shifted copies, the benchmark's flank shape, and the edge families -- those that must be refused are refused in
every case.  Bit-exact: no tolerances."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import dp_kat

HERE = os.path.dirname(os.path.abspath(__file__))
STATS = ["cases", "holds", "diff", "first_diff"]
FAMILIES = {"grid": 0, "tandem": 1, "shift": 2, "bench": 3, "qlen 1-8": 4, "mismatch at an end": 5, "no mismatch": 6, "tlen = qlen": 7,
            "tlen = qlen - 1": 8, "h0 <= b": 9, "0 < zdrop < b": 10, "g <= a + b": 11, "an N": 12}
MUST_REFUSE = ["tlen = qlen - 1", "h0 <= b", "0 < zdrop < b", "g <= a + b", "an N"]


def build_model(tmpdir):
    so = os.path.join(str(tmpdir), "libedg_model.so")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "ext_diag_model.c")], check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.edg_compare.restype = C.c_long
    lib.edg_compare.argtypes = [vp, C.c_uint64, C.c_long, C.c_int, C.POINTER(C.c_long)]
    lib.edg_rule.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 8 + [C.POINTER(C.c_int)]
    return lib


def rule(lib, c):
    """the six results the rule writes down for a dp_kat.Case, or None where it does not apply"""
    out = (C.c_int * 6)()
    ok = lib.edg_rule(c.qlen, c.q.ctypes.data, c.tlen, c.t.ctypes.data, 5, c.mat.ctypes.data, *c.gaps, c.w, c.bonus, c.zdrop, c.h0, out)
    return list(out) if ok else None


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return build_model(tmp_path_factory.mktemp("edg"))


@pytest.fixture(scope="module")
def ora():
    return dp_kat.Oracle()


def _compare(model, ora, seed, n, family, threads=4):
    fn = C.cast(ora.lib.ora_ksw_extend2, C.c_void_p)

    def one(k):
        st = (C.c_long * len(STATS))()
        model.edg_compare(fn, seed * 1000 + k, n // threads, FAMILIES[family], st)
        return dict(zip(STATS, st))
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, range(threads)))
    tot = {k: sum(p[k] for p in parts) for k in STATS}
    tot["first_diff"] = [(k, p["first_diff"]) for k, p in enumerate(parts) if p["first_diff"] >= 0]
    return tot


@pytest.fixture(scope="module")
def runs(model, ora):
    """every family once: 252 000 calls"""
    sizes = {"grid": 80000, "tandem": 40000, "shift": 40000, "bench": 20000}
    return {fam: _compare(model, ora, 31 + k, sizes.get(fam, 8000), fam) for k, fam in enumerate(FAMILIES)}


def test_no_difference_where_the_predicate_holds(runs):
    for fam, st in runs.items():
        print(f"\n{fam}: {st}")
    assert sum(st["cases"] for st in runs.values()) >= 200000
    for fam, st in runs.items():
        assert st["diff"] == 0, (fam, st)
    for fam in ("grid", "tandem", "shift", "qlen 1-8", "mismatch at an end", "no mismatch", "tlen = qlen"):
        assert runs[fam]["holds"] >= runs[fam]["cases"] // 10, (fam, runs[fam])   # (the rule is alive in the family: not vacuous)


def test_edge_families_that_must_refuse(runs):
    for fam in MUST_REFUSE:
        assert runs[fam]["cases"] >= 8000 and runs[fam]["holds"] == 0, (fam, runs[fam])


def test_benchmark_shape_holds_in_half_the_calls(runs):
    """qlen uniform on 3 to 102, the first base a mismatch, 1 % substitutions after it: the rule holds when no other base differs, the mean
    of 0.99^(qlen - 1) = 0.62 of the calls."""
    st = runs["bench"]
    print(f"\nbenchmark shape: {st}; holds in {st['holds'] / st['cases']:.3f}")
    assert st["holds"] >= st["cases"] // 2


def test_rand_case_of_dp_kat(model, ora):
    """Cases from dp_kat.rand_case itself (the generator the device tests use) with few enough errors for the rule to meet them."""
    rng = np.random.default_rng(4343)
    held = 0
    for k in range(3000):
        c = dp_kat.rand_case(rng, "ext", qlen=int(rng.integers(1, 120)), err=0.01, max_n=0.01)
        r = rule(model, c)
        if r is not None:
            held += 1
            assert r == ora.extend(c), (k, c)
    assert held >= 100
