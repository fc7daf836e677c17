"""The list update of mate rescue on the device (csrc/k_pair.hip: ms_list_add / ms_list_close -- the functions k_matesw calls -- with
incr_insert and sort_dedup_nopatch behind them), fed lists directly through bwahip_kat_mate_insert, against ora_sort_dedup_patch applied
as ora_matesw applies it (oracle/ora_pair.c: ora_kat_mate_insert).  Per set of tests/mate_insert_cases.py: the device as shipped
(mode 0), the device never incremental (mode 1), both again with the lists in global memory, each equal to the oracle in every word of
every region but n_comp and secondary; the step counts the device returns must be the ones the Python model predicts, so that every
class provably took the path it was built for.  tests/test_mate_insert_cases_cpu.py checks the cases themselves without a GPU."""
import numpy as np
import pytest
import common
import mate_insert_cases as mc
from common import bw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


_ref = {}
def reference(name):
    """Items, packed arrays, the oracle's lists and the predicted counts of a set; computed once, shared, left unchanged."""
    if name not in _ref:
        if name == "random":
            gap, mlr, items = 10_000, 0.95, mc.random_items()
            want_cnt = None                                          # per item only with the model (CPU test); the totals are mc.RANDOM_COUNTS
        else:
            gap, mlr, build = mc.SETS[name]
            items = build()
            want_cnt = np.array([mc.counts_of(mc.predict(it, gap, mlr, check_model=False)[0]) for it in items], dtype=np.int32).reshape(-1, 3)
        _ref[name] = dict(gap=gap, mlr=mlr, items=items, packed=mc.pack(items), want=[mc.mask(w) for w in mc.oracle_lists(items, gap, mlr)], want_cnt=want_cnt)
    return _ref[name]


def run(ctx, R, mode, where):
    opt = bw.default_opt()
    opt.max_chain_gap = R["gap"]; opt.mask_level_redun = R["mlr"]
    list_off, lw, step_off, sh, sw = R["packed"]
    out, out_n, cnt = ctx.kat_mate_insert(list_off, lw, step_off, sh, sw, opt, mode=mode, where=where)
    base = list_off + step_off
    what = f"mode {mode} where {where}"
    for i, it in enumerate(R["items"]):
        got = mc.mask(out[base[i]:base[i] + out_n[i]])
        want = R["want"][i]
        if got.shape != want.shape or not np.array_equal(got, want):
            bad = next((k for k in range(min(len(got), len(want))) if not np.array_equal(got[k], want[k])), min(len(got), len(want)))
            raise AssertionError(f"{it.name} ({what}): {len(got)} regions, oracle {len(want)}; first difference at {bad}: got {got[bad].tolist() if bad < len(got) else None}, "
                                 f"want {want[bad].tolist() if bad < len(want) else None}; counts {cnt[i].tolist()}")
    return cnt


@pytest.mark.parametrize("name", list(mc.SETS) + ["random"])
def test_device_list_update_equals_oracle(ctx, name):
    R = reference(name)
    items = R["items"]
    n_hits = np.array([int(it.hits().sum()) for it in items]); n_steps = np.array([len(it.steps) for it in items])
    for where in (0, 1):
        cnt = run(ctx, R, 0, where)                                   # as shipped
        print(name, "where", where, "by incr_insert, by score, full passes:", cnt.sum(axis=0).tolist())
        assert np.array_equal(cnt[:, 0] + cnt[:, 1], n_hits)
        if R["want_cnt"] is not None:
            bad = [(it.name, cnt[i].tolist(), R["want_cnt"][i].tolist()) for i, it in enumerate(items) if not np.array_equal(cnt[i], R["want_cnt"][i])]
            assert not bad, f"{name} (where {where}): steps took another path than the model predicts (got, want): {bad[:5]}"
        else:
            # the seed's counts by the model (mate_insert_cases.RANDOM_COUNTS = 12 851 incremental, 3 397 by score, 3 610 full passes): both paths ran
            assert tuple(int(x) for x in cnt.sum(axis=0)) == mc.RANDOM_COUNTS
            assert cnt[:, 0].sum() > 10_000 and cnt[:, 1].sum() > 500
        cnt1 = run(ctx, R, 1, where)                                  # never incremental: every step through the general path
        assert not cnt1[:, 0].any() and np.array_equal(cnt1[:, 1], n_hits) and np.array_equal(cnt1[:, 2], n_steps)
    if name == "reach":                                             # 65 within reach: refused, and the general count rose
        for i, it in enumerate(items):
            if it.name.startswith("reach65"): assert R["want_cnt"][i][1] == 1 and R["want_cnt"][i][2] == 2
    if name == "sizes":
        caps = [it.cap for it in items]
        assert max(c for c in caps if c <= mc.MS_LIST) == mc.MS_LIST and max(caps) > 1000


def test_bad_arguments_are_refused(ctx):
    z = np.zeros((0, 19), dtype=np.int64)
    with pytest.raises(bw.BwahipError):                              # offsets that do not ascend
        ctx.kat_mate_insert(np.array([0, 2, 1]), np.zeros((2, 19), dtype=np.int64), np.array([0, 0, 0]), np.zeros(0, dtype=np.int32), z)
    with pytest.raises(bw.BwahipError):                              # a negative length
        ctx.kat_mate_insert(np.array([0, -1]), z, np.array([0, 0]), np.zeros(0, dtype=np.int32), z)
    with pytest.raises(bw.BwahipError):                              # steps whose offsets do not ascend
        ctx.kat_mate_insert(np.array([0, 0, 0]), z, np.array([0, 1, 0]), np.zeros(1, dtype=np.int32), np.zeros((1, 19), dtype=np.int64))
    out, out_n, cnt = ctx.kat_mate_insert(np.array([0]), z, np.array([0]), np.zeros(0, dtype=np.int32), z)   # no item: nothing launched
    assert len(out_n) == 0
