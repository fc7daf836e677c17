"""The cases of tests/mate_insert_cases.py checked before a GPU sees them: every item is replayed through the oracle's helper
(ora_kat_mate_insert) step by step and through the Python model of tests/test_incr_insert_model.py; the reason each item was built for
must hold on the oracle's lists, the model's refusals must be where the builder says they are, and wherever the model accepts a step its
list must be the oracle's.  A wrong case builder fails here."""
import pytest
import mate_insert_cases as mc


@pytest.mark.parametrize("name", list(mc.SETS))
def test_built_cases_hold_their_reasons(name):
    gap, mlr, build = mc.SETS[name]
    items = build()
    assert items and len(set(it.name for it in items)) == len(items)
    whole = mc.oracle_lists(items, gap, mlr)
    seen = set()
    for it, w in zip(items, whole):
        paths, lists = mc.predict(it, gap, mlr)
        mc.check_reason(it, paths, lists)
        assert mc._dicts(w) == lists[-1], (it.name, "step by step and in one call differ")
        seen.update(paths)
        assert it.cap == len(it.start) + len(it.steps)
    if name in ("sizes", "state"):
        assert seen == {"incr", "score", "none", "none+full"}, seen


def test_sizes_cover_both_address_spaces_and_the_edges():
    items = mc.size_items()
    caps = sorted(it.cap for it in items)
    assert mc.MS_LIST in caps and caps[0] < 64 and any(c > mc.MS_LIST for c in caps)
    starts = set(len(it.start) for it in items)
    assert {0, 1, 2, 63, 64, 65, 128, 223, 224, 225, 1000} <= starts


def test_random_sequences_reach_both_paths_and_the_model_agrees_with_the_oracle():
    """The floors that tests/test_gpu_mate_insert.py asserts on the device's counts come from here."""
    items = mc.random_items()
    n = [0, 0, 0]
    big = 0
    for it in items:
        paths, _ = mc.predict(it, 10_000, 0.95)
        c = mc.counts_of(paths)
        for k in range(3): n[k] += c[k]
        big += it.cap > mc.MS_LIST
    print("random sequences: by incr_insert, by score, full passes:", n, "items beyond the LDS list:", big)
    assert (n[0], n[1], n[2]) == mc.RANDOM_COUNTS, n
    assert n[0] > 5000 and n[1] > 500 and big >= 20
