"""Duplicate marking without a device: the host restatement of the decision (csrc/markdup_host.cpp) against the Python judge
(tests/markdup_ref.py) on every synthetic descriptor set, the end word at its corners, the HBM accounting and the descriptor's layout."""
import ctypes as C

import numpy as np
import pytest

import markdup_cases as cases
import markdup_ref as ref
from common import bw


@pytest.fixture(scope="module")
def sets(built):
    s = cases.desc_sets()
    cases.assert_desc_families(s)
    return s


def test_record_sets_hold_every_family():
    for paired in (False, True):
        cases.assert_record_families(cases.record_set(paired))


def test_decide_host_equals_the_judge(sets):
    for name, descs in sets.items():
        want, _ = ref.decide(descs)
        got = bw.markdup_decide_host(cases.as_desc_array(descs))
        assert got.tolist() == want, name
    bad = cases.as_desc_array([(1, 2, 3, 3)])                         # a kind that does not exist
    with pytest.raises(bw.BwahipError, match="EINVAL"):
        bw.markdup_decide_host(bad)


def test_end_word_at_the_corners(built):
    for ref_id in (0, 1, 2 ** 31 - 1):
        for u5 in (-2 ** 31, -1, 0, 1, 2 ** 31 - 1):
            for rev in (0, 1):
                want = ref_id << 33 | (u5 + 2 ** 31) << 1 | rev
                assert want < 2 ** 64 and bw.dup_end_word(ref_id, u5, rev) == want == ref.end_word(ref_id, u5, rev), (ref_id, u5, rev)
    assert bw.dup_end_word(0, -2 ** 31, 0) == 0 and bw.dup_end_word(2 ** 31 - 1, 2 ** 31 - 1, 1) == 2 ** 64 - 2 ** 33 + 2 ** 33 - 1


def test_hbm_need(built):
    need = bw.bam_devmerge_markdup_hbm_need
    for n_rec, n_tmpl in ((0, 0), (1, 1), (4300, 2150), (4_000_000, 2_000_000), (2 ** 31 - 1, 2 ** 30 - 1)):
        runs, work = 4 * n_rec + 24 * n_tmpl, 115 * n_tmpl + 4096
        assert need(n_rec, n_tmpl) == runs + work + work // 8
    assert need(-1, 0) == -1 and need(0, -1) == -1 and need(-5, -5) == -1
    assert need(10, 5) < need(11, 5) < need(11, 6)


def test_descriptor_layout(built):
    assert C.sizeof(bw.DupDesc) == 24 and bw.DUP_DESC_DTYPE.itemsize == 24 and cases.DESC_DTYPE == bw.DUP_DESC_DTYPE
    assert (bw.DupDesc.end.offset, bw.DupDesc.score.offset, bw.DupDesc.kind.offset) == (0, 16, 20) and C.sizeof(C.c_uint64) == 8
    assert [bw.DUP_DESC_DTYPE.fields[k][1] for k in ("end", "score", "kind")] == [0, 16, 20]
    # the library's own view of the layout: a fragment at the second slot of an array must be read where Python wrote it
    a = cases.as_desc_array([(5, 9, 1, 2), (5, 0, 7, 1), (9, 0, 7, 1), (77, 0, 7, 1)])
    assert bw.markdup_decide_host(a).tolist() == [0, 1, 1, 0]
    assert np.frombuffer(a.tobytes(), dtype=np.uint64)[[0, 1, 3, 4]].tolist() == [5, 9, 5, 0]      # offsets 0 and 8 of records 0 and 1
