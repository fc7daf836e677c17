"""GPU known-answer tests of every device form of the two DPs that decide each score and CIGAR: ksw_global2 with CIGAR through reg2aln's
own code (band forms of at most 64 and of 65 to 128 diagonals on the global slab and on the big slab, the row-wise form at 1, 2, 3, 4 and
11 columns per lane, the wavefront backtrack) and score-only at 3, 4, 5 and 11 columns per lane; ksw_extend2 plain and windowed at 3, 4, 5
and 11 columns per lane, both strides.  Expected values: the reference-made records of tests/golden (kat_ksw.npz, kat_dp_wide.npz) and
liboracle.so, which was compared with the reference's ksw.c over this whole range (test_oracle_vs_ref.py::test_dp_random_vs_reference).
Bit-exact: no tolerances."""
import numpy as np
import pytest
import dp_kat
from dp_kat import Case, scmat, rand_case, rand_query
from common import bw

pytestmark = pytest.mark.gpu

EDGE_QLEN = [1, 2, 63, 64, 65, 127, 128, 191, 192, 255, 256, 700]


@pytest.fixture(scope="module")
def ctx(small_index):
    c = bw.Context(small_index["prefix"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def ora():
    return dp_kat.Oracle()


def _diff(got, want, cases, what):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{what}: {len(bad)} of {len(want)} differ; first {bad[0]}: {cases[bad[0]]}\n got  {got[bad[0]][:24]}\n want {want[bad[0]][:24]}"


def _fit(ans):
    """what the device reports for an answer: the CIGAR staging holds KAT_MAX_CIGAR operations"""
    return ans if ans[1] <= bw.KAT_MAX_CIGAR else [0, -1]


def _check_global(ctx, cases, want, want_rev, what):
    """auto_big and auto_small, forward and reversed; auto_small must decline bands of more than 128 diagonals"""
    small = [2 * c.w + 1 <= 128 for c in cases]
    for rev, ans in ((0, want), (1, want_rev)):
        _diff(dp_kat.device_global(ctx, cases, bw.KAT_GLOBAL_AUTO_BIG, rev), [_fit(a) for a in ans], cases, f"{what} auto_big reverse={rev}")
        _diff(dp_kat.device_global(ctx, cases, bw.KAT_GLOBAL_AUTO_SMALL, rev), [_fit(a) if s else [0, -1] for a, s in zip(ans, small)], cases,
              f"{what} auto_small reverse={rev}")


# ---------------------------------------------------------------------------------------------------------------- ksw_global2
def test_global_fixture(ctx, ora):
    """Every reference-made ksw_global2 record.  For the reversed call the judge is the oracle on the reversed strings fed forward (what reg2aln
    relies on for a reverse-strand hit); that the oracle reproduces the records themselves is test_oracle_golden.py's."""
    cases = dp_kat.load_records("kat_dp_wide.npz")[1] + dp_kat.load_records("kat_ksw.npz")[1]
    assert len(cases) >= 420
    want = [c.res for c in cases]
    _check_global(ctx, cases, want, [ora.global2(c.reversed()) for c in cases], "fixture")


def _indel_family(rng):
    """A single insertion or deletion of 1, 40 and w - 3 bases at the first column, at the last column and 64 and 128 columns from the end: the gap
    state is entered on lane 0 and lane 63 of a backtrack step, and the CIGAR begins or ends with a gap operation."""
    out = []
    for w in (45, 63, 100):
        for g in (1, 40, w - 3):
            for L in (150, 320):
                for where in ("first", "last", "end-64", "end-128"):
                    for kind in ("del", "ins"):
                        q = rand_query(rng, L)
                        p = {"first": 0, "last": L, "end-64": L - 64, "end-128": L - 128}[where]
                        if kind == "del":                               # bases the query lacks
                            t = np.concatenate([q[:p], rand_query(rng, g), q[p:]])
                        else:                                           # bases the target lacks
                            p = min(p, L - g)
                            t = np.concatenate([q[:p], q[p + g:]])
                        out.append(Case("glb", q, t, w, dp_kat.GAPS[0] if rng.random() < 0.7 else dp_kat.GAPS[rng.integers(0, 5)], scmat(1, 4), fam="indel"))
    return out


@pytest.fixture(scope="module")
def glb_items(ora):
    rng = np.random.default_rng(20261)
    items = [rand_case(rng, "glb") for _ in range(1800)]
    for w in (31, 32, 63, 64):                                          # 2w + 1 = 63, 65, 127, 129: each side of both form boundaries
        for _ in range(60):
            qlen = int(rng.integers(w + 1, 701))
            items.append(rand_case(rng, "glb", qlen=qlen, w=w, tlen=max(1, qlen + int(rng.integers(-(w - 3), w - 2))), fam="boundary"))
    for qlen in EDGE_QLEN:                                              # the steps of wave_global_trace's columns per lane (band above 128 diagonals) and of the band forms
        for w in (3, 40, 64, 100, 400):
            for _ in range(5):
                items.append(rand_case(rng, "glb", qlen=qlen, w=w, fam="edge_qlen"))
    for qlen in (1, 2, 5, 30, 61, 120):                                 # a target of one base
        for _ in range(8):
            items.append(rand_case(rng, "glb", qlen=qlen, tlen=1, fam="tlen1"))
    for _ in range(80):                                                 # fewer columns than the band has diagonals
        items.append(rand_case(rng, "glb", qlen=int(rng.integers(1, 130)), w=int(rng.choice([64, 100, 127, 400])), fam="n_col"))
    for L in (64, 65, 128, 700):                                        # backtrack runs of exactly one step, one more, many
        for w in (3, 31, 40, 64, 100):
            for ab in ((1, 4), (50, 60)):
                q = rand_query(rng, L)
                items.append(Case("glb", q, q.copy(), w, dp_kat.GAPS[0], scmat(*ab), fam="identical"))
    items += _indel_family(rng)
    for _ in range(40):
        c = rand_case(rng, "glb", fam="all_n")
        items.append(Case("glb", np.full(c.qlen, 4, np.uint8), c.t, c.w, c.gaps, c.mat, fam="all_n"))
    for _ in range(120):
        items.append(rand_case(rng, "glb", gaps=dp_kat.GAPS[4], fam="free_open"))
    for _ in range(120):
        items.append(rand_case(rng, "glb", ab=(50, 60), fam="mat50"))
    return items, [ora.global2(c) for c in items], [ora.global2(c.reversed()) for c in items]


def test_global_random_vs_oracle(ctx, glb_items):
    items, want, want_rev = glb_items
    n = len(items)
    band = np.array([2 * c.w + 1 for c in items])
    fam = {
        "band 63": (band == 63).sum(), "band 65": (band == 65).sum(), "band 127": (band == 127).sum(), "band 129": (band == 129).sum(),
        "band <= 64": (band <= 64).sum(), "band 65..128": ((band > 64) & (band <= 128)).sum(), "band > 128": (band > 128).sum(),
        "tlen 1": sum(c.tlen == 1 for c in items), "qlen < band": sum(c.qlen < 2 * c.w + 1 for c in items),
        "identical": sum(c.qlen in (64, 65, 128, 700) and np.array_equal(c.q, c.t) for c in items),
        "single indel": sum(c.fam == "indel" for c in items), "all-N query": sum(bool((c.q == 4).all()) for c in items),
        "free gap open": sum(c.gaps[0] == 0 for c in items), "50/60": sum(c.mat[0] == 50 for c in items),
        # from the oracle's answers: the CIGAR begins or ends with a gap, has a gap at all, does not fit the staging
        "gap first/last": sum((a[2] & 15) != 0 or (a[-1] & 15) != 0 for a in want), "with gaps": sum(a[1] > 1 for a in want),
        "over 512 ops": sum(a[1] > bw.KAT_MAX_CIGAR for a in want),
    }
    for q in EDGE_QLEN:
        fam[f"qlen {q}, band > 128"] = sum(c.qlen == q and 2 * c.w + 1 > 128 for c in items)
    print(f"\nglobal: {n} items; " + ", ".join(f"{k}: {int(v)}" for k, v in fam.items()))
    assert 2800 <= n <= 3600
    for k in ("band 63", "band 65", "band 127", "band 129"):
        assert fam[k] >= 60, k
    assert fam["band <= 64"] >= 300 and fam["band 65..128"] >= 300 and fam["band > 128"] >= 500
    assert fam["tlen 1"] >= 48 and fam["qlen < band"] >= 200 and fam["identical"] >= 40 and fam["single indel"] == 144
    assert fam["all-N query"] >= 40 and fam["free gap open"] >= 120 and fam["50/60"] >= 120
    assert fam["gap first/last"] >= 100 and fam["with gaps"] >= 1500 and fam["over 512 ops"] <= n // 100
    assert all(fam[f"qlen {q}, band > 128"] >= 10 for q in EDGE_QLEN)
    _check_global(ctx, items, want, want_rev, "random")


@pytest.mark.parametrize("cpl", dp_kat.CPLS)
def test_global_score_only(ctx, glb_items, cpl):
    """wave_global_score (mem_patch_reg's DP) at every number of columns per lane the dedup kernels are compiled for, both strides."""
    items, want, want_rev = glb_items
    sel = [i for i, c in enumerate(items) if c.qlen + 1 <= 64 * cpl]
    cases = [items[i] for i in sel]
    print(f"\nscore_only cpl {cpl}: {len(cases)} items")
    assert len(cases) >= 1000
    for rev, ans in ((0, want), (1, want_rev)):
        got = dp_kat.device_global(ctx, cases, bw.KAT_GLOBAL_SCORE_ONLY, rev, cpl)
        _diff(got, [[ans[i][0], 0] for i in sel], cases, f"score_only cpl={cpl} reverse={rev}")


# ---------------------------------------------------------------------------------------------------------------- ksw_extend2
PATHS = {"ext_rows<1>": bw.KAT_EXT_ROWS1, "ext_rows<2>": bw.KAT_EXT_ROWS2, "ext_rows<3>": bw.KAT_EXT_ROWS3, "ext_rows<4>": bw.KAT_EXT_ROWS4,
         "short flank": bw.KAT_EXT_SHORT, "wide band": bw.KAT_EXT_WIDE, "beyond 16 bits": bw.KAT_EXT_BEYOND16}


def _coverage(masks):
    return {k: int(((masks & b) != 0).sum()) for k, b in PATHS.items()}


def _check_extend(ctx, ora, cases, cpl, what, want=None):
    want = [ora.extend(c) for c in cases] if want is None else want
    got, masks = dp_kat.device_extend(ctx, cases, cpl, 0)
    _diff(got, want, cases, f"{what} cpl={cpl} forward")
    got_r, masks_r = dp_kat.device_extend(ctx, cases, cpl, 1)
    _diff(got_r, [ora.extend(c.reversed()) for c in cases], cases, f"{what} cpl={cpl} reversed")
    return np.concatenate([masks, masks_r])


@pytest.mark.parametrize("cpl", dp_kat.CPLS)
def test_extend_fixture(ctx, ora, cpl):
    """Every reference-made ksw_extend2 record the instantiation admits, plain and windowed form, both strides."""
    cases = [c for c in dp_kat.load_records("kat_dp_wide.npz")[0] + dp_kat.load_records("kat_ksw.npz")[0] if c.qlen + 1 <= 64 * cpl]
    assert len(cases) >= (430 if cpl == 11 else 150)
    cov = _coverage(_check_extend(ctx, ora, cases, cpl, "fixture", [c.res for c in cases]))
    print(f"\nextend fixture cpl {cpl}: {len(cases)} records; paths " + ", ".join(f"{k}: {v}" for k, v in cov.items()))


def _ext_items(cpl):
    rng = np.random.default_rng(900 + cpl)
    maxq = min(64 * cpl - 1, 700)                                       # the longest flank the instantiation admits

    def qlen_in(lo=1):
        while True:
            n = dp_kat.rand_len(rng) if lo == 1 else int(rng.integers(lo, maxq + 1))
            if lo <= n <= maxq:
                return n
    items = [rand_case(rng, "ext", qlen=qlen_in()) for _ in range(2000)]
    for qlen in (63, 64, 65, maxq):
        items += [rand_case(rng, "ext", qlen=qlen, fam="edge_qlen") for _ in range(40)]
    for w in (0, 1, 119, 120, 121, 127, 128):
        items += [rand_case(rng, "ext", qlen=qlen_in(64), w=w, err=rng.uniform(0, 0.05), fam="edge_w") for _ in range(30)]
    for k in (32759, 32760):                                            # h0 + qlen * mx on either side of what 16 bits hold
        for _ in range(30):
            qlen = int(rng.integers(64, min(maxq, 600) + 1))
            items.append(rand_case(rng, "ext", qlen=qlen, ab=(50, 60), h0=k - 50 * qlen, err=rng.uniform(0, 0.05), fam="16bit"))
    for _ in range(90):
        c = rand_case(rng, "ext", qlen=qlen_in(), fam="edge_h0")
        oe_ins = c.gaps[2] + c.gaps[3]
        items.append(Case("ext", c.q, c.t, c.w, c.gaps, c.mat, (1, oe_ins, oe_ins + 1)[len(items) % 3], c.zdrop, c.bonus, fam="edge_h0"))
    for zdrop in (0, 1):
        items += [rand_case(rng, "ext", qlen=qlen_in(), zdrop=zdrop, fam="zdrop") for _ in range(40)]
    # long near-identical pairs with a gap every 60 bases or so and a band that lets the score spread: these widen the live band, and with it
    # the window hand-overs (w 200 is the extension kernels' second band try: a live band wider than any window)
    for w, count in ((40, 60), (70, 60), (100, 150), (127, 60), (200, 80)):
        for _ in range(count):
            qlen = qlen_in(min(maxq, 150))
            q = rand_query(rng, qlen)
            t = q.copy()
            for p in range(qlen - int(rng.integers(20, 60)), 0, -int(rng.integers(45, 75))):
                g, p = int(rng.integers(1, 11)), min(p, len(t) - 1)
                t = np.delete(t, slice(p, p + g)) if rng.random() < 0.5 else np.insert(t, p, rand_query(rng, g))
            if w == 200 and rng.random() < 0.5:                       # one gap long enough to call for the second band try
                p, g = int(rng.integers(20, len(t) - 10)), int(rng.integers(80, 190))
                t = np.delete(t, slice(p, p + g)) if rng.random() < 0.5 else np.insert(t, p, rand_query(rng, g))
            t = np.concatenate([t, rand_query(rng, int(rng.integers(0, 60)))])
            ab = dp_kat.MATRICES[rng.integers(0, 2)]
            items.append(Case("ext", q, t, w, dp_kat.GAPS[rng.integers(0, 2)], scmat(*ab), int(rng.integers(30, 700)), int(rng.choice([0, 100, 1000])),
                              int(rng.choice([0, 5])), fam=f"long w{w}"))
    return items


@pytest.mark.parametrize("cpl", dp_kat.CPLS)
def test_extend_random_vs_oracle(ctx, ora, cpl):
    """About 3 000 items per instantiation against the oracle, and floors on how many items went through each form of the windowed driver (as the
    kernel itself reports them): a form no item reaches cannot fail."""
    items = _ext_items(cpl)
    maxq = min(64 * cpl - 1, 700)
    fam = {"qlen 63": sum(c.qlen == 63 for c in items), "qlen 64": sum(c.qlen == 64 for c in items), "qlen 65": sum(c.qlen == 65 for c in items),
           f"qlen {maxq}": sum(c.qlen == maxq for c in items), "16 bits - 1": sum(c.h0 + c.qlen * int(c.mat.max()) == 32759 for c in items),
           "16 bits": sum(c.h0 + c.qlen * int(c.mat.max()) == 32760 for c in items), "h0 1": sum(c.h0 == 1 for c in items),
           "h0 oe_ins": sum(c.h0 == c.gaps[2] + c.gaps[3] for c in items), "h0 oe_ins + 1": sum(c.h0 == c.gaps[2] + c.gaps[3] + 1 for c in items),
           "zdrop 0": sum(c.zdrop == 0 for c in items), "zdrop 1": sum(c.zdrop == 1 for c in items), "long": sum(c.fam.startswith("long") for c in items),
           "N's": sum(bool((c.q == 4).any() or (c.t == 4).any()) for c in items)}
    for w in (0, 1, 119, 120, 121, 127, 128, 200):
        fam[f"w {w}"] = sum(c.w == w for c in items)
    assert 2800 <= len(items) <= 3600
    assert all(fam[k] >= 30 for k in fam if k != "N's"), fam
    assert sum(int((c.q == 4).sum()) for c in items) <= 0.05 * sum(c.qlen for c in items)
    cov = _coverage(_check_extend(ctx, ora, items, cpl, "random"))
    print(f"\nextend cpl {cpl}: {len(items)} items, both strides; " + ", ".join(f"{k}: {int(v)}" for k, v in fam.items()) +
          "\n  paths " + ", ".join(f"{k}: {v}" for k, v in cov.items()))
    need = {11: list(PATHS), 3: ["ext_rows<1>", "ext_rows<2>", "ext_rows<3>"]}.get(cpl, ["ext_rows<1>"])
    for k in need:
        assert cov[k] >= 20, (k, cov)
    if cpl <= 3:
        assert cov["ext_rows<4>"] == 0                                  # (flanks below 192 bases: three columns per lane hold any band)


# Found by test_extend_random_vs_oracle (family "long w200") at 5 and 11 columns per lane: with the band of the extension kernels' second try
# (-w doubled to 200, bwamem.c:730) and a score high enough to keep every cell of the band above zero, the live band of a row spans up to 402
# columns (ksw.c:428-430, 466-469), the widest window of the windowed form 256; columns past the window were silently left out and the
# windowed form lost every path more than 55 columns to the right of the band's first column -- plain form and oracle agreed, the windowed
# form differed (score 348 against 470 in the first case met).  wave_extend_fit now takes the plain form whenever the band can outgrow the window.
# A case: the query without `skip` of its bases after the first `keep`, so that the best path runs `skip` columns right of the diagonal.
BAND_BEYOND_WINDOW = {"skip100_of_300": (300, 60, 100), "skip60_of_260": (260, 30, 60), "skip56_of_257": (257, 1, 56)}


def _band_beyond_window_case(name):
    qlen, keep, skip = BAND_BEYOND_WINDOW[name]
    q = rand_query(np.random.default_rng(qlen), qlen)
    return Case("ext", q, np.concatenate([q[:keep], q[keep + skip:]]), 200, (6, 1, 6, 1), scmat(1, 4), 400, 0, 0, fam=name)


@pytest.mark.parametrize("cpl", [5, 11])
@pytest.mark.parametrize("name", sorted(BAND_BEYOND_WINDOW))
def test_extend_band_wider_than_window(ctx, ora, name, cpl):
    c = _band_beyond_window_case(name)
    assert 2 * c.w + 2 > 255 and c.qlen > 255 and c.qlen + 1 <= 64 * cpl
    masks = _check_extend(ctx, ora, [c], cpl, name)
    assert (masks & bw.KAT_EXT_WIDE).all()                              # the plain form, on either stride


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx):
    """The documented error, nothing launched."""
    rng = np.random.default_rng(5)

    def glb(qlen, tlen, w, form, cpl=11, e_ins=1):
        c = Case("glb", rand_query(rng, qlen), rand_query(rng, tlen), w, (6, 1, 6, e_ins), scmat(1, 4))
        return lambda: dp_kat.device_global(ctx, [c], form, 0, cpl)

    def ext(qlen, tlen, cpl, h0=50, e_del=1):
        c = Case("ext", rand_query(rng, qlen), rand_query(rng, tlen), 100, (6, e_del, 6, 1), scmat(1, 4), h0, 100, 5)
        return lambda: dp_kat.device_extend(ctx, [c], cpl)
    for call, err in [(glb(701, 701, 10, bw.KAT_GLOBAL_AUTO_BIG), "ECAPACITY"), (glb(100, 8193, 8200, bw.KAT_GLOBAL_AUTO_BIG), "ECAPACITY"),
                      (glb(100, 2125, 2100, bw.KAT_GLOBAL_SCORE_ONLY), "ECAPACITY"), (glb(192, 192, 10, bw.KAT_GLOBAL_SCORE_ONLY, 3), "ECAPACITY"),
                      (glb(100, 100, 10, 3), "EINVAL"), (glb(100, 100, 10, bw.KAT_GLOBAL_SCORE_ONLY, 6), "EINVAL"),
                      (glb(100, 120, 19, bw.KAT_GLOBAL_AUTO_BIG), "EINVAL"), (glb(100, 100, 10, bw.KAT_GLOBAL_AUTO_SMALL, e_ins=0), "EINVAL"),
                      (ext(701, 700, 11), "ECAPACITY"), (ext(192, 200, 3), "ECAPACITY"), (ext(256, 200, 4), "ECAPACITY"), (ext(100, 2125, 11), "ECAPACITY"),
                      (ext(100, 100, 11, h0=0), "EINVAL"), (ext(100, 100, 11, h0=-3), "EINVAL"), (ext(100, 100, 7), "EINVAL"), (ext(100, 100, 11, e_del=0), "EINVAL")]:
        with pytest.raises(bw.BwahipError, match=err):
            call()
    # what the limits admit is taken: the longest target of each entry, and a declined band comes back as a status, not as an error
    c = Case("glb", rand_query(rng, 10), rand_query(rng, 8192), 8190, (6, 1, 6, 1), scmat(1, 4))
    assert dp_kat.device_global(ctx, [c], bw.KAT_GLOBAL_AUTO_SMALL)[0] == [0, -1]
    assert dp_kat.device_global(ctx, [c], bw.KAT_GLOBAL_AUTO_BIG)[0][1] >= 1
