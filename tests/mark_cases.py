"""Region lists built on purpose for the stage between the region list and the output text: k_mark of csrc/k_final.hip with fin::select_records
and fin::approx_mapq_se (mem_mark_primary_se bwamem.c:500-565, mem_reorder_primary5 bwamem.c:988, the record filter of mem_reg2sam
bwamem.c:1025-1031, the XA membership of mem_gen_alt bwamem_extra.c:116-145, mem_approx_mapq_se bwamem.c:962), fed to bwahip_kat_mark, to
`bwa_oracle katmark` (ora_kat_mark) and, where it is built, to `bwaref katmark` (the reference's own functions).  Deterministic: every
generator is seeded and depends on nothing but the contig table of the suite's small index with its third contig declared ALT.

A region is the 19 words of a stage record.  The code under test never looks at a base, so query spans are free integers (a "read" may be
tens of thousands of bases long where a case needs many regions that do not overlap).  Every region keeps seedcov >= 1, score > 0,
1 <= max(qe - qb, re - rb) < 65536 and sub_n + 1 < 65536: outside those the reference takes log(0) or leaves its log table's range
(bad_case() is the one list beyond them, for the GPU alone).

A set is one batch: (flags for all three programs, the option fields `bwa mem` has no flag for, n_processed, paired, builder).  Cases that
sit on the two sides of a threshold carry `side = (pair name, 0 | 1, kind)`; test_mark_cases_cpu.py checks on the reference's records that
the two sides of every pair really come out differently."""
import hashlib
import math
import os
import subprocess
from collections import namedtuple

import numpy as np

import common
from common import bw

CTG_OFF = (0, 600_000, 900_000)
ALT_RID = 2
TAG_OPT, TAG_MARK, TAG_REGS = 40, 41, 4
W = 25                                                   # words per region of an answer (bw.KAT_MARK_WORDS)
HDR = 4
C_SEC, C_SECALL, C_SUB, C_ALTSC, C_SUBN, C_SCORE, C_ALT, C_QB, C_QE = 13, 14, 7, 8, 10, 5, 17, 2, 3
C_HASH, C_IN, C_NEED, C_OWNER, C_MAPQ, C_BAD = 19, 20, 21, 22, 23, 24
INT_MAX = 0x7fffffff

Case = namedtuple("Case", "name regs side", defaults=(None,))
Set = namedtuple("Set", "flags extra n_processed paired build")


def extra(**kw):
    """The option fields carried in the case file, as mem_opt_init leaves them (bwamem.c:100-107): with mapQ_coef_len = 50 and
    mapQ_coef_fac = (int)log(50) = 3 the first formula of mem_approx_mapq_se is the one every default run takes; mapQ_coef_len = 0
    (what -Q 0 gives) selects the other."""
    d = dict(mask_level=0.5, mapQ_coef_len=50.0, mapQ_coef_fac=3, XA_drop_ratio=0.8, drop_ratio=0.5)
    d.update(kw)
    return d


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def reg(qb, qe, score, alt=0, rb=None, rlen=None, csub=0, sub_n=0, seedcov=None, frac_rep=0.0, w=100, in_range=True):
    """One region; the reference span defaults to the query span's length (at least 1) somewhere inside the region's contig."""
    rid = ALT_RID if alt else 0
    if rlen is None:
        rlen = max(qe - qb, 1)
    if rb is None:
        rb = CTG_OFF[rid] + 1000 + (qb * 7 + score * 13) % 50_000
    if seedcov is None:
        seedcov = max(1, min(qe - qb, score) // 2)
    assert qe >= qb and score > 0 and 1 <= max(qe - qb, rlen) and seedcov >= 1 and 0 <= sub_n < 65535
    assert max(qe - qb, rlen) < 65536 or not in_range
    return [rb, rb + rlen, qb, qe, rid, score, score, 0, 0, csub, sub_n, w, seedcov, -1, -1, 19, 1, alt, f32bits(frac_rep)]


def mk(name, regs, side=None):
    return Case(name, np.array(regs, dtype=np.int64).reshape(-1, 19), side)


def sig(ov, min_l, mask):
    """the overlap test of bwamem.c:512 as C evaluates it: int >= int * float, in float"""
    return bool(np.float32(ov) >= np.float32(min_l) * np.float32(mask))


# ------------------------------------------------------------------------------------------------ list sizes and order
SIZES = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 500, 1000)


def scattered(rng, n, scores, alt_every=0, span=400):
    """n regions of 30 .. 120 query bases scattered over `span`: they overlap one another in every degree"""
    out = []
    for i in range(n):
        ln = int(rng.integers(30, 121))
        qb = int(rng.integers(0, span))
        out.append(reg(qb, qb + ln, int(scores[i]), alt=1 if alt_every and i % alt_every == alt_every - 1 else 0))
    return out


def size_cases():
    rng = np.random.default_rng(41)
    out = []
    for n in SIZES:
        span = 400 if n < 200 else 3000
        out.append(mk(f"size.{n}.equal", scattered(rng, n, [77] * n, span=span)))
        out.append(mk(f"size.{n}.equal_alt", scattered(rng, n, [77] * n, alt_every=3, span=span)))
        out.append(mk(f"size.{n}.two", scattered(rng, n, [60 + 20 * int(x) for x in rng.integers(0, 2, n)], alt_every=5, span=span)))
        out.append(mk(f"size.{n}.desc", scattered(rng, n, [40 + n - i for i in range(n)], alt_every=4, span=span)))
        out.append(mk(f"size.{n}.asc", scattered(rng, n, [40 + i for i in range(n)], alt_every=4, span=span)))
    return out


def position_cases():
    """The same two lists (40 regions: LDS would not hold them; 200: the bitonic sort) at reads 0, 1 and 70 of a batch: the hash, and with it
    the order among equal scores, follows the read's id."""
    rng = np.random.default_rng(42)
    a = scattered(rng, 40, [50 + int(x) for x in rng.integers(0, 3, 40)], alt_every=4)
    b = scattered(rng, 200, [50 + int(x) for x in rng.integers(0, 3, 200)], alt_every=6, span=1500)
    c = scattered(rng, 20, [64] * 20, alt_every=5)
    out = []
    for i in range(72):
        if i in (0, 1, 70):
            out.append(mk(f"pos.{i}.a40", a))
        elif i in (2, 3, 71):
            out.append(mk(f"pos.{i}.b200", b))
        elif i in (4, 5, 69):
            out.append(mk(f"pos.{i}.c20", c))
        else:
            n = int(rng.integers(0, 6))
            out.append(mk(f"pos.{i}.fill", scattered(rng, n, [45 + int(x) for x in rng.integers(0, 30, n)])))
    return out


# ------------------------------------------------------------------------------------------------ the overlap test
def overlap_cases(mask=0.5):
    """Two regions whose overlap is one base below, at and above the first length the test of bwamem.c:512 calls significant -- for minimum
    lengths whose product with mask_level is and is not exact in float --, touching regions, a contained one, an empty query span."""
    out = []
    for min_l in (10, 33, 100, 101, 110, 149, 1000, 3333):
        thr = next(ov for ov in range(0, min_l + 2) if sig(ov, min_l, mask))
        if not 1 <= thr <= min_l:
            continue
        for ov in sorted({thr - 1, thr, thr + 1, min_l} - {0}):
            if ov > min_l:
                continue
            # the longer region first (higher score), the shorter one of min_l bases overlapping its end by ov
            a = reg(0, min_l + 50, 90)
            b = reg(min_l + 50 - ov, 2 * min_l + 50 - ov, 80)
            side = (f"ov.{mask}.{min_l}", int(ov >= thr), "parent") if ov in (thr - 1, thr) else None
            out.append(mk(f"ov.m{mask}.l{min_l}.ov{ov}", [a, b], side))
            out.append(mk(f"ov.m{mask}.l{min_l}.ov{ov}.alt", [a, reg(min_l + 50 - ov, 2 * min_l + 50 - ov, 80, alt=1), reg(5000, 5100, 70)]))
    out.append(mk("ov.touching", [reg(0, 100, 90), reg(100, 200, 80)]))
    out.append(mk("ov.one_base", [reg(0, 100, 90), reg(99, 101, 80)]))
    out.append(mk("ov.contained", [reg(0, 100, 90), reg(40, 60, 80)]))
    out.append(mk("ov.contained_long_first", [reg(40, 60, 90), reg(0, 100, 80)]))
    out.append(mk("ov.empty_span", [reg(0, 100, 90), reg(50, 50, 80, rlen=20), reg(0, 0, 70, rlen=5)]))
    out.append(mk("ov.identical", [reg(10, 110, 90), reg(10, 110, 90), reg(10, 110, 90, alt=1)]))
    return out


# ------------------------------------------------------------------------------------------------ the order of kept regions
def kept_cases():
    out = []
    # a region that overlaps two kept regions becomes the secondary of the first (the higher score)
    out.append(mk("kept.two_parents", [reg(0, 100, 100), reg(100, 200, 95), reg(40, 160, 60)]))
    out.append(mk("kept.two_parents.second_first", [reg(0, 100, 95), reg(100, 200, 100), reg(40, 160, 60)]))
    out.append(mk("kept.three_parents", [reg(0, 100, 100), reg(100, 200, 99), reg(200, 300, 98), reg(30, 270, 50), reg(130, 270, 49)]))
    # 40 kept regions side by side, each with two secondaries; scores fall along the read, so kept and secondary regions interleave after the sort
    regs = []
    for k in range(40):
        regs += [reg(200 * k, 200 * k + 100, 200 - k), reg(200 * k + 10, 200 * k + 90, 120 - k), reg(200 * k + 20, 200 * k + 110, 60 + k, alt=k % 7 == 3)]
    out.append(mk("kept.forty", regs))
    # kept region 0 absorbs nothing among its first 70 candidates (they sit elsewhere, under region 1) and then region 71
    regs = [reg(0, 100, 300), reg(1000, 1100, 299)] + [reg(1000 + i % 7, 1100 - i % 5, 290 - i) for i in range(69)] + [reg(5, 95, 100), reg(1010, 1090, 99)]
    out.append(mk("kept.first_absorbed_beyond_64", regs))
    # kept region 0 absorbs its first 70 candidates; the next open region is number 71
    regs = [reg(0, 100, 300)] + [reg(i % 7, 100 - i % 5, 290 - i) for i in range(70)] + [reg(1000, 1100, 100), reg(1010, 1090, 99), reg(2000, 2100, 98)]
    out.append(mk("kept.next_open_beyond_64", regs))
    # the same two with ALT regions mixed in, so that the second pass over the primaries sees other distances
    regs = [reg(0, 100, 300)] + [reg(i % 7, 100 - i % 5, 290 - i, alt=i % 2) for i in range(140)] + [reg(1000, 1100, 100), reg(1010, 1090, 99, alt=1), reg(2000, 2100, 98)]
    out.append(mk("kept.next_open_beyond_64.alt", regs))
    return out


# ------------------------------------------------------------------------------------------------ sub and sub_n
def tmp_of(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1):
    return max(a + b, o_del + e_del, o_ins + e_ins)


def subn_cases(tmp=7):
    """A kept region and one it absorbs, the score gap at tmp and at tmp + 1, in the four ALT / primary combinations of bwamem.c:518; then
    five absorbed regions of which some count."""
    out = []
    for ja in (0, 1):
        for ia in (0, 1):
            for d in (0, 1):
                regs = [reg(0, 100, 200, alt=ja), reg(5, 95, 200 - tmp - d, alt=ia), reg(1000, 1100, 50)]
                out.append(mk(f"subn.j{ja}.i{ia}.gap{tmp}+{d}", regs, (f"subn.{tmp}.j{ja}.i{ia}", 1 - d, "sub_n") if (ja or not ia) else None))
    out.append(mk("subn.five", [reg(0, 100, 200, sub_n=3)] + [reg(2 + i, 98, 200 - tmp + 2 - i, alt=i == 1) for i in range(5)]))
    out.append(mk("subn.equal_scores", [reg(0, 100, 200), reg(0, 100, 200), reg(0, 100, 200, alt=1), reg(0, 100, 200)]))
    return out


# ------------------------------------------------------------------------------------------------ ALT
def alt_cases():
    rng = np.random.default_rng(43)
    out = []
    for n in (20, 32, 33, 90, 128, 129, 200, 300):
        for n_pri in (0, 1, n - 1, n):
            alt = np.ones(n, dtype=int)
            alt[rng.choice(n, n_pri, replace=False)] = 0
            regs = []
            for i in range(n):
                ln = int(rng.integers(30, 121))
                qb = int(rng.integers(0, 500))
                regs.append(reg(qb, qb + ln, 40 + int(rng.integers(0, 60)), alt=int(alt[i])))
            out.append(mk(f"alt.n{n}.pri{n_pri}", regs))
        # an ALT region scoring above every primary and covering them: alt_sc; ALT regions below them: secondary = INT_MAX
        regs = [reg(0, 150, 150, alt=1)] + [reg(i % 11, 150 - i % 13, 140 - i % 30) for i in range(n - 3)] + [reg(3, 140, 35, alt=1), reg(200, 300, 90, alt=1)]
        out.append(mk(f"alt.n{n}.alt_on_top", regs))
    return out


# ------------------------------------------------------------------------------------------------ -5
def five_cases(T=30):
    out = []

    def fill(regs, n):
        """secondaries under the kept regions until the list has n entries"""
        kept = list(regs)
        i = 0
        while len(regs) < n:
            k = kept[i % len(kept)]
            regs.append(reg(k[2] + 1 + i % 5, k[3] - 1 - i % 3, max(1, k[5] - 5 - i % 9), alt=i % 6 == 5))
            i += 1
        return regs
    for n in (8, 32, 33, 140):
        out.append(mk(f"five.n{n}.one_primary", fill([reg(100, 200, 90)], n)))
        out.append(mk(f"five.n{n}.none_above_T", fill([reg(100, 200, T - 1), reg(300, 400, T - 2)], n)))
        out.append(mk(f"five.n{n}.leftmost_first", fill([reg(0, 100, 90), reg(300, 400, 80), reg(600, 700, 70)], n)))
        out.append(mk(f"five.n{n}.leftmost_at_k", fill([reg(600, 700, 90), reg(300, 400, 80), reg(0, 100, 70)], n)))
        out.append(mk(f"five.n{n}.leftmost_second", fill([reg(600, 700, 90), reg(0, 100, 80)], n), (f"five.swap.n{n}", 1, "first")))
        out.append(mk(f"five.n{n}.leftmost_second.below_T", fill([reg(600, 700, 90), reg(0, 100, T - 1)], n), (f"five.swap.n{n}", 0, "first")))
        out.append(mk(f"five.n{n}.leftmost_is_alt", fill([reg(600, 700, 90), reg(300, 400, 80), reg(0, 100, 70, alt=1)], n)))
        out.append(mk(f"five.n{n}.leftmost_at_T", fill([reg(600, 700, 90), reg(300, 400, 80), reg(0, 100, T)], n)))
    return out


# ------------------------------------------------------------------------------------------------ the selection
def find_rounding(ratio, lo=110, hi=800):
    """(parent, k): parent * ratio is k in float (the product rounds down) but above k in double -- score k passes `score < parent * ratio`
    only when the comparison is made in float, as bwamem.c:1028 makes it"""
    r32 = np.float32(ratio)
    for p in range(lo, hi):
        prod = np.float32(p) * r32
        if float(prod) == int(prod) and float(p) * float(r32) > float(prod):
            return p, int(prod)
    raise AssertionError(ratio)


def select_cases(T=30, drop=0.5, xa=0.8, hits=5, hits_alt=200, all_=False):
    out = []

    def under(name, parent, scores, alts=(), side=None, extra_regs=()):
        regs = [reg(0, 100, parent)] + [reg(1 + i % 3, 100 - i % 4, s, alt=1 if i in alts else 0) for i, s in enumerate(scores)] + list(extra_regs)
        out.append(mk(name, regs, side))
    for d in (0, 1):
        out.append(mk(f"sel.T-{d}", [reg(0, 100, T - d), reg(500, 600, 100)], ("sel.T", 1 - d, "need")))
        out.append(mk(f"sel.T-{d}.alone", [reg(0, 100, T - d)], ("sel.T.alone", 1 - d, "need")))
    # a secondary at parent * drop_ratio, below it, and where float and double part
    p, k = find_rounding(drop) if float(np.float32(drop)) != drop else (100, int(100 * drop))
    for d in (0, 1):
        under(f"sel.drop.{p}.{k}-{d}", p, [k - d], side=("sel.drop", 1 - d, "need") if all_ else None)      # (without -a no secondary prints a record)
    under("sel.drop.alt_secondary", 100, [90, 60, 40], alts=(0, 2))
    under("sel.drop.exact_half", 100, [50, 49])
    # XA_drop_ratio, compared in double: parent * 0.8 integral (100) and not (101)
    for parent in (100, 101):
        t = math.ceil(parent * float(np.float32(xa)))
        for d in (0, 1):
            under(f"sel.xa.p{parent}.s{t - d}", parent, [t - d], side=None if all_ else (f"sel.xa.{parent}", 1 - d, "need"))      # (with -a there is no XA tag)
        under(f"sel.xa.p{parent}.integral", parent, [int(parent * xa), int(parent * xa) + 1])
    # the caps on the number of hits under one primary
    for n, alts in ((hits, ()), (hits + 1, ()), (hits + 1, (2,)), (hits_alt, (0,)), (hits_alt + 1, (0,)), (hits_alt + 1, ()), (300, ()), (300, (299,))):
        side = None
        if not alts and n in (hits, hits + 1) and not all_:
            side = ("sel.cap", int(n == hits), "need")
        if alts == (0,) and n in (hits_alt, hits_alt + 1) and not all_:
            side = ("sel.cap_alt", int(n == hits_alt), "need")
        name = f"sel.hits{n}" + (".alt" if alts else "")
        regs = [reg(0, 100, 100)] + [reg(0, 100, 99 - i % 15, alt=1 if i in alts else 0) for i in range(n)] + [reg(1000, 1100, 95)]
        # two regions pad the comparison of the pair so that both sides have the same length
        if side and side[1] == 1:
            regs.append(reg(1000, 1100, 20))
        out.append(mk(name, regs, side))
    # 70 primaries with one hit each: the per-primary counts of two lane blocks
    regs = []
    for i in range(70):
        regs += [reg(200 * i, 200 * i + 100, 100 + i), reg(200 * i + 1, 200 * i + 99, 90 + i, alt=i % 9 == 8)]
    out.append(mk("sel.seventy", regs))
    # hits below the XA ratio do not count towards the cap
    under("sel.cap.uncounted", 100, [99] * hits + [50, 40, 30])
    return out


# ------------------------------------------------------------------------------------------------ mapQ
def mapq_cases(a=1, b=4, spans=((100, 100), (100, 110), (110, 100)), per_list=96):
    """The grid of mem_approx_mapq_se's inputs.  `sub` is not an input of the stage but what marking makes of the list, so every grid point
    is a kept region with, where sub > 0 is wanted, one region of that score inside it; the points sit 1000 query bases apart, 96 to a list."""
    pts = []
    for q, r in spans:
        l = max(q, r)
        s95 = l * a - l * (a + b) // 20                  # identity 0.95 (exactly, where l is a multiple of 20)
        for score in sorted({int(0.4 * l * a), s95 - 1, s95, s95 + 1, l * a - 2 * (a + b), l * a}):
            if score < 20:
                continue
            for sub in (0, score // 2, score - 1):
                for csub in (0, score - 3):
                    for sub_n in (0, 1, 2, 50):
                        for seedcov in (1, 19, 60):
                            for frac in (0.0, 0.25, 0.999):
                                pts.append((q, r, score, sub, csub, sub_n, seedcov, frac))
    out = []
    for s in range(0, len(pts), per_list):
        regs = []
        for k, (q, r, score, sub, csub, sub_n, seedcov, frac) in enumerate(pts[s:s + per_list]):
            qb = 1000 * k
            regs.append(reg(qb, qb + q, score, rlen=r, csub=csub, sub_n=sub_n, seedcov=seedcov, frac_rep=frac))
            if sub:
                regs.append(reg(qb + 1, qb + q - 1, sub, seedcov=max(1, seedcov // 2), frac_rep=frac, sub_n=sub_n // 2))
        out.append(mk(f"mapq.{s // per_list}", regs))
    return out


def mapq_edge_cases(a=1, b=4, coef_len=0):
    """identity on either side of 0.95 (l = 100: 1 - (100 a - score) / (a + b) / 100) and, with mapQ_coef_len > 0, l on either side of it"""
    out = []
    s95 = 100 * a - 5 * (a + b)
    for d in (0, 1):                                    # (a low seedcov keeps the result below the cap of 60; the first formula has no such test)
        out.append(mk(f"mapq.identity.{s95 - d}", [reg(0, 100, s95 - d, seedcov=3)], None if coef_len else ("mapq.identity", 1 - d, "mapq")))
    if coef_len:
        for d in (0, 1):
            l = coef_len - d
            out.append(mk(f"mapq.coef_len.l{l}", [reg(0, l, 30, seedcov=20), reg(1, l - 1, 20)], ("mapq.coef_len", 1 - d, "mapq")))
        for l in (coef_len - 10, coef_len + 1, 150, 1000):
            out.append(mk(f"mapq.coef_len.l{l}.r", [reg(0, l - 5, l * a - 7, rlen=l, seedcov=20), reg(1, l - 6, 25, alt=1)]))
    return out


# ------------------------------------------------------------------------------------------------ random
def random_cases(n_lists=400, max_n=300, seed=44):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_lists):
        n = int(rng.integers(1, max_n + 1))
        span = int(rng.choice((150, 400, 2000)))
        regs = []
        for _ in range(n):
            ln = int(rng.integers(19, 151))
            qb = int(rng.integers(0, span))
            score = int(rng.integers(19, ln + 1))
            regs.append(reg(qb, qb + ln, score, alt=int(rng.integers(0, 5) == 0), rlen=ln + int(rng.integers(-3, 4)) if ln > 22 else ln, csub=int(rng.integers(0, score)) if rng.integers(0, 3) == 0 else 0,
                            sub_n=int(rng.integers(0, 4)), seedcov=int(rng.integers(1, score + 1)), frac_rep=float(rng.choice((0.0, 0.0, 0.1, 0.5)))))
        out.append(mk(f"random.{k}", regs))
    return out


def bad_case():
    """A reference span of 65 536 bases: mem_approx_mapq_se would need log() beyond the table.  GPU only: bad = 1 and mapQ 0."""
    return mk("bad.long_span", [reg(0, 100, 90, rlen=65536, in_range=False), reg(200, 300, 80)])


# ------------------------------------------------------------------------------------------------ the sets
NP = {"np0": 0, "np1": 1, "np2g": 1 << 31, "np1t": (1 << 40) + 3}
SETS = {
    "sizes": Set([], extra(), 0, False, size_cases),
    "sizes_pe": Set([], extra(), 6, True, size_cases),
    "overlap": Set([], extra(), 0, False, overlap_cases),
    "overlap_m0.3": Set([], extra(mask_level=0.3), 0, False, lambda: overlap_cases(0.3)),
    "overlap_m0.9": Set([], extra(mask_level=0.9), 0, False, lambda: overlap_cases(0.9)),
    "kept": Set([], extra(), 0, False, kept_cases),
    "subn": Set([], extra(), 0, False, subn_cases),
    "subn_ab": Set(["-B", "9"], extra(), 0, False, lambda: subn_cases(tmp_of(b=9))),
    "subn_del": Set(["-O", "8,2"], extra(), 0, False, lambda: subn_cases(tmp_of(o_del=8, o_ins=2))),
    "subn_ins": Set(["-O", "2,8", "-E", "1,2"], extra(), 0, False, lambda: subn_cases(tmp_of(o_del=2, o_ins=8, e_ins=2))),
    "subn_A2": Set(["-A", "2"], extra(), 0, False, lambda: subn_cases(tmp_of(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2))),
    "alt": Set([], extra(), 0, False, alt_cases),
    "five": Set(["-5"], extra(), 0, False, five_cases),
    "five_pe": Set(["-5"], extra(), 10, True, five_cases),
    "select": Set([], extra(), 0, False, select_cases),
    "select_a": Set(["-a"], extra(), 0, False, lambda: select_cases(all_=True)),
    "select_a_D0.3": Set(["-a"], extra(drop_ratio=0.3), 0, False, lambda: select_cases(drop=0.3, all_=True)),
    "select_xa0.7": Set([], extra(XA_drop_ratio=0.7), 0, False, lambda: select_cases(xa=0.7)),
    "select_h3,10": Set(["-h", "3,10"], extra(), 0, False, lambda: select_cases(hits=3, hits_alt=10)),
    "mapq": Set([], extra(), 0, False, lambda: mapq_cases(spans=((49, 49), (50, 50), (51, 49), (100, 100), (100, 110), (110, 100))) + mapq_edge_cases(coef_len=50)),
    "mapq_Q0": Set([], extra(mapQ_coef_len=0.0, mapQ_coef_fac=0), 0, False, lambda: mapq_cases() + mapq_edge_cases()),
    "mapq_Q0_A2": Set(["-A", "2"], extra(mapQ_coef_len=0.0, mapQ_coef_fac=0), 0, False, lambda: mapq_cases(a=2, b=8, spans=((100, 100), (100, 104))) + mapq_edge_cases(a=2, b=8)),
    "mapq_A2": Set(["-A", "2"], extra(), 0, False, lambda: mapq_cases(a=2, b=8, spans=((50, 50), (100, 104))) + mapq_edge_cases(a=2, b=8, coef_len=50)),
    "mapq_Q200": Set([], extra(mapQ_coef_len=200.0, mapQ_coef_fac=5), 0, False, lambda: mapq_edge_cases(coef_len=200)),
    "random": Set([], extra(), 12345, False, random_cases),
    "random_a5": Set(["-a", "-5"], extra(), 777, True, lambda: random_cases(150, 200, 45)),
}
for _k, _v in NP.items():
    SETS[f"position_{_k}"] = Set([], extra(), _v, False, position_cases)
    SETS[f"position_{_k}_pe"] = Set([], extra(), _v, True, position_cases)

_built = {}


def cases_of(name):
    if name not in _built:
        _built[name] = SETS[name].build()
    return _built[name]


def opt_of(name):
    """The bwahip option struct of a set: its flags, then the carried fields, and BWAHIP_F_PE for a paired set."""
    s = SETS[name]
    o, _ = common.opt_from_cli(s.flags)
    for k, v in s.extra.items():
        setattr(o, k, v)
    if s.paired:
        o.flag |= 0x2
    return o


# ------------------------------------------------------------------------------------------------ running them
def pack(cases):
    off = np.cumsum([0] + [len(c.regs) for c in cases]).astype(np.int64)
    regs = np.concatenate([c.regs for c in cases]) if cases else np.zeros((0, 19), np.int64)
    return off, regs


def case_words(name, cases=None):
    """The case file of `bwa_oracle katmark` / `bwaref katmark` (oracle/kat_mark_io.h) as int64 words."""
    s = SETS[name]
    cases = cases_of(name) if cases is None else cases
    e = s.extra
    w = [np.array([TAG_OPT, 7, f32bits(e["mask_level"]), f32bits(e["mapQ_coef_len"]), e["mapQ_coef_fac"], f32bits(e["XA_drop_ratio"]), f32bits(e["drop_ratio"]),
                   s.n_processed, int(s.paired)], np.int64)]
    for i, c in enumerate(cases):
        w += [np.array([bw.TAG_READ, 2, i, 0, TAG_REGS, 1 + c.regs.size, len(c.regs)], np.int64), c.regs.ravel()]
    return np.concatenate(w)


def input_digest(name):
    return hashlib.sha256(case_words(name).tobytes() + " ".join(SETS[name].flags).encode()).hexdigest()


def run_checker(exe, name, workdir, tag="c"):
    """-> per read the answer record (4 header words + 25 per region)."""
    fin, fout = os.path.join(workdir, f"{tag}.{name}.in.bin"), os.path.join(workdir, f"{tag}.{name}.out.bin")
    case_words(name).tofile(fin)
    subprocess.check_call([exe, "katmark", *SETS[name].flags, "-", fin, fout])
    reads = common.by_read(bw.read_record_file(fout))
    assert len(reads) == len(cases_of(name))
    return [r[TAG_MARK] for r in reads]


def shared(rec):
    """An answer with the words the reference cannot give zeroed: the two selection counts, need and the XA owner of every region."""
    a = rec.copy()
    a[2] = a[3] = 0
    body = a[HDR:].reshape(-1, W)
    body[:, C_NEED] = 0
    body[:, C_OWNER] = 0
    return a


def no_plan(rec):
    """What bwahip_kat_mark returns with plan 0: the same as shared()"""
    return shared(rec)


def digests(recs):
    """Per read the sha256 of its answer's shared words: what kat_mark.npz holds."""
    return np.array([hashlib.sha256(shared(r).tobytes()).digest() for r in recs], dtype="S32")


def body(rec):
    return rec[HDR:].reshape(-1, W)


def outcome(rec, kind):
    """What a case on one side of a threshold must differ in from the case on the other side, as a tuple over the regions in input order."""
    b = body(rec)
    by_in = np.argsort(b[:, C_IN], kind="stable")
    src = b[:, C_IN]

    def parent(col):
        return tuple(int(x) if x < 0 or x == INT_MAX else int(src[x]) for x in b[by_in, col])
    if kind == "parent":
        return parent(C_SEC), parent(C_SECALL)
    if kind == "sub_n":
        return tuple(int(x) for x in b[by_in, C_SUBN])
    if kind == "need":
        return tuple(int(x) for x in b[by_in, C_NEED]), tuple(int(x) if x < 0 else int(src[x]) for x in b[by_in, C_OWNER])
    if kind == "mapq":
        return tuple(int(x) for x in b[by_in, C_MAPQ])
    if kind == "first":
        return int(src[0])
    raise KeyError(kind)


def pairs_of(name):
    """{pair name: (kind, index of side 0, index of side 1)}"""
    out = {}
    for i, c in enumerate(cases_of(name)):
        if c.side:
            p, s, kind = c.side
            d = out.setdefault(p, [kind, None, None])
            assert d[0] == kind and d[1 + s] is None, (name, p)
            d[1 + s] = i
    assert all(d[1] is not None and d[2] is not None for d in out.values()), name
    return {p: tuple(d) for p, d in out.items()}
