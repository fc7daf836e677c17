"""Pairs of region lists built on purpose for the pairing stage: k_pair of csrc/k_pair.hip (mem_pair bwamem_pair.c:208-272 and the decisions of
mem_sam_pe bwamem_pair.c:303-365, 397-411), fed to bwahip_kat_pair, to `bwa_oracle katpair` (ora_kat_pair) and, where it is built, to `bwaref
katpair` (the reference's own mem_mark_primary_se, mem_reorder_primary5 and mem_pair).  Deterministic: every generator is seeded and depends on
nothing but the contig table of the suite's small index with its third contig declared ALT (chain_cases.alt_index).

A region is the 19 words of a stage record (mark_cases.py); the code under test never looks at a base.  mem_pair keys a region by
x = contig << 32 | forward position of rb within the contig (a reverse-strand rb is mirrored at l_pac first), and pairs an upstream region k
with a downstream region i of the other end when x_i - x_k lies in [low, high] of the orientation strand_k << 1 | strand_i (FF 0, FR 1, RF 2,
RR 3).  preg() therefore takes the KEY position and the strand and derives rb.  Unless a builder says otherwise the regions of one end share
the query span [0, 100): after marking all but the best are secondary, so is_multi stays 0 and n_pri = n (no ALT region).

A set is one batch: (flags for all three programs, the option fields `bwa mem` has no flag for, n_processed, the four insert-size records,
builder); reads 2p and 2p + 1 are pair p.  Cases on the two sides of a threshold carry side = (pair name, 0 | 1, kind);
test_pair_cases_cpu.py checks that the two sides really come out differently.

mem_pair takes a region for a primary-assembly hit by its is_alt word, not by its contig: the cases that need a candidate at the very end of
the reference (the last contig is the ALT one) give such a region is_alt = 0 on purpose."""
import hashlib
import math
import os
import subprocess
from collections import namedtuple

import numpy as np

import common
import mark_cases as mc
from common import bw

CTG_LEN = (600_000, 300_000, 100_000)
CTG_OFF = (0, 600_000, 900_000)
L_PAC = 1_000_000
ALT_RID = 2
FF, FR, RF, RR = 0, 1, 2, 3
TAG_OPT, TAG_PAIR, TAG_EXTRA, TAG_MEMPAIR, TAG_MARKED, TAG_REGS = 42, 43, 44, 45, 46, 4
HDR, W = 12, 22                                          # bw.KAT_PAIR_WORDS
H_MODE, H_HREG, H_ALT, H_MAPQ, H_FLAG, H_O, H_SUB, H_NSUB, H_N, H_NPRI, H_TASK, H_REC = range(12)
C_SUB, C_SEC, C_SECALL, C_SCORE, C_IN, C_NEED, C_OWNER = 7, 13, 14, 5, 19, 20, 21
X_NV, X_NU, X_BK, X_BI, X_SK, X_SI, X_HAS_UN, X_O_UN, X_MULTI, X_REPARENT = range(10)
NEED_REC, NEED_XA, NEED_H = 1, 2, 4

Case = namedtuple("Case", "name a b side", defaults=(None,))          # a, b: the regions of end 0 and of end 1, [n x 19] int64
Set = namedtuple("Set", "flags extra n_processed pes build")


def pes(ff=None, fr=None, rf=None, rr=None):
    """four insert-size records; an orientation given as (low, high, avg, std) is live, None is failed"""
    return tuple((0, 0, 1, 0.0, 0.0) if d is None else (int(d[0]), int(d[1]), 0, float(d[2]), float(d[3])) for d in (ff, fr, rf, rr))


WIN = (180, 420, 300.0, 30.0)                            # avg +- 4 std, as mem_pestat would leave a tidy library
PES_FR = pes(fr=WIN)
PES_ALL = pes(WIN, WIN, WIN, WIN)


def preg(pos, strand, score, rid=0, qb=0, qe=100, csub=0, sub_n=0, seedcov=None, frac_rep=0.0, is_alt=None, rlen=None):
    """One region whose mem_pair key is (rid, pos): rb = the forward coordinate, or its mirror image at l_pac on the reverse strand."""
    p = CTG_OFF[rid] + pos
    rb = p if strand == 0 else 2 * L_PAC - 1 - p
    if rlen is None:
        rlen = max(qe - qb, 1)
    if seedcov is None:
        seedcov = max(1, min(qe - qb, score) // 2)
    assert 0 <= pos < CTG_LEN[rid] and score > 0 and qe >= qb and 1 <= max(qe - qb, rlen) < 65536 and seedcov >= 1 and 0 <= sub_n < 65535
    return [rb, rb + rlen, qb, qe, rid, score, score, 0, 0, csub, sub_n, 100, seedcov, -1, -1, 19, 1, int(rid == ALT_RID) if is_alt is None else is_alt, mc.f32bits(frac_rep)]


def key_x(r):
    """mem_pair's key x of a region given as its 19 words (bwamem_pair.c:216-217)"""
    rb, rid = int(r[0]), int(r[4])
    return rid << 32 | ((rb if rb < L_PAC else 2 * L_PAC - 1 - rb) - CTG_OFF[rid])


def mk(name, a, b, side=None):
    return Case(name, np.array(a, dtype=np.int64).reshape(-1, 19), np.array(b, dtype=np.int64).reshape(-1, 19), side)


def pen(dist, st, a=1):
    """.721 * log(2 * erfc(|ns| / sqrt 2)) * a of bwamem_pair.c:244 by the host's libm, as the product's table and the checkers make it"""
    ns = (dist - st[2]) / st[3]
    e = 2. * math.erfc(abs(ns) * math.sqrt(.5))
    return .721 * (math.log(e) if e > 0 else -math.inf) * a


def q_of(s0, s1, dist, st, a=1):
    v = s0 + s1 + pen(dist, st, a) + .499
    return max(0, int(v)) if v > -2e9 else 0


def pair_at(pos, dist, d, up, s_up=100, s_down=100, rid=0, **kw):
    """(regions of end 0, of end 1): one candidate pair of orientation d at distance dist, the upstream region belonging to end `up`"""
    u, v = preg(pos, d >> 1, s_up, rid, **kw), preg(pos + dist, d & 1, s_down, rid, **kw)
    return ([u], [v]) if up == 0 else ([v], [u])


# ------------------------------------------------------------------------------------------------ the window
def window_cases(d, st=WIN):
    out = []
    lo, hi = st[0], st[1]
    for up in (0, 1):
        for dist in (lo - 1, lo, lo + 1, round(st[2]), hi - 1, hi, hi + 1):
            side = None
            if dist in (lo - 1, lo):
                side = (f"win.d{d}.up{up}.low", int(dist == lo), "paired")
            if dist in (hi, hi + 1):
                side = (f"win.d{d}.up{up}.high", int(dist == hi), "paired")
            out.append(mk(f"win.d{d}.up{up}.dist{dist}", *pair_at(5000, dist, d, up), side))
    return out


def failed_cases():
    """One candidate pair per orientation, each at a locus of its own with its own scores: the best pair is the best LIVE one.  The same
    16 pairs go through each of the 16 masks (one set per mask)."""
    out = []
    for up in (0, 1):
        for rot in range(8):
            a, b = [], []
            for d in range(4):
                x, y = pair_at(5000 + 20_000 * d, 250 + 30 * d, d, up, 100 - 5 * ((d + rot) % 4), 100 - 3 * ((d + 2 * rot) % 4))
                a += x
                b += y
            out.append(mk(f"failed.up{up}.rot{rot}", a, b))
    return out


# ------------------------------------------------------------------------------------------------ the penalty
def penalty_cases(st, a=1, score=60):
    return [mk(f"pen.dist{dist}", *pair_at(7000, dist, FR, dist & 1, score * a, score * a)) for dist in range(st[0], st[1] + 1)]


# ------------------------------------------------------------------------------------------------ sizes of v
NV = (2, 3, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 600)


def crowd(rng, n0, n1, span=3000):
    """n0 forward regions of end 0 and n1 reverse regions of end 1 within a few kilobases, scores with many ties, positions that collide"""
    a = [preg(5000 + int(rng.integers(0, span)), 0, 60 + int(rng.integers(0, 4))) for _ in range(n0)]
    b = [preg(5000 + int(rng.integers(0, span)), 1, 60 + int(rng.integers(0, 4))) for _ in range(n1)]
    return a, b


def size_cases():
    rng = np.random.default_rng(51)
    out = []
    for nv in NV:
        for n0 in sorted({nv // 2, 1, nv - 1}):
            a, b = crowd(rng, n0, nv - n0, span=300 if nv < 10 else 3000)
            if nv >= 63:                                 # equal x on purpose: across the ends, within an end, on both strands (mid-span: a lone region has partners)
                a[0][0:2] = preg(6500, 0, 60)[0:2]
                b[0][0:2] = preg(6500, 1, 60)[0:2]
                if n0 > 2:
                    a[1][0:2] = a[2][0:2]
            out.append(mk(f"size.nv{nv}.n0_{n0}", a, b))
    return out


# ------------------------------------------------------------------------------------------------ lanes
def lane_cases(nv=130):
    """v of nv keys: forward regions of end 0 1500 bases apart (no two of them pair) and a few reverse regions of end 1, each 300 behind
    a forward one -- so the sorted index i of every admissible pair, and with it the lane i % 64 that finds it, is known by construction.
    spec: [(index of the forward region, score of that region, score of the reverse one, extra forward partners 50 bases on)]"""
    def build(name, spec):
        n_extra = sum(e for _, _, _, e in spec)
        n_fill = nv - len(spec) - n_extra
        at = {j: (su, sd, e) for j, su, sd, e in spec}
        a, b = [], []
        for j in range(n_fill):
            p = 2000 + 1500 * j
            su, sd, e = at.get(j, (50, None, 0))
            a.append(preg(p, 0, su))
            for t in range(e):
                a.append(preg(p + 50 * (t + 1), 0, su - 3 * (t + 1)))
            if sd is not None:
                b.append(preg(p + 300, 1, sd))
        assert len(a) + len(b) == nv
        return mk(f"lanes.{name}", a, b)
    return [
        build("one", [(40, 60, 100, 0)]),
        build("two.other_lanes", [(10, 60, 100, 0), (30, 55, 100, 0)]),
        build("two.same_lane_64_apart", [(10, 60, 100, 0), (73, 55, 100, 0)]),
        build("two.same_i", [(20, 60, 100, 1)]),
        build("best_at_1", [(0, 90, 100, 0), (50, 60, 100, 0), (51, 58, 100, 0)]),
        build("best_at_last", [(5, 60, 100, 0), (nv - 3, 90, 100, 0)]),
        build("second_in_holders_lane", [(10, 90, 100, 1), (30, 70, 100, 0), (50, 60, 100, 0)]),
        build("second_elsewhere", [(10, 90, 100, 1), (30, 88, 100, 0), (31, 60, 100, 0), (95, 87, 99, 1)]),
        build("crowded", [(j, 50 + (j * 37) % 41, 80 + (j * 11) % 17, j % 3 == 0) for j in range(0, 40)]),
    ]


# ------------------------------------------------------------------------------------------------ ties
def loci(scores, base=3000, step=500, dist=300, swap=False):
    """one FR candidate pair per (score of end 0's region, of end 1's) at loci too far apart to pair across; at distance avg its q is the sum"""
    a = [preg(base + step * t, 0, s0) for t, (s0, _) in enumerate(scores)]
    b = [preg(base + step * t + dist, 1, s1) for t, (_, s1) in enumerate(scores)]
    return (b, a) if swap else (a, b)


def tie_cases():
    out = []
    for rep in range(4):
        out.append(mk(f"ties.top2.{rep}", *loci([(100, 100)] * 2 + [(90, 100)] * 3, swap=rep & 1)))
        out.append(mk(f"ties.top3.{rep}", *loci([(80, 100)] * 3 + [(70, 100)] * 3, swap=rep & 1)))
        out.append(mk(f"ties.all40.{rep}", *loci([(75, 75)] * 40, swap=rep & 1)))
    return out


NP_TIES = {"0": 0, "2p23m1": 2 * (2 ** 23 - 1), "2p23": 2 * 2 ** 23, "2p31m4": 2 * (2 ** 31 - 4), "2p31": 2 * 2 ** 31, "2p40": 2 ** 40}


# ------------------------------------------------------------------------------------------------ n_sub
def nsub_cases(tmp=7):
    out = []
    for d in (-1, 0, 1):                                   # a third pair at subo - (tmp + d)
        side = (f"nsub.{tmp}", 1 - d, "n_sub") if d >= 0 else None
        out.append(mk(f"nsub.gap{tmp}{d:+d}", *loci([(100, 100), (100, 95), (100, 95 - tmp - d)]), side))
    for n in (0, 1, 63, 64, 65, 1000):                     # n_sub = the second and n - 1 more at exactly subo - tmp; five just beyond do not count
        sc = [(100, 100)] if n == 0 else [(100, 100), (100, 95)] + [(100, 95 - tmp)] * (n - 1) + [(100, 94 - tmp)] * 5
        out.append(mk(f"nsub.n{n}", *loci(sc)))
    return out


# ------------------------------------------------------------------------------------------------ the log table's end
def logtab_case(n0, n1):
    """n0 x n1 candidate pairs, every one within the window and all of one score: n_sub = n0 n1 - 1"""
    return mk(f"logtab.{n0}x{n1}", [preg(5000 + t % 60, 0, 70) for t in range(n0)], [preg(5300 + t % 61, 1, 70) for t in range(n1)])


# ------------------------------------------------------------------------------------------------ is_multi
def multi_cases(T=30):
    """End `e` holds j + 2 regions of falling scores (their order after marking is the input's), all but region j sharing the best one's
    span; region j scores T - 1 | T and has a span of its own (a second primary hit: is_multi once it reaches T) or shares (secondary)."""
    out = []
    for e in (0, 1):
        for j in (1, 63, 64, 65, 128, -1):
            for own in (1, 0):
                for d in (1, 0):
                    n = 130 if j < 0 else j + 2
                    jj = n - 1 if j < 0 else j
                    lst = []
                    for i in range(n):
                        s = T - d + (jj - i) if i <= jj else T - d - (i - jj)
                        lst.append(preg(10_000 + 1000 * i, 0, s, qb=200 if (i == jj and own) else 0, qe=300 if (i == jj and own) else 100))
                    mate = [preg(10_000 + 300, 1, 100)]
                    side = (f"multi.e{e}.j{j}.own{own}", 1 - d, "paired") if own else None
                    out.append(mk(f"multi.e{e}.j{j}.own{own}.T-{d}", lst if e == 0 else mate, mate if e == 0 else lst, side))
    return out


# ------------------------------------------------------------------------------------------------ paired or not, and the mapQ
WIDE = (1, 1000, 300.0, 30.0)                            # a window wide enough for a penalty of 50 and more


def dist_with_penalty(target, st=WIDE, a=1):
    """a distance whose pair scores exactly `target` below the sum of the two regions' scores"""
    for dist in range(int(st[2]), st[1] + 1):
        if q_of(100, 100, dist, st, a) - 200 == -target:
            return dist
    raise AssertionError(target)


def choice_cases(U=17):
    out = []
    for d in (-1, 0, 1):                                   # o - score_un = U - penalty
        if U - d < 0:
            continue                                     # (a pair never scores above the sum of its regions: with -U 0 the sign + is out of reach)
        for up in (0, 1):
            side = (f"choice.U{U}.up{up}", d, "flag") if d >= 0 and U >= 1 else None
            out.append(mk(f"choice.U{U}.o_un{d:+d}.up{up}", *pair_at(5000, dist_with_penalty(U - d), FR, up), side))
    for e in (0, 1):
        def ends(x, y):
            return (x, y) if e == 0 else (y, x)
        # the best pair takes a region that is not the end's best and is secondary to it: sub is adopted, the parent's family re-parented
        out.append(mk(f"choice.z_secondary.e{e}", *ends([preg(90_000, 0, 100), preg(5000, 0, 95), preg(91_000, 0, 90)], [preg(5300, 1, 100)])))
        # q_pe against q_se: a lone region (q_se 60) with a mate whose two candidates leave q_pe small; a region with a close second (q_se ~ 0)
        # and no second pair (q_pe 60: beyond q_se + 40); the same with a second pair a few points below (q_pe inside q_se + 40)
        out.append(mk(f"choice.q_pe_below.e{e}", *ends([preg(5000, 0, 100)], [preg(5300, 1, 100), preg(5310, 1, 99)])))
        out.append(mk(f"choice.q_pe_beyond.e{e}", *ends([preg(5000, 0, 100), preg(95_000, 0, 99)], [preg(5300, 1, 100)])))
        for gap in (2, 5, 8):
            out.append(mk(f"choice.q_pe_inside.gap{gap}.e{e}", *ends([preg(5000, 0, 100), preg(95_000, 0, 99)], [preg(5300, 1, 100), preg(5305, 1, 100 - gap)])))
        for csub in (0, 97, 95, 92, 50):
            out.append(mk(f"choice.csub{csub}.e{e}", *ends([preg(5000, 0, 100, csub=csub)], [preg(5300, 1, 100)])))
        for fr in (0.0, 0.3, 1.0):
            out.append(mk(f"choice.frac{fr}.e{e}", *ends([preg(5000, 0, 100, frac_rep=fr)], [preg(5300, 1, 100, frac_rep=0.3 if fr == 1.0 else 0.0)])))
            out.append(mk(f"choice.frac{fr}.second.e{e}", *ends([preg(5000, 0, 100, frac_rep=fr), preg(5010, 0, 97)], [preg(5300, 1, 100)])))
    return out


# ------------------------------------------------------------------------------------------------ re-parenting
def reparent_cases(parent_first=True):
    """End e: the best pair takes region zi of a list of n regions whose scores fall along the input; its parent is region 0 (every region
    shares region 0's span) or, with parent_first False, region 1 -- a second primary hit with a span of its own, which the flags of that
    set keep below T, and whose family is every odd region.  Families reach beyond index 64."""
    out = []
    for e in (0, 1):
        for n, zi in ((2, 1), (3, 2), (10, 7), (64, 63), (65, 64), (66, 65), (130, 129), (200, 3), (200, 131), (200, 199)):
            if not parent_first and n < 4:
                continue
            lst = []
            for i in range(n):
                own = (not parent_first) and i % 2 == 1
                lst.append(preg(5000 if i == zi else 50_000 + 1000 * i, 0, 240 - i, qb=200 if own else 0, qe=300 if own else 100))
            if not parent_first and zi % 2 == 0:
                continue
            mate = [preg(5300, 1, 100)]
            out.append(mk(f"reparent.{'k0' if parent_first else 'k1'}.e{e}.n{n}.z{zi}", lst if e == 0 else mate, mate if e == 0 else lst))
    return out


# ------------------------------------------------------------------------------------------------ ALT
def alt_cases(T=30):
    out = []
    for e in (0, 1):
        def ends(x, y):
            return (x, y) if e == 0 else (y, x)
        mate = [preg(5300, 1, 100)]
        fam = [preg(5000, 0, 100)] + [preg(60_000 + 1000 * i, 0, 95 - i) for i in range(4)]                       # z = 0 and four XA members of it
        out.append(mk(f"alt.printable.e{e}", *ends(fam + [preg(1000, 0, 80, rid=ALT_RID, qb=200, qe=300)], mate)))
        out.append(mk(f"alt.printable.xa.e{e}", *ends(fam + [preg(1000, 0, 80, rid=ALT_RID, qb=200, qe=300)] + [preg(2000 + 100 * i, 0, 78 - i, rid=ALT_RID, qb=200, qe=300) for i in range(3)], mate)))
        out.append(mk(f"alt.below_T.e{e}", *ends(fam + [preg(1000, 0, T - 1, rid=ALT_RID, qb=200, qe=300)], mate)))
        out.append(mk(f"alt.at_T.e{e}", *ends(fam + [preg(1000, 0, T, rid=ALT_RID, qb=200, qe=300)], mate)))
        out.append(mk(f"alt.secondary.e{e}", *ends(fam + [preg(1000, 0, 80, rid=ALT_RID)], mate)))
        out.append(mk(f"alt.on_top.e{e}", *ends(fam + [preg(1000, 0, 150, rid=ALT_RID)], mate)))
        # XA members owned by neither record: the family of a second primary hit below T
        other = [preg(70_000, 0, T - 1, qb=200, qe=300)] + [preg(71_000 + 1000 * i, 0, T - 2 - i, qb=200, qe=300) for i in range(3)]
        out.append(mk(f"alt.xa_of_neither.e{e}", *ends(fam + other + [preg(1000, 0, 80, rid=ALT_RID, qb=400, qe=500)], mate)))
        out.append(mk(f"alt.many_xa.e{e}", *ends([preg(5000, 0, 100)] + [preg(60_000 + 1000 * i, 0, 99 - i % 10) for i in range(7)], mate)))
        # no primary-assembly hit on this end: mem_pair is not called
        out.append(mk(f"alt.n_pri0.e{e}", *ends([preg(1000, 0, 80, rid=ALT_RID), preg(2000, 0, 70, rid=ALT_RID)], mate)))
        out.append(mk(f"alt.n_pri0.below_T.e{e}", *ends([preg(1000, 0, T - 1, rid=ALT_RID)], mate)))
    return out


# ------------------------------------------------------------------------------------------------ not paired
def unpaired_cases(T=30):
    out = []
    one = [preg(5000, 0, 100)]
    out.append(mk("unp.both_empty", [], []))
    out.append(mk("unp.empty0", [], one))
    out.append(mk("unp.empty1", one, []))
    for e in (0, 1):
        def ends(x, y):
            return (x, y) if e == 0 else (y, x)
        far = [preg(200_000, 1, 100)]                      # no candidate pair
        for d in (1, 0):
            out.append(mk(f"unp.best_T-{d}.e{e}", *ends([preg(5000, 0, T - d), preg(6000, 0, T - d - 1)], far), (f"unp.T.e{e}", 1 - d, "h")))
            # the best primary-assembly hit is below T: h comes from the first ALT region, if that reaches T
            out.append(mk(f"unp.alt_T-{d}.e{e}", *ends([preg(5000, 0, T - 1), preg(1000, 0, T - d, rid=ALT_RID, qb=200, qe=300)], far), (f"unp.altT.e{e}", 1 - d, "h")))
        out.append(mk(f"unp.secondaries.e{e}", *ends([preg(5000, 0, 100)] + [preg(6000 + 10 * i, 0, 99 - i) for i in range(8)], far)))
        out.append(mk(f"unp.two_primaries.e{e}", *ends([preg(5000, 0, 100), preg(9000, 0, 90, qb=150, qe=250)], [preg(5300, 1, 100)])))
    out.append(mk("unp.proper_candidate", *pair_at(5000, 300, FR, 0)))     # would pair, were pairing not switched off by the set's -P
    return out


# ------------------------------------------------------------------------------------------------ contigs and the ends of the reference
def contig_cases():
    out = []
    e0 = CTG_LEN[0]
    for up in (0, 1):
        def ends(x, y):
            return (x, y) if up == 0 else (y, x)
        # 300 bases apart on the forward strand of the reference, but on neighbouring contigs
        out.append(mk(f"ctg.neighbours.up{up}", *ends([preg(e0 - 100, 0, 100)], [preg(200, 1, 100, rid=1)])))
        # the scan from a candidate on contig 1 meets its partner there and then, at once, contig 0: break
        out.append(mk(f"ctg.break.up{up}", *ends([preg(e0 - 100, 0, 100), preg(50, 0, 90, rid=1)], [preg(350, 1, 100, rid=1)])))
        out.append(mk(f"ctg.break.better_beyond.up{up}", *ends([preg(e0 - 100, 0, 120), preg(50, 0, 90, rid=1)], [preg(350, 1, 100, rid=1)])))
        # first and last bases of a contig, the last contig (is_alt 0 on purpose, see the module's text)
        out.append(mk(f"ctg.first_last.up{up}", *ends([preg(0, 0, 100, rid=1)], [preg(300, 1, 100, rid=1)])))
        out.append(mk(f"ctg.last_contig.up{up}", *ends([preg(CTG_LEN[2] - 301, 0, 100, rid=2, is_alt=0)], [preg(CTG_LEN[2] - 1, 1, 100, rid=2, is_alt=0, rlen=1)])))
        # rb = l_pac - 1 (forward, downstream: FF), rb = l_pac (reverse, the same key: FR), rb = 2 l_pac - 1 (reverse, key 0 of contig 0, upstream: RF, RR)
        out.append(mk(f"ctg.rb_lpac-1.up{up}", *ends([preg(CTG_LEN[2] - 301, 0, 100, rid=2, is_alt=0)], [preg(CTG_LEN[2] - 1, 0, 100, rid=2, is_alt=0, rlen=1)])))
        out.append(mk(f"ctg.rb_lpac.both.up{up}", *ends([preg(CTG_LEN[2] - 301, 0, 100, rid=2, is_alt=0)],
                                                        [preg(CTG_LEN[2] - 1, 1, 100, rid=2, is_alt=0, rlen=1), preg(CTG_LEN[2] - 1, 0, 100, rid=2, is_alt=0, rlen=1)])))
        out.append(mk(f"ctg.rb_2lpac-1.rf.up{up}", *ends([preg(0, 1, 100, rlen=1)], [preg(300, 0, 100)])))
        out.append(mk(f"ctg.rb_2lpac-1.rr.up{up}", *ends([preg(0, 1, 100, rlen=1)], [preg(300, 1, 100)])))
    assert out[-1].a[0][0] == 2 * L_PAC - 1 or out[-1].b[0][0] == 2 * L_PAC - 1
    return out


# ------------------------------------------------------------------------------------------------ statistics nobody simulates
def pes_cases(st, dists):
    out = []
    for up in (0, 1):
        for dist in dists:
            out.append(mk(f"pes.dist{dist}.up{up}", *pair_at(5000, dist, FR, up)))
            out.append(mk(f"pes.dist{dist}.two.up{up}", *[x + y for x, y in zip(pair_at(5000, dist, FR, up), pair_at(5000 + min(max(1, dist // 2), 2000), dist, FR, up, 90, 90))]))
    return out


# ------------------------------------------------------------------------------------------------ random
def random_cases(n_pairs=300, seed=52):
    """Lists of 0 to 40 regions around three loci, both strands, spans of their own in a share that varies from pair to pair (a second
    primary hit above T ends the pairing), ALT regions, csub, sub_n and frac_rep at random."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_pairs):
        base = [int(rng.integers(2000, 500_000)) for _ in range(3)]
        p_own = float(rng.choice((0.0, 0.0, 0.03, 0.3)))
        ends = []
        for e in (0, 1):
            n = int(rng.integers(0, 41)) if rng.integers(0, 8) else 0
            lst = []
            for _ in range(n):
                ln = int(rng.integers(19, 151))
                own = rng.random() < p_own
                qb = int(rng.integers(0, 150)) if own else 0
                alt = int(rng.integers(0, 6) == 0)
                pos = int(rng.integers(100, 90_000)) if alt else base[int(rng.integers(0, 3))] + int(rng.integers(0, 700))
                score = int(rng.integers(19, 32)) if own and rng.integers(0, 2) else int(rng.integers(19, ln + 1))
                lst.append(preg(pos, int(rng.integers(0, 4) == 0) ^ e, score, rid=ALT_RID if alt else 0, qb=qb, qe=qb + ln,
                                csub=int(rng.integers(0, 19)) if rng.integers(0, 3) == 0 else 0, sub_n=int(rng.integers(0, 4)), frac_rep=float(rng.choice((0.0, 0.0, 0.1, 0.5)))))
            ends.append(lst)
        out.append(mk(f"random.{k}", *ends))
    return out


# ------------------------------------------------------------------------------------------------ the sets
extra = mc.extra
SETS = {}
for _d in range(4):
    SETS[f"window_{'ff fr rf rr'.split()[_d]}"] = Set([], extra(), 0, pes(*[WIN if k == _d else None for k in range(4)]), lambda _d=_d: window_cases(_d))
for _m in range(16):
    SETS[f"failed_{_m:04b}"] = Set([], extra(), 100, pes(*[None if _m >> k & 1 else WIN for k in range(4)]), failed_cases)
PEN_STATS = {"s30": (180, 420, 300.0, 30.0), "s7.3": (180, 420, 291.7, 7.3), "s1": (180, 420, 300.0, 1.0)}
for _a in (1, 2, 5):
    for _k, _st in PEN_STATS.items():
        SETS[f"penalty_A{_a}_{_k}"] = Set(["-A", str(_a)] if _a > 1 else [], extra(), 0, pes(fr=_st), lambda _a=_a, _st=_st: penalty_cases(_st, _a))
SETS["sizes"] = Set([], extra(), 40, PES_FR, size_cases)
SETS["lanes"] = Set([], extra(), 0, PES_FR, lane_cases)
for _k, _v in NP_TIES.items():
    SETS[f"ties_{_k}"] = Set([], extra(), _v, PES_FR, tie_cases)
SETS["nsub"] = Set([], extra(), 0, PES_FR, nsub_cases)
SETS["nsub_ab"] = Set(["-B", "9"], extra(), 0, PES_FR, lambda: nsub_cases(mc.tmp_of(b=9)))
SETS["nsub_del"] = Set(["-O", "8,2"], extra(), 0, PES_FR, lambda: nsub_cases(mc.tmp_of(o_del=8, o_ins=2)))
SETS["nsub_ins"] = Set(["-O", "2,8", "-E", "1,2"], extra(), 0, PES_FR, lambda: nsub_cases(mc.tmp_of(o_del=2, o_ins=8, e_ins=2)))
SETS["logtab"] = Set([], extra(), 0, PES_FR, lambda: [logtab_case(255, 257), logtab_case(3, 5)])
SETS["multi"] = Set([], extra(), 0, PES_FR, multi_cases)
for _u in (0, 17, 50):
    SETS[f"choice_U{_u}"] = Set(["-U", str(_u)], extra(), 0, pes(fr=WIDE), lambda _u=_u: choice_cases(_u))
SETS["reparent"] = Set(["-U", "500"], extra(), 0, PES_FR, reparent_cases)      # (-U: the pair with a low-scoring z[i] must still beat the two best regions unpaired)
SETS["reparent_k1"] = Set(["-U", "500", "-T", "300"], extra(), 0, PES_FR, lambda: reparent_cases(False))
SETS["alt"] = Set([], extra(), 0, PES_FR, alt_cases)
SETS["alt_a"] = Set(["-a"], extra(), 0, PES_FR, alt_cases)
SETS["unpaired"] = Set([], extra(), 0, PES_FR, unpaired_cases)
SETS["unpaired_P"] = Set(["-P"], extra(), 0, PES_FR, unpaired_cases)
SETS["contigs"] = Set([], extra(), 0, PES_ALL, contig_cases)
SETS["pes_std0"] = Set([], extra(), 0, pes(fr=(180, 420, 300.0, 0.0)), lambda: pes_cases(None, (299, 300, 301, 180, 420)))
SETS["pes_low_eq_high"] = Set([], extra(), 0, pes(fr=(300, 300, 300.0, 30.0)), lambda: pes_cases(None, (299, 300, 301)))
SETS["pes_2p20"] = Set([], extra(), 0, pes(fr=(1, 1 + (1 << 20), 300_000.0, 50_000.0)), lambda: pes_cases(None, (1, 2, 300_000, 450_000, 590_000)))
SETS["pes_all_failed"] = Set([], extra(), 0, pes(), lambda: pes_cases(None, (300,)))
PES_RANDOM = pes(ff=(100, 500, 300.0, 50.0), fr=WIN)
for _k, _f in {"": [], "_U0": ["-U", "0"], "_T10": ["-T", "10"], "_T60": ["-T", "60"], "_5": ["-5"], "_a": ["-a"], "_A2B3": ["-A", "2", "-B", "3"], "_O3,9_E1,4": ["-O", "3,9", "-E", "1,4"]}.items():
    SETS[f"random{_k}"] = Set(_f, extra(), 9000, PES_RANDOM, random_cases)

_built = {}


def cases_of(name):
    if name not in _built:
        _built[name] = SETS[name].build()
    return _built[name]


def bad_logtab_case():
    """256 x 256 candidate pairs: n_sub + 1 = 65536 is one beyond the log table.  GPU only: error 61, BWAHIP_EINTERNAL."""
    return logtab_case(256, 256)


def opt_of(name):
    """The bwahip option struct of a set: its flags, then the carried fields (BWAHIP_F_PE is implied by the entry)."""
    s = SETS[name]
    o, _ = common.opt_from_cli(s.flags)
    for k, v in s.extra.items():
        setattr(o, k, v)
    return o


def pes_of(name):
    p = (bw.PeStat * 4)()
    for d, (low, high, failed, avg, std) in enumerate(SETS[name].pes):
        p[d].low, p[d].high, p[d].failed, p[d].avg, p[d].std = low, high, failed, avg, std
    return p


def f64bits(x):
    return int(np.float64(x).view(np.int64))


# ------------------------------------------------------------------------------------------------ running them
def pack(cases):
    lists = [r for c in cases for r in (c.a, c.b)]
    off = np.cumsum([0] + [len(r) for r in lists]).astype(np.int64)
    regs = np.concatenate(lists) if lists else np.zeros((0, 19), np.int64)
    return off, regs


def case_words(name, cases=None):
    """The case file of `bwa_oracle katpair` / `bwaref katpair` (oracle/kat_pair_io.h) as int64 words."""
    s = SETS[name]
    cases = cases_of(name) if cases is None else cases
    e = s.extra
    o = opt_of(name)
    head = [mc.f32bits(e["mask_level"]), mc.f32bits(e["mapQ_coef_len"]), e["mapQ_coef_fac"], mc.f32bits(e["XA_drop_ratio"]), mc.f32bits(e["drop_ratio"]), s.n_processed,
            int(o.pen_unpaired), int(o.flag) | 0x2]
    for low, high, failed, avg, std in s.pes:
        head += [low, high, failed, f64bits(avg), f64bits(std)]
    w = [np.array([TAG_OPT, len(head)] + head, np.int64)]
    for p, c in enumerate(cases):
        for e_, r in enumerate((c.a, c.b)):
            w += [np.array([bw.TAG_READ, 2, 2 * p + e_, 0, TAG_REGS, 1 + r.size, len(r)], np.int64), r.ravel()]
    return np.concatenate(w)


def input_digest(name):
    return hashlib.sha256(case_words(name).tobytes() + " ".join(SETS[name].flags).encode()).hexdigest()


def run_checker(exe, name, prefix, workdir, tag="c"):
    """-> per read the dict of its answer records (TAG_MARKED, and from the oracle TAG_PAIR; with the even reads TAG_MEMPAIR, TAG_EXTRA)."""
    fin, fout = os.path.join(workdir, f"{tag}.{name}.in.bin"), os.path.join(workdir, f"{tag}.{name}.out.bin")
    case_words(name).tofile(fin)
    subprocess.check_call([exe, "katpair", *SETS[name].flags, prefix, fin, fout])
    reads = common.by_read(bw.read_record_file(fout))
    assert len(reads) == 2 * len(cases_of(name))
    os.remove(fin)
    os.remove(fout)
    return reads


def body(rec):
    return rec[HDR:].reshape(-1, W)


def shared_words(n_npri_regs0, n_npri_regs1, mempair3):
    """What the reference gives and the device gives too, of one pair: per end n, n_pri and the marked regions in their final order without
    the three words mem_sam_pe goes on to change (sub, secondary, secondary_all), then mem_pair's ret, sub and n_sub."""
    out = []
    for n, n_pri, regs in (n_npri_regs0, n_npri_regs1):
        r = np.array(regs, dtype=np.int64).reshape(-1, 19).copy()
        r[:, [C_SUB, C_SEC, C_SECALL]] = 0
        out += [np.array([n, n_pri], np.int64), r.ravel()]
    out.append(np.array(mempair3, dtype=np.int64))
    return np.concatenate(out)


def digests_of_checker(reads):
    """per pair the sha256 of its shared words, from the records of `bwaref katpair` (or of the oracle): what kat_pair.npz holds"""
    out = []
    for p in range(len(reads) // 2):
        m0, m1 = reads[2 * p][TAG_MARKED], reads[2 * p + 1][TAG_MARKED]
        out.append(hashlib.sha256(shared_words((m0[0], m0[1], m0[2:]), (m1[0], m1[1], m1[2:]), reads[2 * p][TAG_MEMPAIR][:3]).tobytes()).digest())
    return np.array(out, dtype="S32")


def digests_of_device(recs):
    """the same from bwahip_kat_pair's records (per read the KAT_PAIR_TAG array)"""
    out = []
    for p in range(len(recs) // 2):
        r0, r1 = recs[2 * p], recs[2 * p + 1]
        out.append(hashlib.sha256(shared_words((r0[H_N], r0[H_NPRI], body(r0)[:, :19]), (r1[H_N], r1[H_NPRI], body(r1)[:, :19]), r0[H_O:H_O + 3]).tobytes()).digest())
    return np.array(out, dtype="S32")


def outcome(reads, p, kind):
    """What the case on one side of a threshold must differ in from the case on the other side (from the oracle's records of pair p)."""
    r0, r1 = reads[2 * p][TAG_PAIR], reads[2 * p + 1][TAG_PAIR]
    if kind == "paired":
        return int(r0[H_MODE])
    if kind == "flag":
        return int(r0[H_FLAG]), int(r1[H_FLAG])
    if kind == "n_sub":
        return int(r0[H_NSUB])
    if kind == "h":
        return int(r0[H_HREG]), int(r1[H_HREG])
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
