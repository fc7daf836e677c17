"""Region lists built on purpose for mem_sort_dedup_patch (bwamem.c:444-496, mem_patch_reg bwamem.c:413) and the is_alt marking of
bwamem.c:1091-1095, fed to bwahip_kat_dedup (the dedup kernels of csrc/k_extend.hip: k_dedup_fast, k_dedup with the list in LDS or in global
memory, the slab form), to `bwa_oracle katdedup` (ora_kat_dedup) and, where it is built, to `bwaref katdedup` (the reference's own function).
Deterministic: every list comes from a seed that is part of its name.  Over the committed 60 kb genome tests/golden/g60k.fa.gz with ctg3
declared ALT: ctg1 [0, 40000), ctg2 [40000, 56000) (no N: the patch queries are cut from it), ctg3 [56000, 60000); l_pac = 60000.

Every region carries a value of its own in the fields the function never reads and the device carries (seedlen0, sub_n, the bits of frac_rep),
so a record moved to the wrong place or merged into the wrong neighbour shows up; alt_sc, secondary and secondary_all are not part of the
device's region record and are 0.  All 19 words are compared, nothing is masked.

A patch query is two flanks cut from ctg2 with g bases of the reference left out (a deletion) or g random bases put in (an insertion)
between them and m substitutions in the second flank: the global score is then (matches) - 5 m - (6 + g) with the default scores, and
the case lands where it is meant to.  The one case left out: bwa_gen_cigar2 returning without a score (a window across l_pac or an empty
query) -- the reference reads an uninitialised int there; bwahip_kat_dedup refuses such regions.

Two things the function cannot show, whatever the list (reasons in build_reach and below): a difference between the two sides of the
reach test under the default max_chain_gap and the default -w, and a tie in (score, rb, qb) at the second sort under mask_level_redun < 1.  Two regions with
the same rb and qb overlap each other fully on both axes (orr = the shorter's length = mr, oq >= mq), are within reach of each other, and
so one of them is always excluded before the second sort; a merge gives p the rb and qb of a q that is then gone, and two q with the same
start have excluded each other before.  Ties at the second sort therefore come from the sets under mask_level_redun 1.0 only.

What the sets cover is stated per builder."""
import gzip
import hashlib
import itertools
import os
import random
import subprocess
from types import SimpleNamespace as NS

import numpy as np

import common
from common import bw

NW = 19
C_RB, C_RE, C_QB, C_QE, C_RID, C_SCORE, C_TRUESC, C_SUB, C_CSUB, C_SUBN, C_W, C_SEEDCOV, C_SEEDLEN0, C_NCOMP, C_ISALT, C_FRAC = 0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 15, 16, 17, 18
TAG_OPT, TAG_SEQ, TAG_OUT, TAG_REGS = 42, 43, 44, 4
STAT_N = 9
S_EXCL_P, S_EXCL_Q, S_ALIGN, S_MERGE, S_RATIO, S_KEPT, S_IDENT, S_FLAGS, S_WHY = range(STAT_N)
F_COMB1, F_COMB2, F_TIE1 = 1, 2, 4
WHY = dict(strand=1, qb=2, qe=4, re=8, gap_w=16, gap_r=32, ovl_w=64, ovl_r=128, ratio=256)
L_PAC = 60000
CTG = {0: (0, 40000), 1: (40000, 56000), 2: (56000, 60000)}
FAST_N, STAGE_N = 8, 32
MAXT = 700 + 2 * 200 + 1024                                      # k_extend.hip: the compiled LDS window


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


_genome = None


def genome():
    """The forward strand as codes 0..3 (N: 4), contigs concatenated in file order."""
    global _genome
    if _genome is None:
        txt = gzip.open(os.path.join(common.GOLDEN, "g60k.fa.gz"), "rt").read().split(">")[1:]
        s = "".join("".join(c.split("\n")[1:]) for c in txt).upper()
        assert len(s) == L_PAC
        _genome = np.array([{"A": 0, "C": 1, "G": 2, "T": 3}.get(ch, 4) for ch in s], dtype=np.uint8)
    return _genome


def make_index(workdir):
    """The g60k index with its ALT list, built where the test modules' module-scoped fixtures ask for it."""
    fa = os.path.join(workdir, "g60k.fa")
    open(fa, "wb").write(gzip.open(os.path.join(common.GOLDEN, "g60k.fa.gz")).read())
    bw.make_index(fa, os.path.join(workdir, "g60k"))
    open(os.path.join(workdir, "g60k.alt"), "wb").write(open(os.path.join(common.GOLDEN, "g60k.alt"), "rb").read())
    return os.path.join(workdir, "g60k")


def reg(rb, re, qb, qe, score, rid=None, w=0, **kw):
    if rid is None:
        lo = rb if rb < L_PAC else 2 * L_PAC - re
        rid = next(k for k, (a, b) in CTG.items() if a <= lo < b)
    d = dict(rb=rb, re=re, qb=qb, qe=qe, rid=rid, score=score, w=w, sub=0, csub=0, seedcov=min(re - rb, qe - qb) >> 1)
    d.update(kw)
    return d


def words(r, tag):
    return [r["rb"], r["re"], r["qb"], r["qe"], r["rid"], r["score"], r.get("truesc", r["score"]), r["sub"], 0, r["csub"], (tag * 7) % 1009 + 1, r["w"],
            r["seedcov"], 0, 0, 1000 + tag, 0, 0, f32bits((tag + 1) / 4096.0)]


class Case:
    def __init__(self, name, seq, regs, heavy=False, side=None, rlen=None, expect=None):
        """regs: dicts in the order the list is handed over in; side: (pair name, 0 or 1) for the two sides of a threshold; rlen: the
        reference window of the patch the case is built around (hand-over prediction); expect: dict of judge counts the case is built for."""
        self.name, self.seq, self.heavy, self.side, self.rlen, self.expect = name, np.asarray(seq, dtype=np.uint8), heavy, side, rlen, expect or {}
        self.regs = np.array([words(r, t) for t, r in enumerate(regs)], dtype=np.int64).reshape(-1, NW)
        assert len(self.regs) >= 2


def rand_seq(rng, n):
    return np.array([rng.randrange(4) for _ in range(n)], dtype=np.uint8)


def mirror(case_name, seq, regs, **kw):
    """The same list on the reverse strand: the query reverse-complemented, every region at its mirror image."""
    n = len(seq)
    s2 = np.where(seq[::-1] < 4, 3 - seq[::-1], 4).astype(np.uint8)
    r2 = [dict(r, rb=2 * L_PAC - r["re"], re=2 * L_PAC - r["rb"], qb=n - r["qe"], qe=n - r["qb"]) for r in regs]
    return Case(case_name, s2, r2, **kw)


# ------------------------------------------------------------------------------------------------ sizes
SIZES = [2, 3, 8, 9, 32, 33, 63, 64, 65, 128, 129, 255, 256, 257, 383, 384, 2048, 2049, 3000]


def size_list(n, tie_re, tie_sc, falling, score_falling, cluster, seed):
    """n regions of 8 bases on ctg1 with max_chain_gap 3.  far: 12 apart, so every entry fails the reach test (rb = previous re + 4);
    cluster: groups of 16 that start one base apart, the groups beginning at indices 11, 27, ... so that entries 64 and 128 sit inside
    one (a long list in one cluster costs n^2 sequential steps on one wavefront: the groups keep a 3 000-region list within the time of
    a test).  tie_re: every second region ends where its predecessor ends (one base shorter); tie_sc (with mask_level_redun 1.0, under
    which regions with the same start are never redundant): every third region repeats the (score, rb, qb) of its predecessor with
    another end.  Scores are distinct otherwise and rise or fall with re (score_falling); the list is handed over in rising or falling
    re order (falling)."""
    rng = random.Random(seed)
    out, pos = [], 100
    for k in range(n):
        if cluster and (k + 5) % 16:
            pos += 1
        elif k:
            pos += 12
        qb = (k * 37) % 140
        r = reg(pos, pos + 8, qb, qb + 8, 1000 + (n - k if score_falling else k), rid=0)
        if tie_re and k % 2 and out:
            p = out[-1]
            r.update(rb=p["rb"] + 1, re=p["re"], qe=qb + 7)
            pos = p["rb"]
        if tie_sc and k % 3 == 2 and out:
            p = out[-1]
            r.update(rb=p["rb"], re=p["re"] + 1, qb=p["qb"], qe=p["qe"] + 1, score=p["score"])
            pos = p["rb"]
        out.append(r)
    if falling:
        out.reverse()
    return Case(f"n{n}_{'t' if tie_re else ''}{'s' if tie_sc else ''}_{'fall' if falling else 'rise'}_{'sf' if score_falling else 'sr'}_{'clu' if cluster else 'far'}_{seed}",
                rand_seq(rng, 150), out, heavy=n > 256)


def build_sizes(tie_sc):
    def build():
        cs = []
        for n in SIZES:
            for v in range(16):
                tie_re, falling, score_falling, cluster = bool(v & 1), bool(v & 2), bool(v & 4), bool(v & 8)
                if n > 384 and v not in (0, 15):
                    continue                                     # the three longest: two variants each
                cs.append(size_list(n, tie_re, tie_sc, falling, score_falling, cluster, len(cs)))
        rng = random.Random(5)
        for n in (17, 40, 100, 300, 700):                        # shuffled hand-over order with ties: the quicksort phase proper
            c = size_list(n, True, tie_sc, False, False, True, 900 + n)
            perm = list(range(n))
            rng.shuffle(perm)
            cs.append(Case(c.name + "_shuf", c.seq, [_undict(c.regs[i]) for i in perm]))
        return cs
    return build


def _bare(c):
    """The same list without the expectations it was built for under its own set's options."""
    d = Case.__new__(Case)
    d.__dict__.update(c.__dict__, side=None, expect={})
    return d


def _undict(w):
    return dict(rb=int(w[C_RB]), re=int(w[C_RE]), qb=int(w[C_QB]), qe=int(w[C_QE]), rid=int(w[C_RID]), score=int(w[C_SCORE]), w=int(w[C_W]),
                sub=int(w[C_SUB]), csub=int(w[C_CSUB]), seedcov=int(w[C_SEEDCOV]))


# ------------------------------------------------------------------------------------------------ redundancy
def build_redun(mask):
    """Two regions p (later end) and q: orr and oq one base either side of mask * mr and mask * mq (each conjunct failing alone, both
    holding), lengths whose float product is inexact among them; p.score < q.score against equal scores (with equal scores q goes);
    an excluded q skipped by a later p; p excluded after it has excluded an earlier q; three mutually redundant regions in every score
    order.  Queries are random: where a pair is not redundant and passes mem_patch_reg's pre-tests, the alignment runs and fails the ratio."""
    def build():
        rng = random.Random(int(mask * 100))
        cs = []
        for ln in (20, 37, 100, 133, 139):                       # 0.95 * 37, 0.3 * 133 ... are inexact in float
            thr = float(np.float32(mask) * np.float32(ln))       # the comparison is (float)orr > mask * (float)mr in float
            ov = int(np.floor(thr))                              # largest overlap that is NOT > thr; ov + 1 is
            for dr in (0, 1):
                for dq in (0, 1):
                    q = reg(1000, 1000 + ln, 5, 5 + ln, 50)
                    # p starts so that orr = q.re - p.rb = ov + dr; its query part so that oq = q.qe - p.qb = ov + dq (q.qb < p.qb)
                    p = reg(1000 + ln - (ov + dr), 1000 + 2 * ln - (ov + dr), 5 + ln - (ov + dq), 5 + 2 * ln - (ov + dq), 60)
                    cs.append(Case(f"thr_l{ln}_r{dr}q{dq}", rand_seq(rng, 300), [q, p], side=(f"thr_l{ln}", dr & dq) if dr == dq else None))
        base = [reg(2000, 2100, 0, 100, 50), reg(2002, 2102, 2, 102, 50)]
        for sp, sq in ((49, 50), (50, 50), (51, 50)):
            cs.append(Case(f"score_p{sp}_q{sq}", rand_seq(rng, 150), [dict(base[0], score=sq), dict(base[1], score=sp)],
                           side=("score", 0 if sp < sq else 1) if sp != 51 else None))
        # p1 (score 80, 38 query bases) excludes q0 (score 70).  p2 (score 60) shares 36 query bases with p1: not redundant at 0.95 (36.1 are
        # needed; at 0.5 and 0.3 it would be, so the case is built for 0.95 only), and mem_patch_reg refuses the pair on r.  p2 is redundant
        # with q0, whose score is higher: only the skip of the excluded q0 keeps p2 in the list.
        skip = [reg(3000, 3100, 0, 100, 70), reg(3001, 3101, 1, 39, 80), reg(3002, 3102, 3, 103, 60)]
        if mask >= 0.95:
            cs.append(Case("skip_excluded_q", rand_seq(rng, 150), skip, expect=dict(n=2, excl=1, align=0)))
        # p (score 50, last end) excludes qB (40) next to it and goes on to qA (90), which excludes p: one region is left
        cs.append(Case("p_after_excluding", rand_seq(rng, 150), [reg(3000, 3100, 0, 100, 90), reg(3001, 3101, 1, 101, 40), reg(3002, 3102, 2, 102, 50)],
                       expect=dict(n=1, excl=2)))
        for perm in itertools.permutations((40, 50, 60)):
            cs.append(Case("three_" + "_".join(map(str, perm)), rand_seq(rng, 150), [reg(4000 + k, 4100 + k, k, 100 + k, s) for k, s in enumerate(perm)]))
        cs.append(Case("three_equal", rand_seq(rng, 150), [reg(4000 + k, 4100 + k, k, 100 + k, 50) for k in range(3)]))
        return cs
    return build


# ------------------------------------------------------------------------------------------------ reach
def reach_list(gap, d, pre, fill, x=2000):
    """Two flanks of 100 bases cut from one stretch of ctg2 with gap - d bases between them, in the reference and in the query alike: the
    second flank p starts at q.re + gap - d.  In reach (d = 1) mem_patch_reg finds w = 0 and r = 0, the window equals the query and the
    pair merges into one region of 200 + gap - 1; at d = 0 the inner loop ends at q and both stay.  `pre` far-apart regions of ctg1 in
    front of q and `fill` short regions that end between q.re and p.re (in reach by their order, never redundant, refused by
    mem_patch_reg on q.qb >= p.qb) put q at index `pre` and p at index pre + 1 + fill of the sorted list."""
    G = genome()
    g = gap - d
    x += 40000
    L = 200 + g
    rng = random.Random(gap * 7 + d + pre * 131 + fill)
    q = np.concatenate([G[x:x + L], rand_seq(rng, 20)])
    regs = [reg(100 + 160 * k, 200 + 160 * k, 0, 100, 30 + k, rid=0) for k in range(pre)]
    regs.append(reg(x, x + 100, 0, 100, 100, sub=2, csub=6))
    E = x + 100
    assert fill <= g + 90
    regs += [reg(E + 1 + k - 8, E + 1 + k, L + 2, L + 10, 8) for k in range(fill)]
    regs.append(reg(E + g, E + g + 100, 100 + g, L, 100, sub=5, csub=1))
    return q, regs, L


def build_reach(gap):
    """What the reach test p.rb < a[j].re + max_chain_gap can decide.  The list is sorted by re, so a[j].re falls as j falls: once an entry is
    out of reach all farther ones are, the test against a[i-1] in front of the loop decides nothing the loop's own test does not, and an
    entry that overlaps another (the only way to be redundant) is always in reach.  The threshold therefore shows only through
    mem_patch_reg, on a pair with max_chain_gap - 1 bases between its two regions -- which, under the default -w, mem_patch_reg refuses
    for w > opt.w << 1 at the default gap of 10 000, whatever the query of at most 700 bases (a -w of several thousand would let it
    through): there the two sides are told apart by the judge's count alone, and under -G 50 by a merge.  Under -G 50: the pair alone; the same pair at index 64, 65, 128 and 129 of the list with its partner at 63, 0,
    127, 63 and 1 -- in the block of 64 before it and two blocks back, which the reach test evaluated ahead of time must get right.
    Both: a contig change between neighbours that would merge inside one contig."""
    def build():
        rng = random.Random(gap)
        cs = []
        G = genome()
        if gap <= 200:
            for at, partner in ((1, 0), (64, 63), (65, 63), (64, 0), (128, 127), (128, 63), (129, 1)):
                for d in (0, 1):
                    q, regs, L = reach_list(gap, d, partner, at - partner - 1)
                    cs.append(Case(f"idx{at}_partner{partner}_G{gap}_d{d}", q, regs, rlen=L, side=(f"reach_{at}_{partner}", d),
                                   expect=dict(align=d, merge=d)))
        else:
            for d in (0, 1):                                     # in reach the pair gets as far as mem_patch_reg's w test: seen by the judge only
                cs.append(Case(f"reach_G{gap}_d{d}", rand_seq(rng, 150), [reg(100, 200, 0, 100, 50), reg(200 + gap - d, 300 + gap - d, 40, 140, 60)],
                               expect=dict(align=0, **({"why": "gap_w"} if d else {}))))
        # the last 100 bases of ctg1 and the first 100 of ctg2 against the same geometry inside ctg2: one diagonal, adjacent, a merge by the shortcut
        for name, x in (("contig_change", 39900), ("contig_same", 44900)):
            cs.append(Case(f"{name}_G{gap}", G[x:x + 200], [reg(x, x + 100, 0, 100, 100), reg(x + 100, x + 200, 100, 200, 100)], rlen=200,
                           side=("contig", 0 if name == "contig_change" else 1), expect=dict(merge=0 if name == "contig_change" else 1)))
        return cs
    return build


# ------------------------------------------------------------------------------------------------ patch
def patch_case(name, x, l1, l2, g, m=0, ins=False, nmid=False, qlen=None, w1=0, w2=0, lead=0, rev=False, extra=None, sc1=None, sc2=None, **kw):
    """Flank 1 = ctg2[x, x + l1), flank 2 = the l2 bases behind it with g reference bases skipped (deletion) or g random bases put into the
    query (insertion); m substitutions in flank 2; `lead` random bases in front; the query is padded to qlen with random bases."""
    G = genome()
    rng = random.Random(hash((x, l1, l2, g, m, ins)) & 0xffff)
    x += 40000
    f1 = G[x:x + l1]
    r2 = x + l1 + (0 if ins else g)
    f2 = G[r2:r2 + l2].copy()
    assert f1.max() < 4 and f2.max() < 4
    for k in rng.sample(range(5, l2 - 5), m):
        f2[k] = (f2[k] + 1 + rng.randrange(3)) % 4
    mid = (np.full(g, 4, np.uint8) if nmid else rand_seq(rng, g)) if ins else np.zeros(0, np.uint8)
    q = np.concatenate([rand_seq(rng, lead), f1, mid, f2])
    if qlen:
        assert qlen >= len(q)
        q = np.concatenate([q, rand_seq(rng, qlen - len(q))])
    qb2 = lead + l1 + len(mid)
    regs = [reg(x, x + l1, lead, lead + l1, l1 if sc1 is None else sc1, w=w1, sub=3, csub=5),
            reg(r2, r2 + l2, qb2, qb2 + l2, l2 - 5 * m if sc2 is None else sc2, w=w2, sub=7, csub=2)] + (extra or [])
    rlen = r2 + l2 - x
    return mirror(name, q, regs, rlen=rlen, **kw) if rev else Case(name, q, regs, rlen=rlen, **kw)


def build_patch():
    """Accepted patches and every refusal, on both strands.  With flanks of 70 and the default scores a gap of g costs 6 + g: the merged
    score is 140 - 6 - g against max(q_s, r_s) = 140 + g, so g = 4 merges (130 / 144 = 0.9028) and g = 5 does not (129 / 145 = 0.8897) --
    once with r_s the larger (deletion) and once with q_s (insertion).  Overlapping flanks on one diagonal take the shortcut (w == 0,
    lq == rlen); the same pair with q.w = 1 goes through the DP.  Queries of 150, 250, 300 and 600 bases reach k_dedup<3|4|5|11>."""
    cs = []
    for rev in (False, True):
        s = "r" if rev else "f"
        for ins in (False, True):
            for g in (1, 3, 4, 5, 8):
                cs.append(patch_case(f"{s}_{'ins' if ins else 'del'}{g}", 1000 + 37 * g, 70, 70, g, ins=ins, rev=rev, qlen=150,
                                     side=(f"ratio_{s}_{'ins' if ins else 'del'}", 0 if g == 4 else 1) if g in (4, 5) else None,
                                     expect=dict(align=1, merge=1 if g <= 4 else 0) if g < 8 else dict(why="gap_r", align=0)))   # 8 / 148 = 0.054
        for m in (0, 1, 2, 3):                                   # 200 - 5m - 7 against 201: 0.96, 0.935, 0.91, 0.886
            cs.append(patch_case(f"{s}_sub{m}", 3000, 100, 100, 1, m=m, rev=rev, qlen=250, sc2=100, expect=dict(align=1, merge=1 if m <= 2 else 0)))
        for qlen, x in ((150, 5000), (250, 5200), (300, 5400), (600, 5600)):
            cs.append(patch_case(f"{s}_len{qlen}", x, 60, 60, 2, rev=rev, qlen=qlen, lead=qlen - 125, expect=dict(align=1, merge=1)))
        # one diagonal, overlapping by 20: the shortcut, and the DP with q.w = 1
        G = genome()
        for w1 in (0, 1):
            q = G[46000:46140]
            regs = [reg(46000, 46080, 0, 80, 80, w=w1, sub=1, csub=9), reg(46060, 46140, 60, 140, 80, sub=4, csub=4)]
            cs.append((mirror if rev else Case)(f"{s}_diag_w{w1}", q, regs, rlen=140, expect=dict(align=1, merge=1)))
        # two and three merges into one p: three / four flanks on one diagonal with small deletions between them
        for k in (3, 4):
            parts, regs, pos, qpos = [], [], 47000, 0
            for t in range(k):
                parts.append(G[pos:pos + 60])
                regs.append(reg(pos, pos + 60, qpos, qpos + 60, 60, sub=t, csub=10 - t, w=t))
                pos += 62; qpos += 60
            cs.append((mirror if rev else Case)(f"{s}_merge{k - 1}", np.concatenate(parts), regs, rlen=pos - 2 - 47000, expect=dict(merge=k - 1)))
        # every refusal alone (the pair is otherwise the g = 3 deletion that merges)
        base = dict(x=7000, l1=70, l2=70, g=3, qlen=150, rev=rev)
        c = patch_case(f"{s}_ref_ok", **base, expect=dict(merge=1))
        cs.append(c)
        q0, p0 = _undict(c.regs[0]), _undict(c.regs[1])
        if rev:
            q0, p0 = p0, q0                                      # (on the reverse strand the second flank has the smaller rb)
        for why, dq, dp in (("qb", dict(qb=p0["qb"] + 1, qe=p0["qe"] - 1), {}), ("qe", dict(qe=p0["qe"]), {}), ("re", dict(re=p0["re"], rb=q0["rb"] - 10), {})):
            cs.append(Case(f"{s}_ref_{why}", c.seq, [dict(q0, **dq), dict(p0, **dp)], expect=dict(why=why, align=0)))
        cs.append(patch_case(f"{s}_ref_gap_w", 8000, 70, 70, 1201, qlen=150, rev=rev, expect=dict(why="gap_w", align=0)))
        cs.append(patch_case(f"{s}_ref_gap_r", 9000, 70, 70, 9, qlen=150, rev=rev, expect=dict(why="gap_r", align=0)))      # 9 / 149 = 0.060
        cs.append(patch_case(f"{s}_gap_r_in", 9000, 70, 70, 7, qlen=150, rev=rev, expect=dict(align=1, merge=0)))           # 7 / 147 = 0.048
    # N's in the gap: 3 bases of the query between the flanks that match nothing
    for rev in (False, True):
        cs.append(patch_case(f"{'r' if rev else 'f'}_ngap3", 6000, 70, 70, 3, ins=True, nmid=True, qlen=150, rev=rev, expect=dict(align=1, merge=1)))
    # a merge moves p.rb and p.qb to q's; z, which ends behind p, covers p on the reference either way but shares query bases only with the
    # q part: redundant with the merged p alone.  Its score is higher, so the merged region goes and z stays by itself.
    c = patch_case("merge_then_redundant", 6500, 70, 70, 3, qlen=150)
    q0, p0 = _undict(c.regs[0]), _undict(c.regs[1])
    z = reg(q0["rb"] + 2, p0["re"] + 1, 0, 66, 300)
    cs.append(Case("merge_then_redundant", c.seq, [p0, z, q0], rlen=c.rlen, expect=dict(align=1, merge=1, excl=1, n=1)))
    cs.append(Case("merge_then_redundant_twin", c.seq, [p0, dict(z, qb=80, qe=146), q0], rlen=c.rlen, expect=dict(merge=1, excl=0)))
    # a forward and a reverse region of ctg3 within reach of each other: the strand refusal
    rng = random.Random(77)
    # the overlap branch (q.re >= p.rb and q.qe >= p.qb) beyond its w limit: 500 bases of overlap on the reference, 50 on the query
    cs.append(Case("ref_ovl_w", rand_seq(rng, 150), [reg(41000, 41600, 0, 100, 90), reg(41100, 41700, 50, 150, 95)], expect=dict(why="ovl_w", align=0)))
    for k in range(12):
        cs.append(Case(f"ref_strand{k}", rand_seq(rng, 150), [reg(59800 - 7 * k, 59900 - 7 * k, 0, 100, 50, rid=2), reg(60050 + 11 * k, 60150 + 11 * k, 40, 140, 60, rid=2)],
                       expect=dict(why="strand", align=0)))
    return cs


# ------------------------------------------------------------------------------------------------ the limits of mem_patch_reg
def limit_pair(name, dr, dq, R, Q, side=None, expect=None, X=42000):
    """Regions q and p with q.re - p.rb = dr, q.qe - p.qb = dq, p.re - q.rb = R and p.qe - q.qb = Q: mem_patch_reg's w = |dr - dq| and
    r = |dr / R - dq / Q| (in double).  The regions are input, not alignments: the reference spans may be many times the query's."""
    a = (R + dr) // 2
    c = (Q + dq) // 2
    q, p = reg(X, X + a, 0, c, 40), reg(X + a - dr, X + R, c - dq, Q, 45)
    assert q["rb"] < p["rb"] and q["re"] < p["re"] and q["qb"] < p["qb"] and q["qe"] < p["qe"] and Q <= 150
    return Case(name, rand_seq(random.Random(R * 31 + Q), 150), [q, p], side=side, rlen=R, expect=expect)


def build_limits():
    """w at opt.w << 1 and one above in the gap branch (q.re < p.rb), at opt.w << 2 and one above in the overlap branch; r either side of
    0.05f and of 2 * 0.05f.  The constant is a float compared in double: 10 / 200 is 0.05000000000000000277 in double, below
    (double)0.05f = 0.0500000007450580597, so the pair passes -- with the constant written as a double it would not --, and 20 / 200 passes
    below (double)(0.05f * 2) = 0.100000001490116119 likewise; 10 / 199 and 20 / 199 are refused.  (The queries are random: an alignment
    that runs fails the ratio.)  The band min(w + q.w + p.w, opt.w << 2) at 399, 400, 401 and 500 on a pair that merges: the merged
    region's w is the band."""
    assert float(np.float32(0.05)) > 10 / 200 >= 0.05 and float(np.float32(0.05) * np.float32(2)) > 20 / 200 >= 0.1
    cs = [limit_pair("gap_w200", -220, -20, 660, 60, ("gap_w", 1), dict(align=1)), limit_pair("gap_w201", -221, -20, 661, 60, ("gap_w", 0), dict(align=0, why="gap_w")),
          limit_pair("ovl_w400", 410, 10, 1640, 40, ("ovl_w", 1), dict(align=1)), limit_pair("ovl_w401", 411, 10, 1644, 40, ("ovl_w", 0), dict(align=0, why="ovl_w")),
          limit_pair("gap_r_at_0.05", -10, 0, 200, 100, ("gap_r", 1), dict(align=1)), limit_pair("gap_r_above", -10, 0, 199, 100, ("gap_r", 0), dict(align=0, why="gap_r")),
          limit_pair("ovl_r_at_0.1", 20, 0, 200, 100, ("ovl_r", 1), dict(align=1)), limit_pair("ovl_r_above", 20, 0, 199, 100, ("ovl_r", 0), dict(align=0, why="ovl_r"))]
    for rev in (False, True):
        for w1, band in ((196, 399), (197, 400), (198, 400), (297, 400)):
            cs.append(patch_case(f"{'r' if rev else 'f'}_band_{w1 + 203}", 10000, 70, 70, 3, qlen=150, w1=w1, w2=200, rev=rev,
                                 side=(f"band_{'r' if rev else 'f'}", band - 399) if w1 in (196, 197) else None, expect=dict(merge=1, w=band)))
    return cs


# ------------------------------------------------------------------------------------------------ what k_dedup_fast must refuse
def build_fast():
    """Lists of 2 to 8: far-away bystanders plus a pair that is, alone: clean (k_dedup_fast finishes it); a tie in re (a tie in (score, rb,
    qb) among the survivors needs mask_level_redun 1.0: build_fast_m1); a patch candidate whose alignment fails the ratio (refused all
    the same, and the full form must not merge); one that merges; and, from 3 regions on, a patch candidate behind an excluded q, which
    must NOT refuse, beside the same list with the q not excluded, which must."""
    cs = []
    rng = random.Random(8)
    for n in range(2, 9):
        by = [reg(20000 + 400 * k, 20100 + 400 * k, 5, 105, 30 + k, rid=0) for k in range(n - 2)]
        cs.append(Case(f"clean_n{n}", rand_seq(rng, 150), [reg(100, 200, 0, 100, 50), reg(150, 260, 30, 140, 60)] + by, expect=dict(taker="fast")))
        cs.append(Case(f"tie_re_n{n}", rand_seq(rng, 150), by + [reg(100, 200, 0, 100, 50), reg(150, 200, 30, 80, 60)], expect=dict(taker="staged", why_fast=1)))
        for g, mg in ((5, 0), (4, 1)):
            cs.append(patch_case(f"patch_g{g}_n{n}", 11000 + 10 * n, 70, 70, g, qlen=150, extra=by, expect=dict(taker="staged", why_fast=2, align=1, merge=mg)))
        # q0 and p2 are a patch candidate that merges.  p1 is q0 moved by a base with a query part that ends where p2's ends, so
        # mem_patch_reg refuses p1 against p2 on qe; it is redundant with q0.  With the higher score p1 excludes q0 and nothing is left to
        # patch: k_dedup_fast must finish the list.  With the lower score p1 goes itself, q0 stays a candidate and the list is refused.
        if n >= 3:
            c = patch_case(f"behind_excluded_n{n}", 12000 + 10 * n, 70, 70, 3, qlen=150)
            q0, p2 = _undict(c.regs[0]), _undict(c.regs[1])
            for d, s_ in ((10, 0), (-10, 1)):
                p1 = dict(q0, rb=q0["rb"] + 1, re=q0["re"] + 1, qb=q0["qb"] + 1, qe=p2["qe"], score=q0["score"] + d)
                cs.append(Case(f"behind_{'excluded' if d > 0 else 'live'}_n{n}", c.seq, [q0, p1, p2] + by[:n - 3], side=(f"behind_n{n}", s_),
                               expect=dict(taker="fast", align=0, merge=0, excl=1, n=n - 1) if d > 0 else dict(why_fast=2, align=1, merge=1, excl=1, n=n - 2)))
            # An excluded entry is left with qe = qb.  Here q0's query part starts 3 bases before p2's, so that with its qe collapsed onto
            # its qb it passes every pre-test against p2 (w = 0, r = 0.02) -- which, whole, it fails on r: a fast_dedup that tested excluded
            # entries would refuse this list, the right one finishes it.
            q0c = dict(q0, qb=p2["qb"] - 3, qe=p2["qb"] + 67)
            p1c = dict(q0c, rb=q0c["rb"] + 1, re=q0c["re"] + 1, qb=q0c["qb"] + 1, qe=p2["qe"], score=q0c["score"] + 10)
            cs.append(Case(f"behind_collapsed_n{n}", c.seq, [q0c, p1c, p2] + by[:n - 3], expect=dict(taker="fast", align=0, merge=0, excl=1, n=n - 1)))
    return cs


def build_fast_m1():
    """With mask_level_redun 1.0 two regions with the same start are never redundant: a tie in (score, rb, qb) among the survivors."""
    cs = []
    rng = random.Random(9)
    for n in range(2, 9):
        by = [reg(20000 + 400 * k, 20100 + 400 * k, 5, 105, 30 + k, rid=0) for k in range(n - 2)]
        for v in range(3):                                       # the tied pair in front of, behind and around the bystanders
            pair = [reg(100 + v, 200, 0, 100, 50 + v), reg(100 + v, 210, 0, 110, 50 + v)]
            cs.append(Case(f"tie_sc_n{n}_v{v}", rand_seq(rng, 150), (pair + by, by + pair, pair[:1] + by + pair[1:])[v], expect=dict(taker="staged", why_fast=3)))
    return cs


# ------------------------------------------------------------------------------------------------ hand-over
def build_handover(window):
    """Patch windows one base below, at and one above the LDS window the set runs under (ext_lds_window), short lists and one of more
    than 32 regions (k_dedup has sorted that one in place before it hands the read over)."""
    def build():
        cs = []
        qlen = 150 if window <= 150 else 600
        for d in (-1, 0, 1):
            l = (window + d - 2) // 2
            l2 = window + d - 2 - l
            by = [reg(20000 + 40 * k, 20030 + 40 * k, 5, 35, 300 - k, rid=0) for k in range(40)]
            cs.append(patch_case(f"win{window}{d:+d}", 13000, l, l2, 2, qlen=qlen, expect=dict(align=1, merge=1)))
            cs.append(patch_case(f"win{window}{d:+d}_n42", 13500, l, l2, 2, qlen=qlen, extra=by, expect=dict(align=1, merge=1)))
            assert cs[-1].rlen == window + d
        return cs
    return build


# ------------------------------------------------------------------------------------------------ ALT
def build_alt():
    rng = random.Random(3)
    return [Case("alt_only", rand_seq(rng, 150), [reg(56100, 56200, 0, 100, 50), reg(57000, 57100, 10, 110, 60)]),
            Case("primary_only", rand_seq(rng, 150), [reg(100, 200, 0, 100, 50), reg(41000, 41100, 10, 110, 60)]),
            Case("mixed", rand_seq(rng, 150), [reg(56100, 56200, 0, 100, 50), reg(100, 200, 0, 100, 55), reg(2 * L_PAC - 57100, 2 * L_PAC - 57000, 10, 110, 60, rid=2)]),
            Case("mixed_n40", rand_seq(rng, 150), [reg(56000 + 90 * k, 56080 + 90 * k, k, 80 + k, 50 + k) for k in range(20)] + [reg(90 * k, 80 + 90 * k, k, 80 + k, 150 + k) for k in range(20)])]


# ------------------------------------------------------------------------------------------------ random
def build_random(count=2000, seed0=10000):
    """`count` seeded lists of 2 to 200 regions over real flanks of ctg2: the query is a stretch of the genome with a few small indels; the
    regions are pieces of its true alignment (so neighbours on one diagonal are patch candidates), copies of pieces shifted by a base or
    two (redundant), exact repeats of (score, rb, qb) and of re (ties), and decoys elsewhere."""
    def build():
        G = genome()
        cs = []
        for i in range(count):
            rng = random.Random(seed0 + i)
            n = rng.choice((2, 2, 3, 3, 4, 5, 6, 8, 9, 12, 20, 33, 40, 70, 120, 200)) if i % 4 else rng.randrange(2, 9)
            qlen = rng.choice((150, 150, 150, 250))
            x = 40000 + rng.randrange(200, 15000)
            # the query: pieces of the reference with a small deletion or insertion between them
            parts, segs, pos = [], [], x
            qpos = 0
            while qpos < qlen - 30:
                ln = min(rng.randrange(30, 80), qlen - qpos)
                parts.append(G[pos:pos + ln]); segs.append((pos, qpos, ln))
                pos += ln; qpos += ln
                if rng.random() < .5:
                    pos += rng.randrange(1, 5)
                elif qpos < qlen - 4:
                    k = rng.randrange(1, 4); parts.append(rand_seq(rng, k)); qpos += k
            q = np.concatenate(parts)
            q = np.concatenate([q, rand_seq(rng, max(0, qlen - len(q)))])[:qlen]
            segs = [s for s in segs if s[1] + s[2] <= qlen]
            rev = rng.random() < .3
            regs = []
            while len(regs) < n:
                t = rng.random()
                if t < .45 or not regs:
                    rb, qb, ln = rng.choice(segs)
                    regs.append(reg(rb, rb + ln, qb, qb + ln, ln - rng.choice((0, 0, 0, 5)), w=rng.choice((0, 0, 3)), sub=rng.randrange(20), csub=rng.randrange(20)))
                elif t < .65:
                    b = dict(rng.choice(regs)); d = rng.randrange(0, 3)
                    if b["qe"] + d <= qlen and b["re"] + d <= 56000:
                        regs.append(dict(b, rb=b["rb"] + d, re=b["re"] + d, qb=b["qb"] + d, qe=b["qe"] + d, score=b["score"] + rng.randrange(-2, 3)))
                elif t < .72:
                    b = dict(rng.choice(regs))
                    if b["re"] - b["rb"] > 12:
                        regs.append(dict(b, rb=b["rb"] + 5, qb=b["qb"] + 5))                   # same end: a tie in re
                elif t < .78:
                    regs.append(dict(rng.choice(regs)))                                          # an identical hit
                elif t < .84:
                    b = dict(rng.choice(regs))                                                   # strictly inside another on both axes: redundant under any mask_level_redun
                    if b["re"] - b["rb"] > 16 and b["qe"] - b["qb"] > 16:
                        regs.append(dict(b, rb=b["rb"] + 3, re=b["re"] - 3, qb=b["qb"] + 3, qe=b["qe"] - 3, score=b["score"] - rng.randrange(0, 9)))
                else:
                    rb = rng.randrange(100, 39000); ln = rng.randrange(20, 100); qb = rng.randrange(0, qlen - ln)
                    regs.append(reg(rb, rb + ln, qb, qb + ln, rng.randrange(20, ln + 1), rid=0))
            rng.shuffle(regs)
            cs.append((mirror if rev else Case)(f"rnd{i}", q, regs, heavy=rng.random() < .1))
        return cs
    return build


# ------------------------------------------------------------------------------------------------ the sets
def S(build, flags=(), mask=0.95, gap=10000, knobs=None, slab=False, pairs=True):
    """pairs False: the set runs lists built for the default options under others -- their threshold pairs and expectations do not apply."""
    return NS(build=build, flags=list(flags), mask=mask, gap=gap, knobs=knobs or {}, slab=slab, pairs=pairs)


SETS = {
    "sizes": S(build_sizes(False), gap=3, slab=True),
    "sizes_m1": S(build_sizes(True), gap=3, mask=1.0, slab=True),
    "sizes_rsm": S(build_sizes(False), gap=3, knobs=dict(rank_sort_min=1 << 30)),
    "redun_0.95": S(build_redun(0.95)),
    "redun_0.5": S(build_redun(0.5), mask=0.5),
    "redun_0.3": S(build_redun(0.3), mask=0.3),
    "reach": S(build_reach(10000)),
    "reach_G50": S(build_reach(50), flags=["-G", "50"], gap=50),
    "patch": S(build_patch, slab=True),
    "patch_w300": S(build_patch, flags=["-w", "300"], pairs=False),
    "fast": S(build_fast),
    "fast_m1": S(build_fast_m1, mask=1.0),
    "handover_150": S(build_handover(150), knobs=dict(ext_lds_window=150)),
    "handover_400": S(build_handover(400), knobs=dict(ext_lds_window=400)),
    "alt": S(build_alt, slab=True),
    "limits": S(build_limits, slab=True),
    "patch_A2B3": S(build_patch, flags=["-A", "2", "-B", "3"], pairs=False),
    "patch_O4,8_E2,1": S(build_patch, flags=["-O", "4,8", "-E", "2,1"], pairs=False),
    "mixed": S(lambda: [_bare(c) for c in cases_of("sizes")[:200:7] + cases_of("fast") + cases_of("patch")[:20] + cases_of("reach_G50")[-6:]]),   # every taker in one batch, judged under one option set
    # identical hits reach the second sort only where nothing with the same start is redundant, that is under mask_level_redun >= 1 (see the
    # module's docstring): the random set runs under 1.0, where a region strictly inside another is still redundant; random_m95 is the same
    # generator under the default
    "random": S(build_random(), mask=1.0),
    "random_m95": S(build_random(600, 50000)),
}
_built = {}


def cases_of(name):
    if name not in _built:
        _built[name] = SETS[name].build()
        names = [c.name for c in _built[name]]
        assert len(set(names)) == len(names), name
    return _built[name]


def opt_of(name):
    s = SETS[name]
    o, _ = common.opt_from_cli(s.flags)
    o.mask_level_redun, o.max_chain_gap = s.mask, s.gap
    return o


def pack(cases):
    off = np.cumsum([0] + [len(c.seq) for c in cases]).astype(np.int64)
    codes = np.concatenate([c.seq for c in cases])
    reg_off = np.cumsum([0] + [len(c.regs) for c in cases]).astype(np.int64)
    regs = np.concatenate([c.regs for c in cases])
    heavy = np.array([c.heavy for c in cases], dtype=np.uint8)
    return codes, off, reg_off, regs, heavy


def case_words(name):
    """The case file of `bwa_oracle katdedup` / `bwaref katdedup` (oracle/kat_dedup_io.h) as int64 words."""
    s = SETS[name]
    w = [np.array([TAG_OPT, 2, f32bits(s.mask), s.gap], np.int64)]
    for i, c in enumerate(cases_of(name)):
        w += [np.array([bw.TAG_READ, 2, i, len(c.seq), TAG_SEQ, len(c.seq)], np.int64), c.seq.astype(np.int64),
              np.array([TAG_REGS, 1 + c.regs.size, len(c.regs)], np.int64), c.regs.ravel()]
    return np.concatenate(w)


def input_digest(name):
    return hashlib.sha256(case_words(name).tobytes() + " ".join(SETS[name].flags).encode()).hexdigest()


def run_checker(exe, name, prefix, workdir, tag="c"):
    """-> per read (final regions [n x 19], stat words [STAT_N])."""
    fin, fout = os.path.join(workdir, f"{tag}.{name}.in.bin"), os.path.join(workdir, f"{tag}.{name}.out.bin")
    case_words(name).tofile(fin)
    subprocess.check_call([exe, "katdedup", *SETS[name].flags, prefix, fin, fout])
    reads = common.by_read(bw.read_record_file(fout))
    assert len(reads) == len(cases_of(name))
    out = []
    for r in reads:
        a = r[TAG_OUT]
        n = int(a[0])
        out.append((a[1 + STAT_N:].reshape(n, NW), a[1:1 + STAT_N]))
    return out


def digests(lists):
    """Per read the sha256 of its final list: what kat_dedup.npz holds."""
    return np.array([hashlib.sha256(np.ascontiguousarray(x, dtype=np.int64).tobytes()).digest() for x in lists], dtype="S32")


def pairs_of(name):
    out = {}
    if not SETS[name].pairs:
        return out
    for i, c in enumerate(cases_of(name)):
        if c.side:
            out.setdefault(c.side[0], [None, None])[c.side[1]] = i
    assert all(None not in v for v in out.values()), (name, out)
    return out


# ------------------------------------------------------------------------------------------------ the model of who takes a list
def fast_model(regs, mask, gap, w_opt, skip_excluded=True):
    """k_dedup_fast's decision from the list alone (fast_dedup of csrc/k_extend.hip restated): 0 it finishes the list, 1 a tie in the
    first sort, 2 a pair mem_patch_reg would go on to align, 3 a tie in the second sort."""
    a = [dict(rb=int(w[C_RB]), re=int(w[C_RE]), qb=int(w[C_QB]), qe=int(w[C_QE]), rid=int(w[C_RID]), score=int(w[C_SCORE])) for w in regs]
    if len({x["re"] for x in a}) != len(a):
        return 1
    a.sort(key=lambda x: x["re"])
    f32 = np.float32
    for i in range(1, len(a)):
        p = a[i]
        if p["rid"] != a[i - 1]["rid"] or p["rb"] >= a[i - 1]["re"] + gap:
            continue
        j = i - 1
        while j >= 0 and p["rid"] == a[j]["rid"] and p["rb"] < a[j]["re"] + gap:
            q = a[j]
            j -= 1
            if skip_excluded and q["qe"] == q["qb"]:             # (False: a wrong fast_dedup that tests excluded entries too; the CPU test shows that it would be seen)
                continue
            orr = q["re"] - p["rb"]
            oq = q["qe"] - p["qb"] if q["qb"] < p["qb"] else p["qe"] - q["qb"]
            mr = min(q["re"] - q["rb"], p["re"] - p["rb"])
            mq = min(q["qe"] - q["qb"], p["qe"] - p["qb"])
            if f32(orr) > f32(mask) * f32(mr) and f32(oq) > f32(mask) * f32(mq):
                if p["score"] < q["score"]:
                    p["qe"] = p["qb"]
                    break
                q["qe"] = q["qb"]
            elif q["rb"] < p["rb"]:
                if q["rb"] < L_PAC <= p["rb"] or q["qb"] >= p["qb"] or q["qe"] >= p["qe"] or q["re"] >= p["re"]:
                    continue
                w = abs((q["re"] - p["rb"]) - (q["qe"] - p["qb"]))
                r = abs((q["re"] - p["rb"]) / (p["re"] - q["rb"]) - (q["qe"] - p["qb"]) / (p["qe"] - q["qb"]))
                if q["re"] < p["rb"] or q["qe"] < p["qb"]:
                    if w > w_opt << 1 or r >= float(f32(0.05)):
                        continue
                elif w > w_opt << 2 or r >= float(f32(0.05) * f32(2)):
                    continue
                return 2
    keys = [(x["score"], x["rb"], x["qb"]) for x in a if x["qe"] > x["qb"]]
    return 3 if len(set(keys)) != len(keys) else 0


def predict(name, case, stat, form=bw.KAT_DEDUP_PRODUCT, knobs=None):
    """The diag word bwahip_kat_dedup must return for a case: the taker and k_dedup_fast's reason from the list alone (fast_model, the
    list's length, the list it enters, the window of its patch against ext_lds_window); which sort ran on one lane and the two counts from
    the judge's record of what the function did."""
    s = SETS[name]
    knobs = s.knobs if knobs is None else knobs
    rsm = knobs.get("rank_sort_min", 2)
    n = len(case.regs)
    d = 0
    if form == bw.KAT_DEDUP_PRODUCT and not case.heavy and n <= FAST_N:
        why = fast_model(case.regs, s.mask, s.gap, opt_of(name).w)
        if why == 0:
            return bw.KAT_DEDUP_FAST
        d |= why << bw.KAT_DEDUP_WHY_SHIFT
    handed = form != bw.KAT_DEDUP_SLAB and stat[S_ALIGN] > 0 and case.rlen is not None and case.rlen > min(knobs.get("ext_lds_window", 1 << 30), MAXT)
    if handed:
        d |= bw.KAT_DEDUP_HANDED
    d |= bw.KAT_DEDUP_SLABBED if handed or form == bw.KAT_DEDUP_SLAB else bw.KAT_DEDUP_STAGED if n <= STAGE_N else bw.KAT_DEDUP_GLOBAL
    if n < rsm or (stat[S_FLAGS] & F_TIE1 and stat[S_FLAGS] & F_COMB1):
        d |= bw.KAT_DEDUP_LANE1
    if stat[S_KEPT] < rsm or (stat[S_IDENT] > 0 and stat[S_FLAGS] & F_COMB2):
        d |= bw.KAT_DEDUP_LANE2
    return d | min(int(stat[S_ALIGN]), 2047) << bw.KAT_DEDUP_ALN_SHIFT | min(int(stat[S_MERGE]), 2047) << bw.KAT_DEDUP_MRG_SHIFT
