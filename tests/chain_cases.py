"""Seed lists built on purpose for chaining and the chain filter (csrc/k_chain.hip; mem_chain's seed loop bwamem.c:280-317 through kbtree.h,
mem_chain_flt bwamem.c:334-392), fed to bwahip_kat_chain, to `bwa_oracle katchain` (ora_kat_chain) and, where it is built, to `bwaref katchain`
(the reference's own kbtree / test_and_merge / mem_chain_flt).  Deterministic: every generator is seeded and depends on nothing but the layout
of the test genome of conftest.small_index (three contigs of 600 000, 300 000 and 100 000 bases; the third an ALT contig in the index
alt_index() makes), which test_chain_cases_cpu.py checks against the index itself, together with every seed's contig (ora_intv2rid).

A seed is (rbeg, qbeg, len, rid) in the forward-reverse coordinate of the doubled reference, exactly what the SA look-up hands to chaining; the
kernels never look at the bases, so any coordinates inside a contig are as good as a real read's.  A read is at most 700 bases long.

What cannot be built (shown in test_chain_cases_cpu.py rather than assumed):
  * a sort area that does not fit: for every class the LDS (or, with global nodes, the filter's scratch) holds the sort of as many chains as the
    class admits seeds, so the one-lane sort "because the area was too small" is unreachable with the shipped constants;
  * a kept chain that overlaps chain i significantly, does not shadow it, and stands in front of the kept chain that does: the kept list is in
    order of falling weight and the weight test of bwamem.c:365 can only turn true -> false as w_j falls.  What the wavefront filter must get
    right instead: kept chains BEHIND the shadowing one that overlap as well (they must not receive `first`), and a `first` set by an earlier,
    unshadowed chain that a later one must not overwrite."""
import hashlib
import os
import subprocess
from collections import namedtuple

import numpy as np

import common
from common import bw

CTG_LEN = (600_000, 300_000, 100_000)
CTG_OFF = (0, 600_000, 900_000)
L_PAC = 1_000_000
ALT_RID = 2
READ_LEN = 700
TAG_SEEDS, TAG_INTV, TAG_CHAIN_STAT = 6, 1, 30

# the budgets of k_chain.hip: seeds a class admits -> B-tree nodes it has room for (class 3 and the helped-out reads: S / 4 + 4 global slots)
SMALL_SEEDS, MID_SEEDS, BIG_SEEDS = 256, 1536, 3200
NODE_CAP = {0: 72, 1: 400, 2: 800}
KNOBS_SHIPPED = dict(chain_big_min=512, chain_mid_max=1536, chain_big_max=3200, chain_glb_grid=2048)

Case = namedtuple("Case", "name seeds intv expect", defaults=(None,))   # seeds [n x 4] int64, intv [m x 3] int64 (x[2], qbeg, qend); expect: what the case is for


def rid_of(rbeg, length):
    """bns_intv2rid (bntseq.c:370): the contig holding [rbeg, rbeg + len) on either strand, -1 when it bridges two or the strand boundary."""
    rend = rbeg + length
    if rbeg < L_PAC < rend:
        return -1

    def pos2rid(p):
        p = 2 * L_PAC - 1 - p if p >= L_PAC else p
        return 0 if p < CTG_OFF[1] else 1 if p < CTG_OFF[2] else 2
    a, b = pos2rid(rbeg), pos2rid(rend - 1)
    return a if a == b else -1


def rev(pos_f, length):
    """rbeg on the reverse strand of the seed that covers [pos_f, pos_f + len) forward."""
    return 2 * L_PAC - (pos_f + length)


def mk(name, seeds, intv=(), expect=None):
    s = np.array([(r, q, l, rid_of(r, l)) for r, q, l in seeds], dtype=np.int64).reshape(-1, 4)
    assert all(0 <= q and l >= 1 and q + l <= READ_LEN and 0 <= r and r + l <= 2 * L_PAC for r, q, l, _ in s), name
    return Case(name, s, np.array(sorted(intv, key=lambda t: (t[1] << 32) | t[2]), dtype=np.int64).reshape(-1, 3), expect)


INTV_KINDS = [(), ((600, 10, 50),), ((3, 0, 30), (501, 20, 90), (9000, 60, 120), (500, 100, 400), (777, 300, 330))]


# ------------------------------------------------------------------------------------------------ merge rule
def merge_cases(w=100, gap=10_000):
    """One chain plus one seed on either side of every inequality of test_and_merge, for band w and max_chain_gap gap."""
    R, out = 5000, []

    def two(name, b, a=((R, 100, 20),), expect=None):
        """expect, of the last seed: 'merge' into the one chain of `a`, 'new' chain, 'swallow' (contained: dropped), 'skip' (no contig)"""
        out.append(mk(f"merge.{name}", list(a) + [b], INTV_KINDS[len(out) % 3], expect))
    for d in (0, 1):                                    # x - y against w; y - x against w (where the gap does not decide first)
        if 100 + 10 + w + d + 20 <= READ_LEN and 10 + w + d - 20 < gap:
            two(f"x-y=w+{d}", (R + 10, 100 + 10 + w + d, 20), expect="new" if d else "merge")
            two(f"y-x=w+{d}", (R + 10 + w + d, 110, 20), expect="new" if d else "merge")
    x0 = min(w, 1)
    pair = ((R, 100, 20), (R + 50, 150, 20))            # a chain of two seeds: q [100, 170), r [R, R + 70)
    two("y=0", (R + 50, 150 + x0, 20), pair, expect="merge")
    two("y=-1", (R + 49, 150 + x0, 20), pair, expect="new")
    for d in (-1, 0):                                   # x - last_len and y - last_len against max_chain_gap
        x = 20 + gap + d
        if 100 + x + 20 <= READ_LEN:
            two(f"x-len=G{d:+d}", (R + x - min(w, 10), 100 + x, 20), expect="new" if d == 0 else "merge")   # (y - len stays below the gap)
        if 100 + max(x - w, 0) + 20 <= READ_LEN:
            two(f"y-len=G{d:+d}", (R + x, 100 + max(x - w, 0), 20), expect="new" if d == 0 else "merge")
    two("contained.inside", (R + 10, 110, 20), pair, expect="swallow")
    two("contained.qbeg=", (R, 100, 20), pair, expect="swallow")
    two("contained.qbeg-1", (R + 10, 99, 20), pair, expect="new")
    two("contained.qend=", (R + 50, 150, 20), pair, expect="swallow")
    two("contained.qend+1", (R + 50 + x0, 150 + x0, 20), pair, expect="merge")
    two("contained.rbeg-1", (R - 1, 101, 20), pair, expect="new")
    two("contained.rend=", (R + 50, 140, 20), pair, expect="swallow")
    two("contained.rend+1", (R + 51, 140, 20), pair)
    two("contained.short", (R + 60, 160, 10), pair, expect="swallow")
    two("other_rid", (CTG_OFF[1] + 5000, 130, 20), expect="new")
    two("other_rid.near", (CTG_OFF[1] + 3, 133, 20), ((CTG_OFF[1] - 30, 100, 20),), expect="new")
    two("rid<0.contigs", (CTG_OFF[1] - 10, 130, 20), expect="skip")
    two("rid<0.strands", (L_PAC - 10, 130, 20), expect="skip")
    two("rid<0.first", (R, 100, 20), ((CTG_OFF[2] - 5, 90, 20),))
    # l_pac rule: a forward chain never takes a reverse seed, although contig, band and gap would all allow it
    f0 = L_PAC - 60
    two("l_pac.fwd_then_rev", (L_PAC + 5, 100 + 65, 20), ((f0, 100, 20),), expect="new")
    two("l_pac.rev_then_fwd", (f0, 165, 20), ((L_PAC + 5, 100, 20),), expect="new")
    two("l_pac.rev_then_rev", (L_PAC + 50, 145, 20), ((L_PAC + 5, 100, 20),), expect="merge")
    two("l_pac.fwd2_then_rev", (L_PAC + 5, 100 + 65, 20), ((f0 - 30, 70, 20), (f0, 100, 20)), expect="new")
    return out


# ------------------------------------------------------------------------------------------------ tree shape
TREE_W = 30                                             # the tree sets run under -w 30, so that 12 chains can share a pos (below)
TREE_COUNTS = (11, 12, 71, 72, 131, 132, 256, 257, 258, 259, 1536, 1537, 3200, 3201)
TREE_ORDERS = ("asc", "desc", "zigzag", "random")


def tree_case(n, order, ties, seed=0):
    """n seeds that each open a chain: n - ties distinct positions 150 apart at one qbeg (x = 0, y >= 150 > w: no merge), and `ties` more
    chains on ONE of these positions, told apart by qbeg steps of 31 > w (y = 0, |x| > w), interleaved with the rest.  Where the equal
    positions land in the tree, and so the order they come out in, depends on every split (kbtree.h:197 `pos > x->pos[i]`)."""
    rng = np.random.default_rng(1000 * n + 10 * ties + seed)
    m = n - ties
    pos = [1000 + 150 * i for i in range(m)]
    if order == "desc":
        pos = pos[::-1]
    elif order == "zigzag":
        pos = [pos[i // 2] if i % 2 == 0 else pos[m - 1 - i // 2] for i in range(m)]
    elif order == "random":
        pos = list(rng.permutation(pos))
    seeds = [(int(p), 0, 19) for p in pos]
    if ties:
        p_tie = int(sorted(pos)[m // 2])
        at = sorted(int(v) for v in rng.choice(np.arange(1, m), size=ties, replace=False)) if m > ties else list(range(1, ties + 1))
        for k, a in enumerate(at):
            seeds.insert(min(a + k, len(seeds)), (p_tie, 31 * (k + 1), 19))
    return mk(f"tree.{n}.{order}.{ties}", seeds, INTV_KINDS[(n + ties) % 3])


def tree_cases():
    return [tree_case(n, o, t) for n in TREE_COUNTS for o in TREE_ORDERS for t in (0, 2, 12) if n > t]


# ------------------------------------------------------------------------------------------------ sort by weight
SORT_COUNTS = (1, 2, 33, 64, 65, 255)


def lone_chains(name, weights, q=0, pos0=2000, step=1000, intv=()):
    """One single-seed chain per weight (a seed's weight is its length), in B-tree order: no two merge (x = 0, y = step > w)."""
    return mk(name, [(pos0 + step * i, q, int(wt)) for i, wt in enumerate(weights)], intv)


def sort_cases():
    out = []
    for n in SORT_COUNTS:
        out.append(lone_chains(f"sort.{n}.equal", [40] * n, step=600))
        out.append(lone_chains(f"sort.{n}.two", [40 if (i * 7) % 3 else 41 for i in range(n)], step=600))
        out.append(lone_chains(f"sort.{n}.rising", [19 + i for i in range(n)], step=600))
        out.append(lone_chains(f"sort.{n}.falling", [19 + n - i for i in range(n)], step=600))
    # sorted input with ties: the reference's introsort reaches its depth limit here (as in test_wavefront_introsort_equals_ksort_restatement)
    rng = np.random.default_rng(77)
    for n in (129, 255, 600):
        wts = np.sort(rng.integers(0, n // 2, n))[::-1] + 19
        out.append(lone_chains(f"sort.{n}.depth", wts, step=900))
    return out


# ------------------------------------------------------------------------------------------------ overlap filter
def chains(name, spec, pad=0, intv=()):
    """spec: chains as lists of (qbeg, len) seeds (+ 'alt' as a last element for a chain on the ALT contig); every chain lies 3000 bases
    from the next, its seeds on one diagonal.  pad: that many more chains in q [0, 250), weights 250, 249, ...: heavier than any chain of
    a spec (which stay in q >= 260 when padded) and clear of them, all kept -- there to carry the read past 32 chains and the kept list past
    a ballot chunk."""
    seeds, p_main, p_alt = [], 3000, CTG_OFF[2] + 1000
    for ch in list(spec) + [[(0, 250 - k)] for k in range(pad)]:
        alt = ch[-1] == "alt"
        ch = [s for s in ch if s != "alt"]
        base = p_alt if alt else p_main
        if alt:
            p_alt += 1500
        else:
            p_main += 3000
        seeds += [(base + q - ch[0][0], q, l) for q, l in ch]
    return mk(name, seeds, intv)


def filter_cases(gap=10_000, min_seed_len=19):
    out = []
    two_k = 2 * min_seed_len
    for pad in (0, 40, 70):                             # 0: the sequential filter; 40, 70: k_chain_flt, kept lists below and beyond 64
        P = f"p{pad}"
        Q = 260
        # exact equality of mask_level (0.5) in float: overlap 20 of min_l 40 is significant, 19 is not
        for ov in (19, 20, 21):
            out.append(chains(f"flt.{P}.mask.{ov}", [[(Q, 200)], [(Q + 200 - ov, 40)]], pad))
        # drop_ratio at equality: 50 < 100 * 0.5 is false (kept), 49 is dropped (100 - 49 >= 38).  (A chain of weight 60 in front takes the
        # `first` of the heavy one, which would otherwise bring the dropped chain back with kept = 1.)
        for wi in (49, 50, 51):
            out.append(chains(f"flt.{P}.drop.{wi}", [[(Q, 100)], [(Q + 2, 60)], [(Q + 10, wi)]], pad))
        # w_j - w_i at 2 * min_seed_len and one below (w_i < w_j / 2 in both)
        for wi in (70 - two_k - 1, 70 - two_k, 70 - two_k + 1):
            if wi >= 1:
                out.append(chains(f"flt.{P}.diff.{wi}", [[(Q, 70)], [(Q + 2, 60)], [(Q + 5, wi)]], pad))
        # min_l against max_chain_gap (reachable only under -G 50)
        for ml in (gap - 1, gap, gap + 1):
            if 1 <= ml <= 200:
                out.append(chains(f"flt.{P}.minl.{ml}", [[(Q, 2 * ml + two_k + 2)], [(Q + 3, ml)]], pad))
        # ALT: an ALT chain never shadows a primary one; a primary one shadows an ALT one; ALT over ALT
        out.append(chains(f"flt.{P}.alt_over_pri", [[(Q, 200), "alt"], [(Q + 10, 40)]], pad))
        out.append(chains(f"flt.{P}.pri_over_alt", [[(Q, 200)], [(Q + 10, 40), "alt"]], pad))
        out.append(chains(f"flt.{P}.alt_over_alt", [[(Q, 200), "alt"], [(Q + 10, 40), "alt"]], pad))
        # `first`: set by the first chain that overlaps significantly, shadowed or not; a later one must not overwrite it
        out.append(chains(f"flt.{P}.first.kept_then_dropped", [[(Q, 100)], [(Q + 5, 80)], [(Q + 10, 30)]], pad))
        out.append(chains(f"flt.{P}.first.two_dropped", [[(Q, 100)], [(Q + 5, 30)], [(Q + 10, 29)], [(Q + 300, 90)], [(Q + 310, 28)]], pad))
        # chains of two and three seeds: weight below span, `first` and the seed copy of multi-seed chains
        out.append(chains(f"flt.{P}.multi", [[(Q, 30), (Q + 60, 30), (Q + 150, 40)], [(Q + 20, 25), (Q + 50, 30)], [(Q + 155, 20)]], pad))
        # max_chain_extend (-N): several chains of kept 1 / 2 in a row
        out.append(chains(f"flt.{P}.extend", [[(Q, 120)], [(Q + 4, 118)], [(Q + 8, 116)], [(Q + 12, 40)], [(Q + 200, 110)], [(Q + 204, 108)], [(Q + 208, 35)]], pad))
    # kept lists of 63, 64, 65 and 130 chains, the shadowing chain at kept index 0, 63, 64 and last: kept chain i weighs 400 - i and lies
    # in q [0, 400 - i) in front of the shadowing index k, in q [300, 700 - i) from k on; the two light chains in [500, 525) meet only the
    # latter.  Chain k and the light ones are ALT, the rest primary: no primary chain sets `first` on an ALT one, so chain k still has none
    # when the first light chain stops at it (and receives it: kept = 1), while the kept chains behind k overlap it as well and must be left alone
    for n_kept in (63, 64, 65, 130):
        for k in sorted({0, 63, 64, n_kept - 1}):
            if k < n_kept:
                spec = [[(0 if i < k else 300, 400 - i)] + (["alt"] if i == k else []) for i in range(n_kept)] + [[(500, 20), "alt"], [(505, 19), "alt"]]
                out.append(chains(f"flt.kept{n_kept}.shadow{k}", spec))
    # exactly 32 and 33 chains: the last that the sequential filter takes, the first that goes to k_chain_flt
    for n in (32, 33):
        out.append(chains(f"flt.count{n}", [[(10 * (i % 8), 300 - 3 * i)] for i in range(n - 2)] + [[(400, 30)], [(405, 29)]]))
        # ... and as many SURVIVING min_chain_weight 40 (under -W 40; six more below it)
        out.append(chains(f"flt.survive{n}", [[(10 * (i % 8), 300 - 3 * i)] for i in range(n - 2)] + [[(400, 41)], [(405, 40)]] + [[(500 + 20 * j, 39 - j)] for j in range(6)]))
    return out


# ------------------------------------------------------------------------------------------------ random reads
def rand_read(rng, n_seeds, name):
    """Seeds of a few loci that mostly merge, single seeds that open chains, and seeds on the pos of an earlier chain at another qbeg."""
    loci, seeds, openers = [], [], []

    def new_locus():
        ctg = int(rng.integers(0, 3))
        ln = int(rng.integers(19, 40))
        pf = CTG_OFF[ctg] + int(rng.integers(100, CTG_LEN[ctg] - 2000))
        p = rev(pf, ln) - 1000 if rng.random() < 0.4 else pf
        loci.append([p, int(rng.integers(0, 200)), 0])
    for _ in range(max(1, n_seeds // 12)):
        new_locus()
    for _ in range(n_seeds):
        u = rng.random()
        ln = int(rng.integers(19, 45))
        if u < 0.5:
            lc = loci[int(rng.integers(0, len(loci)))]
            if lc[1] + lc[2] + ln + 30 > READ_LEN:
                lc[1], lc[2] = int(rng.integers(0, 100)), 0
                lc[0] += 20_000 if lc[0] + 40_000 < (L_PAC if lc[0] < L_PAC else 2 * L_PAC) else -200_000
            q = lc[1] + lc[2]
            s = (lc[0] + lc[2] + int(rng.integers(-3, 4)), q, ln)
            lc[2] += int(rng.integers(1, 30))
        elif u < 0.8 or not openers:
            ctg = int(rng.integers(0, 3))
            pf = CTG_OFF[ctg] + int(rng.integers(0, CTG_LEN[ctg] - ln + 1))
            s = (rev(pf, ln) if rng.random() < 0.5 else pf, int(rng.integers(0, READ_LEN - ln + 1)), ln)
            openers.append(s)
        else:
            o = openers[int(rng.integers(0, len(openers)))]
            s = (o[0], int(rng.integers(0, READ_LEN - o[2] + 1)), o[2])
        if s[0] < 0 or s[0] + s[2] > 2 * L_PAC:
            s = (5000, s[1], s[2])
        seeds.append(s)
    return mk(name, seeds, INTV_KINDS[n_seeds % 3])


def random_cases():
    rng = np.random.default_rng(20261)
    return [rand_read(rng, int(rng.integers(1, 401)), f"random.{i}") for i in range(400)]


CLASS_SIZES = (1, 5, 8, 9, 100, 256, 257, 258, 259, 300, 512, 513, 700)
# knob settings the class set runs under -> per size the class that must take the read
CLASS_KNOBS = {
    "off": dict(chain_big_min=-1), "all": dict(chain_big_min=0), "min8": dict(chain_big_min=8), "shipped": dict(chain_big_min=512),
    "narrow": dict(chain_big_min=0, chain_mid_max=257, chain_big_max=258),
}


def class_cases():
    rng = np.random.default_rng(20262)
    edge = [mk("class.empty", []), mk("class.all_skipped", [(CTG_OFF[1] - 10, 5, 20), (L_PAC - 5, 50, 19)])]   # no seed; none that has a contig
    return [rand_read(rng, n, f"class.{n}") for n in CLASS_SIZES] + [tree_case(n, "random", 12, seed=3) for n in (257, 258, 259, 600)] + edge


def flood_cases(which):
    """The smallest batches that switch the help-out loop of the global-node kernel on: 2049 reads of class 1, 513 of class 2."""
    n, lo = (2049, 257) if which == 1 else (513, 258)
    rng = np.random.default_rng(20263 + which)
    return [rand_read(rng, int(rng.integers(lo, 301)), f"flood{which}.{i}") for i in range(n)]


def expected_taker(n_seeds, knobs):
    """Who must take a read of n_seeds under `knobs` (the classification of k_chain_classify; a class 1 / 2 read may also be helped out)."""
    k = dict(KNOBS_SHIPPED, **knobs)
    if k["chain_big_min"] < 0 or n_seeds <= k["chain_big_min"]:
        return bw.CHAIN_BY_LANE
    return 0 if n_seeds <= SMALL_SEEDS else 1 if n_seeds <= min(k["chain_mid_max"], MID_SEEDS) else 2 if n_seeds <= min(k["chain_big_max"], BIG_SEEDS) else 3


def node_room(n_seeds, taker):
    return NODE_CAP[taker] if taker in NODE_CAP else n_seeds // 4 + 4


# ------------------------------------------------------------------------------------------------ the sets
# name -> (option flags for all three programs, builder, knob settings the GPU test runs it under, in kat_chain.npz?)
BOTH = {"shipped": {}, "all": dict(chain_big_min=0)}
SETS = {
    "merge": ([], merge_cases, BOTH, True),
    "merge_w1": (["-w", "1"], lambda: merge_cases(w=1), BOTH, True),
    "merge_w300": (["-w", "300"], lambda: merge_cases(w=300), BOTH, True),
    "merge_G50": (["-G", "50"], lambda: merge_cases(gap=50), BOTH, True),
    "tree": (["-w", str(TREE_W)], tree_cases, dict(BOTH, off=dict(chain_big_min=-1)), True),
    "sort": ([], sort_cases, BOTH, True),
    "filter": ([], filter_cases, BOTH, True),
    "filter_G50": (["-G", "50"], lambda: filter_cases(gap=50), BOTH, True),
    "filter_D0.1": (["-D", "0.1"], filter_cases, BOTH, True),
    "filter_D0.9": (["-D", "0.9"], filter_cases, BOTH, True),
    "filter_W40": (["-W", "40"], filter_cases, BOTH, True),
    "filter_N1": (["-N", "1"], filter_cases, BOTH, True),
    "filter_N2": (["-N", "2"], filter_cases, BOTH, True),
    "filter_N5": (["-N", "5"], filter_cases, BOTH, True),
    "classes": ([], class_cases, CLASS_KNOBS, True),
    "random": ([], random_cases, BOTH, True),
    "flood1": ([], lambda: flood_cases(1), {"all": dict(chain_big_min=0)}, False),
    "flood2": ([], lambda: flood_cases(2), {"narrow_mid": dict(chain_big_min=0, chain_mid_max=257)}, False),
}
FAMILIES = {"merge": ["merge", "merge_w1", "merge_w300", "merge_G50"], "tree": ["tree"], "sort": ["sort"],
            "filter": [s for s in SETS if s.startswith("filter")], "classes": ["classes"], "random": ["random"], "flood": ["flood1", "flood2"]}

_built = {}


def cases_of(name):
    if name not in _built:
        _built[name] = SETS[name][1]()
    return _built[name]


# ------------------------------------------------------------------------------------------------ running them
def pack(cases):
    seed_off = np.cumsum([0] + [len(c.seeds) for c in cases]).astype(np.int64)
    intv_off = np.cumsum([0] + [len(c.intv) for c in cases]).astype(np.int64)
    seeds = np.concatenate([c.seeds for c in cases]) if cases else np.zeros((0, 4), np.int64)
    intv = np.concatenate([c.intv for c in cases]) if cases else np.zeros((0, 3), np.int64)
    return np.full(len(cases), READ_LEN, np.int32), seed_off, seeds, intv_off, intv


def case_words(cases):
    """The case file of `bwa_oracle katchain` / `bwaref katchain` as int64 words."""
    w = []
    for i, c in enumerate(cases):
        w += [np.array([bw.TAG_READ, 2, i, READ_LEN], np.int64), np.array([TAG_SEEDS, c.seeds.size], np.int64), c.seeds.ravel(),
              np.array([TAG_INTV, c.intv.size], np.int64), c.intv.ravel()]
    return np.concatenate(w) if w else np.zeros(0, np.int64)


def input_digest(cases):
    return hashlib.sha256(case_words(cases).tobytes()).hexdigest()


def run_checker(exe, prefix, cases, flags, workdir, tag="c"):
    """-> (per read {TAG: record}, stats [n x 4] or None)."""
    fin, fout = os.path.join(workdir, f"{tag}.in.bin"), os.path.join(workdir, f"{tag}.out.bin")
    case_words(cases).tofile(fin)
    subprocess.check_call([exe, "katchain", *flags, prefix, fin, fout])
    reads = common.by_read(bw.read_record_file(fout))
    assert len(reads) == len(cases)
    stats = np.array([r[TAG_CHAIN_STAT] for r in reads], np.int64) if reads and TAG_CHAIN_STAT in reads[0] else None
    return reads, stats


def mask_prefilter(rec):
    """w / kept / first of the chains before the filter mean nothing (test_gpu_stages._mask_chain_prefilter)."""
    a = rec.copy()
    n, i = int(a[0]), 1
    for _ in range(n):
        a[i + 3] = a[i + 4] = a[i + 5] = 0
        i += 8 + 4 * int(a[i + 7])
    return a


def masked(reads):
    return [{bw.STAGE_CHAIN: mask_prefilter(r[bw.STAGE_CHAIN]), bw.STAGE_CHAIN_FLT: r[bw.STAGE_CHAIN_FLT]} for r in reads]


def chain_list(rec):
    """record -> [(pos, rid, is_alt, w, kept, first, n_seeds, [(rbeg, qbeg, len)])]"""
    out, i = [], 1
    for _ in range(int(rec[0])):
        n = int(rec[i + 7])
        sd = rec[i + 8:i + 8 + 4 * n].reshape(n, 4)
        out.append((int(rec[i]), int(rec[i + 1]), int(rec[i + 2]), int(rec[i + 3]), int(rec[i + 4]), int(rec[i + 5]), n, sd[:, :3]))
        i += 8 + 4 * n
    return out


def chain_weight(sd):
    """mem_chain_weight (bwamem.c:220) of a chain's seeds [(rbeg, qbeg, len)]"""
    def cover(col):
        w = end = 0
        for s in sd:
            b, e = int(s[col]), int(s[col]) + int(s[2])
            w += e - b if b >= end else max(0, e - end)
            end = max(end, e)
        return w
    return min(cover(1), cover(0), (1 << 30) - 1)


def expected_diag(case, rd, st, taker, min_chain_weight=0):
    """What bwahip_kat_chain must report for a read the model (ora_kat_chain's statistics st) saw: [taker, nodes, height, sort, filter,
    chains].  The sort: k_chain's own below a wavefront class; otherwise the wavefront's, which hands over to one lane only when the
    introsort reaches its depth limit on weights with ties (without ties it places by rank and never partitions)."""
    n_sorted = int(st[2])
    if n_sorted < 2:
        sort = bw.CHAIN_SORT_NONE
    elif taker == bw.CHAIN_BY_LANE:
        sort = bw.CHAIN_SORT_LANE
    else:
        sort = bw.CHAIN_SORT_WAVE
        if st[3]:
            w = [x for x in (chain_weight(ch[7]) for ch in chain_list(rd[bw.STAGE_CHAIN])) if x >= min_chain_weight]
            assert len(w) == n_sorted
            if len(set(w)) < len(w):
                sort = bw.CHAIN_SORT_LANE_DEPTH
    flt = bw.CHAIN_FLT_NONE if n_sorted == 0 else bw.CHAIN_FLT_SEQ if n_sorted <= 32 else bw.CHAIN_FLT_WAVE
    nodes, height = (int(st[0]), int(st[1])) if len(case.seeds) else (0, 0)      # a read without seeds is left before the tree is made
    return [taker, nodes, height, sort, flt, int(rd[bw.STAGE_CHAIN][0])]


def digests(reads):
    """Per read the sha256 of its two records (the one before the filter masked): what kat_chain.npz holds of the larger cases."""
    return np.array([[hashlib.sha256(r[t].tobytes()).digest() for t in (bw.STAGE_CHAIN, bw.STAGE_CHAIN_FLT)] for r in masked(reads)], dtype="S32")


def alt_index(small_index, workdir):
    """small_index with its third contig declared ALT (links to the index files + a .alt list)."""
    alt = os.path.join(str(workdir), "alt")
    for e in ("amb", "ann", "bwt", "pac", "sa"):
        os.symlink(small_index["prefix"] + "." + e, alt + "." + e)
    with open(alt + ".alt", "w") as f:
        f.write("ctg3\n")
    return alt
