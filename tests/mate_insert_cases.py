"""Cases for the list update of mate rescue (csrc/k_pair.hip: ms_list_add / ms_list_close with incr_insert and sort_dedup_nopatch behind
them; entry bwahip_kat_mate_insert), built on purpose: every class states why it exists, and `check_reason` asserts that reason on the
oracle's result or on the step counts the model predicts.  Used by tests/test_mate_insert_cases_cpu.py (no GPU: the cases themselves are
checked) and tests/test_gpu_mate_insert.py (the device against the oracle).

An item is a start list (any arrangement, ties and duplicates allowed) and steps; a step is one orientation of mem_matesw's loop in
which the alignment was attempted: ("hit", region) or ("none",).  The judge of the lists is oracle/liboracle.so's ora_kat_mate_insert
(ora_matesw's list update: append, move in front of the first lower score, ora_sort_dedup_patch with bns == 0).  The model of the
device's path choice (`predict`) is the Python model of tests/test_incr_insert_model.py plus the `clean` flag as k_matesw carries it."""
import ctypes as C
import os
import random
import numpy as np
import common
import test_incr_insert_model as model

NW = 19                                                          # words per region (STAGE_REGS_PE): see `words`
W_RB, W_RE, W_QB, W_QE, W_RID, W_SCORE, W_TAG, W_SECONDARY, W_NCOMP = 0, 1, 2, 3, 4, 5, 7, 13, 16
L_PAC = 3_100_000_000                                            # a 3.1 Gbp genome: its reverse strand lies above 2^32
MS_LIST = 224                                                    # k_pair.hip: capacity up to which a list is worked on in LDS


def reg(rb, ln, score, qb=10, rid=0, dre=0, qln=None):
    """A region of `ln` reference bases (re = rb + ln + dre) and qln (default ln) query bases."""
    return dict(rid=rid, rb=rb, re=rb + ln + dre, qb=qb, qe=qb + (ln if qln is None else qln), score=score)


def words(r, tag):
    """The 19 words; every field the device carries gets a value that tells regions apart (tag: the item's running number, in `sub`)."""
    frac = int(np.float32((tag % 97) / 97.0).view(np.uint32))
    return [r["rb"], r["re"], r["qb"], r["qe"], r["rid"], r["score"], r["score"] + 1, tag, 0, tag % 41, tag % 5, 100 + tag % 7,
            min(r["re"] - r["rb"], r["qe"] - r["qb"]) >> 1, 0, 0, 19 + tag % 3, 0, 0, frac]


class Item:
    def __init__(self, name, start, steps, shuffle=None, **why):
        """start: the start list; its regions are tagged 0, 1, .. in the order given, the steps' regions after them; shuffle: seed of the
        arrangement the list is handed over in (None: as given)."""
        self.name, self.start, self.steps, self.why = name, [dict(x) for x in start], steps, why
        t = 0
        for x in self.start:
            x["tag"] = t; t += 1
        if shuffle is not None:
            random.Random(shuffle).shuffle(self.start)
        self.step_regs = []
        for s in steps:
            if s[0] == "hit":
                b = dict(s[1]); b["tag"] = t; t += 1
                self.step_regs.append(b)
            else:
                self.step_regs.append(None)
        self.cap = len(start) + len(steps)

    def start_words(self):
        return np.array([words(x, x["tag"]) for x in self.start], dtype=np.int64).reshape(-1, NW)

    def step_words(self):
        return np.array([words(b, b["tag"]) if b else [0] * NW for b in self.step_regs], dtype=np.int64).reshape(-1, NW)

    def hits(self):
        return np.array([1 if b else 0 for b in self.step_regs], dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------------ the judge
_ora = None
def ora():
    global _ora
    if _ora is None:
        _ora = C.CDLL(os.path.join(common.ROOT, "oracle", "liboracle.so"))
        _ora.ora_kat_mate_insert.argtypes = [C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _ora.ora_kat_mate_insert.restype = C.c_int
    return _ora


def oracle_replay(gap, mlr, start_w, hit, step_w):
    """ora_kat_mate_insert on one list: -> the final list's words (n x 19)."""
    start_w = np.ascontiguousarray(start_w, dtype=np.int64).reshape(-1, NW); step_w = np.ascontiguousarray(step_w, dtype=np.int64).reshape(-1, NW)
    hit = np.ascontiguousarray(hit, dtype=np.int32)
    out = np.zeros((len(start_w) + len(step_w) + 1, NW), dtype=np.int64)
    n = ora().ora_kat_mate_insert(gap, mlr, len(start_w), start_w.ctypes.data, len(step_w), hit.ctypes.data, step_w.ctypes.data, out.ctypes.data)
    return out[:n].copy()


def mask(w):
    """n_comp and secondary are not compared (tests/test_gpu_pe_stages.py: _mask_regs_pe gives the reason)."""
    w = np.array(w, dtype=np.int64).reshape(-1, NW).copy()
    w[:, W_SECONDARY] = 0; w[:, W_NCOMP] = 0
    return w


def _dicts(w):
    return [dict(rid=int(x[W_RID]), rb=int(x[W_RB]), re=int(x[W_RE]), qb=int(x[W_QB]), qe=int(x[W_QE]), score=int(x[W_SCORE]), tag=int(x[W_TAG])) for x in w]


class _params:
    """The model's GAP / MLR are module globals: set for the duration of a call, restored after it."""
    def __init__(self, gap, mlr): self.v = (gap, mlr)
    def __enter__(self): self.old = (model.GAP, model.MLR); model.GAP, model.MLR = self.v
    def __exit__(self, *a): model.GAP, model.MLR = self.old


def predict(item, gap, mlr, check_model=True):
    """What the device must do with the item as shipped (mode 0), step by step: 'incr' (incr_insert placed the region), 'score' (placed by
    score, the orientation ends in the full pass), 'none+full' / 'none' (no hit; with or without a full pass).  The list after every step
    is the oracle's.  -> (paths, lists): lists[0] = the start list as handed over, lists[t + 1] = the oracle's list after step t, as
    dicts.  With check_model, an incremental step's result by the Python model must be the oracle's list."""
    cur = item.start_words(); sw = item.step_words(); hit = item.hits()
    clean = False
    paths, lists = [], [_dicts(cur)]
    with _params(gap, mlr):
        for t, b in enumerate(item.step_regs):
            nxt = oracle_replay(gap, mlr, cur, hit[t:t + 1], sw[t:t + 1])
            general = not clean
            if b is not None:
                got = None if general else model.incr(_dicts(cur), b)
                if got is not None:
                    paths.append("incr")
                    if check_model:
                        assert model.key(got) == model.key(_dicts(nxt)), (item.name, t, "the model's incr_insert differs from the oracle")
                else:
                    general = True; paths.append("score")
            else:
                paths.append("none+full" if general else "none")
            if general:
                res = [int(x[W_RE]) for x in cur] + ([b["re"]] if b is not None else [])
                clean = len(set(res)) == len(res)
            cur = nxt
            lists.append(_dicts(cur))
    return paths, lists


def counts_of(paths):
    """(by incr_insert, by score, full passes) as bwahip_kat_mate_insert counts them."""
    return (paths.count("incr"), paths.count("score"), paths.count("score") + paths.count("none+full"))


# ------------------------------------------------------------------------------------------------------------------------ building blocks
def filler(n, base=50_000_000, spacing=30_000, rid=0, scores=None):
    """n regions that are out of each other's reach for every gap used here (30 kb apart), distinct `re`, scores with repeats."""
    return [reg(base + i * spacing, 100 + i % 13, scores[i] if scores else 30 + (i * 37) % 101, qb=i % 17, rid=rid) for i in range(n)]


def check_reason(item, paths, lists):
    """The item's reason for existing, asserted on the oracle's lists and on the predicted paths."""
    w = item.why
    final = lists[-1]
    tags = lambda l: set(x["tag"] for x in l)
    if "paths" in w: assert paths == w["paths"], (item.name, paths, w["paths"])
    if "path_at" in w:
        for t, p in w["path_at"].items(): assert paths[t] == p, (item.name, t, paths, p)
    if "no_incr" in w: assert "incr" not in paths, (item.name, paths)
    if "absent" in w: assert not (set(w["absent"]) & tags(final)), (item.name, "absent", w["absent"], sorted(tags(final)))
    if "present" in w: assert set(w["present"]) <= tags(final), (item.name, "present", w["present"], sorted(tags(final)))
    if "final_len" in w: assert len(final) == w["final_len"], (item.name, len(final), w["final_len"])
    if "pos_of" in w:
        tag, pos = w["pos_of"]
        assert [x["tag"] for x in final].index(tag) == pos, (item.name, "position", [x["tag"] for x in final].index(tag), pos)
    if "unchanged_at" in w:
        for t in w["unchanged_at"]: assert lists[t + 1] == lists[t], (item.name, "step", t, "changed the list")
    if "changed_at" in w:
        for t in w["changed_at"]: assert lists[t + 1] != lists[t], (item.name, "step", t, "changed nothing")
    if "min_dropped_at" in w:
        t, k = w["min_dropped_at"]
        assert len(tags(lists[t]) - tags(lists[t + 1])) >= k, (item.name, "step", t, "dropped", len(tags(lists[t]) - tags(lists[t + 1])), "<", k)


# ------------------------------------------------------------------------------------------------------------------------ the classes
def size_items():
    """Start lists at the wavefront's and the LDS list's edges.  216 + 8 steps is the largest capacity worked on in LDS; 223, 224, 225 and
    1000 are worked on in global memory and grow past 224 on the way.  Shuffled start, a duplicate and an `re` tie in some."""
    out = []
    for n in (0, 1, 2, 63, 64, 65, 128, 216, 223, 224, 225, 1000):
        f = filler(n)
        far = lambda k, sc: reg(10_000_000 + k * 30_000, 90 + k, sc, qb=3 + k)
        steps = [("none",), ("hit", far(0, 500)), ("hit", far(1, 1)), ("hit", far(2, 66)), ("none",), ("hit", far(3, 66)), ("hit", far(1, 1)), ("hit", far(4, 30))]
        # steps: sort the fresh list; top; end; middle; nothing; middle again; an exact duplicate of the one at the end (refused); after it
        out.append(Item(f"size{n}", f, steps, final_len=n + 5, path_at={0: "none+full", 1: "incr", 2: "incr", 3: "incr", 4: "none", 6: "score", 7: "score"},
                        unchanged_at=[4], shuffle=n))
        if n >= 2:
            dup = f + [dict(f[0]), dict(f[n // 2])]                  # two exact duplicates in the start list: the first pass removes them
            out.append(Item(f"size{n}+dups", dup, steps[:4], final_len=n + 3, path_at={0: "none+full", 1: "score"}, shuffle=n + 1))
    return out


def reach_items(gap):
    """0, 1, 63, 64, 65 entries within reach of b (none redundant with it: 150 bases apart, 100 long), all before b in `re` order, all
    after it, or on both sides; 65 are one too many for incr_insert, and the general path must give the same list."""
    out = []
    if gap < 10_000: return out
    C0 = 200_000_000
    for k in (0, 1, 63, 64, 65):
        for side in ("pred", "succ", "mixed"):
            cl = [reg(C0 + j * 150, 100, 40 + j % 50, qb=j % 9) for j in range(k)]
            at = {"pred": C0 + k * 150, "succ": C0 - 150, "mixed": C0 + (k // 2) * 150 - 75}[side]
            b = reg(at, 100, 70, qb=4)
            start = filler(20) + cl
            out.append(Item(f"reach{k}{side}", start, [("none",), ("hit", b), ("hit", reg(at + 20_000_000, 80, 90))], final_len=20 + k + 2,
                            paths=["none+full", "incr" if k <= 64 else "score", "incr"], present=[20 + k], shuffle=k))
    return out


def redundancy_items(gap, mlr, C0=300_000_000, tagp=""):
    """Every outcome of the redundancy rule for b (bwamem.c:459-470).  100-base regions with the same query interval are redundant while
    their starts differ by less than (1 - mlr) x 100."""
    out = []
    pre = filler(12, base=C0 + 40_000_000)
    n0 = len(pre)
    d_in = 1                                                    # start offset at which two 100-base regions are redundant for any mlr >= 0.5
    def item(name, cluster, b, **why):
        out.append(Item(tagp + name, pre + cluster, [("none",), ("hit", b)], **why, shuffle=len(name)))
    tb = lambda cluster: n0 + len(cluster)                       # b's tag
    # excluded by its nearest predecessor
    c = [reg(C0, 100, 100)]
    item("b_out_by_nearest_pred", c, reg(C0 + d_in, 100, 50), absent=[tb(c)], present=[n0], paths=["none+full", "incr"])
    # excluded by a far predecessor after it excluded a nearer one, which stays excluded
    c = [reg(C0, 100, 100, qb=10), reg(C0 + 50, 100, 40, qb=60)]
    item("b_out_by_far_pred", c, reg(C0 - 2, 200, 50, qb=8), absent=[tb(c), n0 + 1], present=[n0], paths=["none+full", "incr"])
    # excluded by a successor
    c = [reg(C0 + d_in, 100, 100)]
    item("b_out_by_succ", c, reg(C0, 100, 50), absent=[tb(c)], present=[n0], paths=["none+full", "incr"])
    # survives and excludes one predecessor / one successor
    c = [reg(C0, 100, 50)]
    item("b_drops_pred", c, reg(C0 + d_in, 100, 100), absent=[n0], present=[tb(c)], paths=["none+full", "incr"])
    c = [reg(C0 + d_in, 100, 50)]
    item("b_drops_succ", c, reg(C0, 100, 100), absent=[n0], present=[tb(c)], paths=["none+full", "incr"])
    # survives and excludes several: two short predecessors and a long successor (none redundant with another)
    c = [reg(C0, 20, 30, qb=10), reg(C0 + 25, 20, 31, qb=35), reg(C0 + 50, 960, 60, qb=59)]
    item("b_drops_several", c, reg(C0 - 1, 1000, 200, qb=9), absent=[n0, n0 + 1, n0 + 2], present=[tb(c)], paths=["none+full", "incr"], min_dropped_at=(1, 3))
    # survives and excludes 38 short predecessors lying along it: the compaction and the recomputed position run over several entries
    c = [reg(C0 + 25 * i, 20, 30 + i, qb=10 + 25 * i) for i in range(38)]
    item("b_drops_38", c, reg(C0 - 1, 1000, 200, qb=9), absent=list(range(n0, n0 + 38)), present=[tb(c)], paths=["none+full", "incr"], min_dropped_at=(1, 32), pos_of=(tb(c), 0))
    # ... and lands in the middle of the score order after the compaction (entries of higher score in front of it were not touched)
    hi = filler(70, base=C0 + 80_000_000, scores=[900 - i for i in range(70)])
    out.append(Item(tagp + "b_drops_38_mid", pre + hi + c, [("none",), ("hit", reg(C0 - 1, 1000, 200, qb=9))], absent=list(range(n0 + 70, n0 + 108)),
                    paths=["none+full", "incr"], min_dropped_at=(1, 32), pos_of=(n0 + 70 + 38, 70), shuffle=5))
    # equal scores on a redundant pair: the reference drops q, the earlier one in `re` order
    c = [reg(C0, 100, 77)]
    item("tie_b_later", c, reg(C0 + d_in, 100, 77), absent=[n0], present=[tb(c)], paths=["none+full", "incr"])
    c = [reg(C0 + d_in, 100, 77)]
    item("tie_b_earlier", c, reg(C0, 100, 77), absent=[tb(c)], present=[n0], paths=["none+full", "incr"])
    # overlaps on, and one base either side of, mlr x the shorter length: reference side (same query interval) and query side (same start + 1)
    thr = int(round((1 - mlr) * 100))                            # 5 at 0.95, 50 at 0.5: an overlap of 100 - thr is not above mlr x 100
    for d, red in ((thr - 1, True), (thr, False), (thr + 1, False)):
        c = [reg(C0, 100, 100)]
        item(f"ref_overlap_{100 - d}", c, reg(C0 + d, 100, 50), paths=["none+full", "incr"], **({"absent": [tb(c)]} if red else {"present": [tb(c), n0]}))
        c = [reg(C0, 100, 100, qb=10)]
        item(f"query_overlap_{100 - d}", c, reg(C0 + 1, 100, 50, qb=10 + d), paths=["none+full", "incr"], **({"absent": [tb(c)]} if red else {"present": [tb(c), n0]}))
    return out


def position_items():
    """Where b lands in the score order: first, in the middle, last; and so that the upward shift moves 64, 65, 120 and 128 entries (the
    shift goes 64 at a time from the top)."""
    out = []
    for n, pos in ((40, 0), (40, 17), (40, 40), (64, 0), (65, 0), (128, 64), (129, 64), (130, 10), (200, 72), (193, 1)):
        f = filler(n, scores=[3000 - 2 * i for i in range(n)])
        b = reg(9_000_000, 120, 3000 - 2 * pos + 1)
        out.append(Item(f"pos{pos}of{n}", f, [("none",), ("hit", b)], paths=["none+full", "incr"], pos_of=(n, pos), final_len=n + 1, shuffle=n + pos))
    return out


def refusal_items(gap):
    """Each condition under which incr_insert must refuse, alone; and for the other-contig window both sides of both ends."""
    out = []
    C0 = 400_000_000
    pre = filler(10, base=C0 + 40_000_000)
    n0 = len(pre)
    # b.re equal to an entry's (not redundant with it, other start and query interval)
    out.append(Item("same_re", pre + [reg(C0, 100, 60, qb=10)], [("none",), ("hit", reg(C0 + 60, 40, 50, qb=200)), ("hit", reg(C0 + 9_000_000, 50, 40))],
                    paths=["none+full", "score", "score"], present=[n0, n0 + 1]))   # the tie stays in the list: never clean again
    # (score, rb, qb) equal to an entry's, `re` not
    out.append(Item("same_key", pre + [reg(C0, 100, 60, qb=10)], [("none",), ("hit", reg(C0, 100, 60, qb=10, dre=3)), ("hit", reg(C0 + 9_000_000, 50, 40))],
                    paths=["none+full", "score", "incr"], final_len=n0 + 2))
    # the exact duplicate, the usual hit inside a repeat: refused, removed by the full pass, after which the list is clean again one orientation later
    out.append(Item("exact_dup", pre + [reg(C0, 100, 60, qb=10)], [("none",), ("hit", reg(C0, 100, 60, qb=10)), ("hit", reg(C0 + 9_000_000, 50, 40)), ("hit", reg(C0 + 9_500_000, 50, 41))],
                    paths=["none+full", "score", "score", "incr"], final_len=n0 + 3))
    # an entry of another contig at the ends of the window b.rb - gap - 1 < re < b.re + gap + 65536
    b = reg(C0, 100, 50)
    for name, re_, inside in (("lo_out", b["rb"] - gap - 1, False), ("lo_in", b["rb"] - gap, True), ("hi_in", b["re"] + gap + 65535, True), ("hi_out", b["re"] + gap + 65536, False)):
        y = reg(re_ - 100, 100, 55, rid=1)
        out.append(Item(f"other_contig_{name}", pre + [y], [("none",), ("hit", b), ("hit", reg(C0 + 9_000_000, 50, 40))], paths=["none+full", "score" if inside else "incr", "incr"],
                        final_len=n0 + 3))
    # a start list whose `re` tie survives the first pass: never clean, no step may be incremental
    tie = [reg(C0, 100, 60, qb=10), reg(C0 + 60, 40, 50, qb=200)]
    out.append(Item("start_tie_stays", pre + tie, [("none",), ("hit", reg(C0 + 9_000_000, 50, 40)), ("none",), ("hit", reg(C0 + 9_500_000, 50, 41))],
                    no_incr=True, paths=["none+full", "score", "none+full", "score"], present=[n0, n0 + 1], shuffle=3))
    return out


def state_items():
    """The clean flag across steps: sequences of 1 to 12 steps that mix hits and orientations without one."""
    out = []
    C0 = 500_000_000
    pre = filler(30, base=C0 + 40_000_000)
    far = lambda k, sc=45: reg(C0 + 1_000_000 + 25_000 * k, 80 + k, sc + k, qb=k)
    out.append(Item("one_none_fresh", pre + [dict(pre[3])], [("none",)], paths=["none+full"], changed_at=[0], final_len=30, shuffle=1))
    out.append(Item("one_hit_fresh", pre, [("hit", far(0))], paths=["score"], final_len=31, shuffle=2))
    out.append(Item("none_on_clean", pre, [("none",), ("none",), ("hit", far(0)), ("none",)], paths=["none+full", "none", "incr", "none"], unchanged_at=[1, 3], changed_at=[0], shuffle=3))
    cl = [reg(C0 + j * 150, 100, 40 + j % 50, qb=j % 9) for j in range(65)]
    out.append(Item("refused_then_accepted", pre + cl, [("none",), ("hit", reg(C0 + 65 * 150, 100, 70)), ("hit", far(1)), ("hit", far(2)), ("none",), ("hit", far(3))],
                    paths=["none+full", "score", "incr", "incr", "none", "incr"], final_len=30 + 65 + 4, shuffle=4))
    rng = random.Random(11)
    for n_steps in range(1, 13):
        steps = []
        for t in range(n_steps):
            r = rng.random()
            if r < 0.3: steps.append(("none",))
            elif r < 0.5: steps.append(("hit", dict(rng.choice(pre))))                          # a duplicate of a start entry
            elif r < 0.7: steps.append(("hit", reg(pre[rng.randrange(30)]["rb"] + rng.randint(-6, 6), 100, rng.randint(20, 140), qb=rng.randint(0, 16))))   # near a start entry
            else: steps.append(("hit", far(10 + t, rng.randint(20, 120))))
        out.append(Item(f"mixed{n_steps}", pre, steps, shuffle=20 + n_steps))
    return out


def coordinate_items(gap, mlr):
    """Coordinates above 2^32 (the reverse strand of a 3.1 Gbp genome) and both strands of one contig in the same list."""
    hi = 2 * L_PAC - 600_000_000                                   # 5.6e9
    assert hi > 1 << 32
    out = redundancy_items(gap, mlr, C0=hi, tagp="rev_")
    fw, rv = 700_000_000, 2 * L_PAC - 700_000_100                # the same place seen from both strands
    both = [reg(fw, 100, 60), reg(rv, 100, 61), reg(fw + 300, 100, 50), reg(rv - 300, 100, 51)]
    out.append(Item("both_strands", filler(8) + both, [("none",), ("hit", reg(fw + 1, 100, 90)), ("hit", reg(rv + 1, 100, 20)), ("hit", reg(rv + 500_000_000, 100, 33))],
                    paths=["none+full", "incr", "incr", "incr"], absent=[8, 8 + 4 + 1], shuffle=6))
    return out


def random_items(seed=7, n_items=600, n_steps=30):
    """The generator of tests/test_incr_insert_model.py -- clustered regions, two contigs, a contig boundary within reach, equal scores --
    with start lists of up to 300 regions, left in the arrangement they were drawn in; every eighth item keeps its `re` ties, every tenth
    step is an orientation without a hit."""
    rng = random.Random(seed)
    out = []
    for trial in range(n_items):
        big = trial % 5 == 4
        centers = [rng.randint(0, 4_990_000) for _ in range(rng.randint(4, 12) if big else rng.randint(1, 4))] + [rng.randint(5_000_100, 9_000_000) for _ in range(rng.randint(0, 2))]
        if rng.random() < 0.2: centers.append(4_999_000); centers.append(5_000_500)          # a contig boundary nearby
        L = [model.rnd_reg(rng, centers) for _ in range(rng.randint(41, 300) if big else rng.randint(0, 40))]
        if trial % 8 != 7:                                           # tie-free start
            seen = set(); L2 = []
            for x in L:
                if x["re"] in seen: continue
                seen.add(x["re"]); L2.append(x)
            L = L2
        steps = [("none",) if rng.random() < 0.1 else ("hit", model.rnd_reg(rng, centers)) for _ in range(n_steps)]
        out.append(Item(f"rnd{trial}", L, steps))
    return out


# ------------------------------------------------------------------------------------------------------------------------ the sets
# name -> (max_chain_gap, mask_level_redun, builder); one launch per set, mode and address space
SETS = {
    "sizes": (10_000, 0.95, size_items),
    "reach": (10_000, 0.95, lambda: reach_items(10_000)),
    "redundancy_095": (10_000, 0.95, lambda: redundancy_items(10_000, 0.95) + position_items()),
    "redundancy_050": (10_000, 0.5, lambda: redundancy_items(10_000, 0.5)),
    "refusals": (10_000, 0.95, lambda: refusal_items(10_000)),
    "state": (10_000, 0.95, state_items),
    "coordinates": (10_000, 0.95, lambda: coordinate_items(10_000, 0.95)),
    "gap0": (0, 0.95, lambda: redundancy_items(0, 0.95) + refusal_items(0) + coordinate_items(0, 0.95)),
}


def pack(items):
    """-> (list_off, list_words, step_off, step_hit, step_words) for bwahip_kat_mate_insert."""
    list_off = np.zeros(len(items) + 1, dtype=np.int64); step_off = np.zeros(len(items) + 1, dtype=np.int64)
    lw, sw, sh = [], [], []
    for i, it in enumerate(items):
        list_off[i + 1] = list_off[i] + len(it.start); step_off[i + 1] = step_off[i] + len(it.steps)
        lw.append(it.start_words()); sw.append(it.step_words()); sh.append(it.hits())
    cat = lambda l, w: np.concatenate(l) if l else np.zeros((0, w), dtype=np.int64)
    return list_off, cat(lw, NW).reshape(-1, NW), step_off, np.concatenate(sh) if sh else np.zeros(0, dtype=np.int32), cat(sw, NW).reshape(-1, NW)


def oracle_lists(items, gap, mlr):
    return [oracle_replay(gap, mlr, it.start_words(), it.hits(), it.step_words()) for it in items]
# random_items() at its default seed under (10 000, 0.95), by `predict`: regions placed by incr_insert, placed by score, full passes
# (tests/test_mate_insert_cases_cpu.py recomputes them; tests/test_gpu_mate_insert.py asserts them on the device)
RANDOM_COUNTS = (12851, 3397, 3610)
