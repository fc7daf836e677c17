"""The table jump of bwt_smem1a ("k_smem: the short-string triangle skipped by table jumps") pinned without a GPU:
tests/smem_skip_model.c restates bwt_smem1a with the jump, the dormant entries and the fallback on top of liboracle.so's ora_set_intv and
ora_extend, and ora_smem1a is the judge: for every call the return value and the whole list (x0, x1, x2, info) must be the same, bit for
bit.  Every ACGT x of every read is a call, on the 1 Mbp three-contig index of the small_index fixture (log4 of the text is about 10.5, so
a depth of 11 falls back often and a depth of 5 almost never).  The model also counts what the kernel pays: the plain path's bwt_extend
calls against the skip path's extends plus look-ups plus the turns of abandoned attempts."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import common
from common import bw

HERE = os.path.dirname(os.path.abspath(__file__))
ORA_DIR = os.path.join(common.ROOT, "oracle")
STATS = ["calls", "can_jump", "jumped", "fallbacks", "lookups", "plain_turns", "skip_turns", "abandoned_turns", "diff", "first_diff_read", "first_diff_x"]
MIN_INTVS = [1, 2, 3, 6, 11]
DEPTHS = [2, 5, 8, 11]


class Model:
    def __init__(self, tmpdir, prefix):
        so = os.path.join(str(tmpdir), "libssk_model.so")
        subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + ORA_DIR, "-o", so, os.path.join(HERE, "smem_skip_model.c"),
                        "-L" + ORA_DIR, "-loracle", "-Wl,-rpath," + ORA_DIR], check=True)
        self.ora = C.CDLL(os.path.join(ORA_DIR, "liboracle.so"), mode=C.RTLD_GLOBAL)
        self.lib = C.CDLL(so)
        vp, lp = C.c_void_p, C.POINTER(C.c_long)
        self.ora.ora_index_load.restype = C.POINTER(C.c_void_p)        # ora_index_t: { fmi, ref }
        self.ora.ora_index_load.argtypes = [C.c_char_p]
        self.lib.ssk_compare_every_x.restype = C.c_long
        self.lib.ssk_compare_every_x.argtypes = [vp, C.c_long, vp, vp, C.c_int, C.c_int, lp]
        self.lib.ssk_collect.restype = C.c_long
        self.lib.ssk_collect.argtypes = [vp, C.c_long, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, lp, lp, lp, C.c_int]
        idx = self.ora.ora_index_load(prefix.encode())
        assert idx
        self.fmi = idx[0]

    def every_x(self, reads, min_intv, depth):
        codes, off = reads
        st = (C.c_long * len(STATS))()
        self.lib.ssk_compare_every_x(self.fmi, len(off) - 1, codes.ctypes.data, off.ctypes.data, min_intv, depth, st)
        return dict(zip(STATS, st))

    def collect(self, reads, depth, min_seed_len=19, split_factor=1.5, split_width=10, n_by_intv=16):
        codes, off = reads
        s1, s2 = (C.c_long * len(STATS))(), (C.c_long * len(STATS))()
        by = (C.c_long * (2 * n_by_intv))()
        self.lib.ssk_collect(self.fmi, len(off) - 1, codes.ctypes.data, off.ctypes.data, min_seed_len, split_factor, split_width, depth, s1, s2, by, n_by_intv)
        return dict(zip(STATS, s1)), dict(zip(STATS, s2)), [(by[2 * m], by[2 * m + 1]) for m in range(n_by_intv)]


def load_genome(fa):
    """the contigs as code arrays (0-3, 4 = N)"""
    ctg, cur = [], []
    with open(fa, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if cur:
                    ctg.append(b"".join(cur))
                cur = []
            else:
                cur.append(line.strip())
    ctg.append(b"".join(cur))
    return [bw.NT4[np.frombuffer(c, dtype=np.uint8)].astype(np.uint8) for c in ctg]


def revcomp(s):
    r = s[::-1].copy()
    r[r < 4] = 3 - r[r < 4]
    return r


def repeat_starts(g, k=24, min_copies=4):
    """positions of one contig whose k-mer occurs at least min_copies times in it: tandem repeats and the dispersed families"""
    n = len(g) - k + 1
    code = np.zeros(n, dtype=np.uint64)
    bad = np.zeros(n, dtype=bool)
    for j in range(k):
        code = code << np.uint64(2) | (g[j:j + n] & 3).astype(np.uint64)
        bad |= g[j:j + n] > 3
    _, inv, cnt = np.unique(code, return_inverse=True, return_counts=True)
    return np.flatnonzero((cnt[inv] >= min_copies) & ~bad)


def cut(rng, ctgs, n, lens, sub, n_rate=0.0, starts=None):
    """n reads cut from the genome (either strand), lengths drawn from lens, substitutions and N at the given rates"""
    out = []
    while len(out) < n:
        ln = int(rng.choice(lens))
        if starts is None:
            g = ctgs[int(rng.integers(len(ctgs)))]
            at = int(rng.integers(0, len(g) - ln))
        else:
            g = ctgs[0]
            at = min(max(0, int(rng.choice(starts)) - int(rng.integers(0, ln))), len(g) - ln)
        s = g[at:at + ln].copy()
        if (s > 3).mean() > 0.5:
            continue
        m = (rng.random(ln) < sub) & (s < 4)
        s[m] = (s[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
        s[rng.random(ln) < n_rate] = 4
        out.append(revcomp(s) if rng.integers(2) else s)
    return out


def packed(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.ascontiguousarray(np.concatenate(reads), dtype=np.uint8), off


@pytest.fixture(scope="module")
def model(small_index, tmp_path_factory):
    return Model(tmp_path_factory.mktemp("ssk"), small_index["prefix"])


@pytest.fixture(scope="module")
def families(small_index):
    rng = np.random.default_rng(20240607)
    ctgs = load_genome(small_index["fa"])
    reps = repeat_starts(ctgs[0])
    assert len(reps) > 1000
    half = cut(rng, ctgs, 3, [75], 0.0)
    half = [h for h in half if (h < 4).all()] or [np.arange(75, dtype=np.uint8) & 3]
    fam = {
        "150 bp, 1 %": cut(rng, ctgs, 40, [150], 0.01),
        "150 bp, 5 %": cut(rng, ctgs, 40, [150], 0.05),
        "19-40 bases": cut(rng, ctgs, 120, list(range(19, 41)), 0.01),
        "2 % N": cut(rng, ctgs, 40, [150], 0.01, 0.02),
        "repeats": cut(rng, ctgs, 40, [150], 0.01, starts=reps),
        "fewer than J bases": cut(rng, ctgs, 150, list(range(1, 13)), 0.0),       # (and the last J - 1 starts of every other read)
        "N inside the first J": cut(rng, ctgs, 30, [150], 0.01, 0.12),
        "own reverse complement": [np.concatenate([h, revcomp(h)]) for h in half],
    }
    return {k: packed(v) for k, v in fam.items()}


@pytest.fixture(scope="module")
def runs(model, families):
    """every family under every (min_intv, depth) once"""
    jobs = [(f, m, j) for f in families for m in MIN_INTVS for j in DEPTHS]
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda a: model.every_x(families[a[0]], a[1], a[2]), jobs))
    return dict(zip(jobs, res))


def test_every_call_equals_ora_smem1a(runs, families):
    for fam in families:
        for j in DEPTHS:
            tot = {k: sum(runs[(fam, m, j)][k] for m in MIN_INTVS) for k in STATS[:9]}
            print(f"\n{fam}, J = {j}: {tot}  turns skip / plain = {tot['skip_turns'] / max(1, tot['plain_turns']):.3f}")
    assert sum(st["calls"] for st in runs.values()) >= 300000
    for key, st in runs.items():
        assert st["diff"] == 0, (key, st)
        assert st["calls"] > 0 and st["jumped"] + st["fallbacks"] == st["can_jump"] <= st["calls"], (key, st)


def test_the_jump_is_alive_in_every_family(runs, families):
    """not vacuous: in every family the jump is attempted, and is carried through, in at least a tenth of the calls (the grid of min_intv and
    depths taken together); a depth of 11 falls back in at least 1 000 calls (a string of 11 bases occurs 0.5 times on average in this text),
    a depth of 5 in fewer than 1 % of them."""
    for fam in families:
        calls = sum(runs[(fam, m, j)]["calls"] for m in MIN_INTVS for j in DEPTHS)
        can = sum(runs[(fam, m, j)]["can_jump"] for m in MIN_INTVS for j in DEPTHS)
        done = sum(runs[(fam, m, j)]["jumped"] for m in MIN_INTVS for j in DEPTHS)
        print(f"\n{fam}: {calls} calls, {can} could jump, {done} did")
        assert can >= calls // 10 and done >= calls // 10, (fam, calls, can, done)
    fb11 = sum(st["fallbacks"] for (f, m, j), st in runs.items() if j == 11)
    fb5 = sum(st["fallbacks"] for (f, m, j), st in runs.items() if j == 5)
    calls5 = sum(st["calls"] for (f, m, j), st in runs.items() if j == 5)
    print(f"\nfallbacks at J = 11: {fb11}; at J = 5: {fb5} of {calls5} calls")
    assert fb11 >= 1000
    assert fb5 * 100 < calls5


def test_edge_families_meet_their_edge(runs, families):
    """reads with fewer than J bases after x and reads with an N inside the first J bases must really hold calls that cannot jump, next to
    calls that can"""
    for fam in ("fewer than J bases", "N inside the first J"):
        st = runs[(fam, 1, 8)]
        assert st["calls"] - st["can_jump"] >= st["calls"] // 4 and st["can_jump"] > 0, (fam, st)
    st = runs[("150 bp, 1 %", 1, 8)]
    assert st["calls"] - st["can_jump"] >= 7 * 40          # the last J - 1 starts of every read


def test_call_pattern_of_mem_collect_intv(model, families):
    """passes 1 and 2 as bwamem.c:144-165 make their calls, the depth clamped to min_seed_len (-k 10 under a depth of 11); the ratio of
    turns per family is printed"""
    for fam, reads in families.items():
        for depth, k in ((8, 19), (11, 19), (11, 10), (5, 19)):
            s1, s2, _ = model.collect(reads, depth, min_seed_len=k)
            assert s1["diff"] == 0 and s2["diff"] == 0, (fam, depth, k, s1, s2)
            plain, skip = s1["plain_turns"] + s2["plain_turns"], s1["skip_turns"] + s2["skip_turns"]
            print(f"\n{fam}, J = {depth}, -k {k}: pass 1 {s1['calls']} calls, pass 2 {s2['calls']} calls, turns {plain} -> {skip} ({skip / max(1, plain):.3f}), "
                  f"fallbacks {s1['fallbacks']} + {s2['fallbacks']}")
    s1, s2, _ = model.collect(families["150 bp, 1 %"], 8)
    assert s1["jumped"] > 0 and s2["calls"] > 0
