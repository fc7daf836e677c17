"""Shared by the known-answer tests of the two DP forms (ksw_extend2, ksw_global2): the reference-made records of
tests/golden/kat_ksw.npz and kat_dp_wide.npz as cases, liboracle.so through ctypes as the judge, seeded random cases over the range
the oracle was checked against the reference on (tests), and the packing the device entries take."""
import ctypes as C
import os
import numpy as np
import common
from common import bw

TAG_EXT, TAG_GLB, TAG_EXT_W, TAG_GLB_W = 20, 21, 24, 25
MATRICES = [(1, 4), (2, 3), (1, 1), (3, 9), (50, 60)]
GAPS = [(6, 1, 6, 1), (4, 2, 7, 1), (1, 1, 1, 1), (16, 1, 16, 1), (0, 1, 0, 1)]
BANDS = [0, 1, 2, 5, 20, 31, 32, 63, 64, 100, 127, 400]
ZDROPS = [0, 1, 10, 100, 1000]
BONUSES = [0, 5, 50]
CPLS = [3, 4, 5, 11]


def scmat(a, b):
    """bwa_fill_scmat (bwa.c:252)."""
    m = np.full((5, 5), -1, dtype=np.int8)
    m[:4, :4] = -b
    m[np.arange(4), np.arange(4)] = a
    return m.reshape(25)


class Case:
    """One DP call: the inputs of ksw_extend2 (kind 'ext') or ksw_global2 (kind 'glb'), and -- for a record -- the reference's results."""
    __slots__ = ("kind", "qlen", "tlen", "w", "h0", "zdrop", "bonus", "gaps", "mat", "q", "t", "res", "fam")

    def __init__(self, kind, q, t, w, gaps, mat, h0=0, zdrop=0, bonus=0, res=None, fam=""):
        self.kind, self.q, self.t = kind, np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)
        self.qlen, self.tlen, self.w, self.h0, self.zdrop, self.bonus = len(self.q), len(self.t), int(w), int(h0), int(zdrop), int(bonus)
        self.gaps, self.mat, self.res, self.fam = tuple(int(x) for x in gaps), np.ascontiguousarray(mat, dtype=np.int8), res, fam

    def reversed(self):
        """Both sequences backwards, fed forward: what a device call with reverse = 1 on this case must equal."""
        return Case(self.kind, self.q[::-1], self.t[::-1], self.w, self.gaps, self.mat, self.h0, self.zdrop, self.bonus, None, self.fam)

    def __repr__(self):
        return (f"{self.kind}[{self.fam}] qlen={self.qlen} tlen={self.tlen} w={self.w} h0={self.h0} zdrop={self.zdrop} bonus={self.bonus} gaps={self.gaps} "
                f"mat={self.mat[0]}/{self.mat[1]}")


def load_records(name):
    """The ksw_extend2 / ksw_global2 records of a fixture as (ext cases, glb cases).  kat_ksw.npz: 1/-4 matrix; kat_dp_wide.npz: per record."""
    ext, glb = [], []
    for tag, v in bw.parse_records(np.load(os.path.join(common.GOLDEN, name))["words"]):
        if tag not in (TAG_EXT, TAG_GLB, TAG_EXT_W, TAG_GLB_W):
            continue
        qlen, tlen, w, h0, zdrop, bonus = (int(x) for x in v[:6])
        wide = tag in (TAG_EXT_W, TAG_GLB_W)
        mat, s = (v[10:35], 35) if wide else (scmat(1, 4), 10)
        c = Case("ext" if tag in (TAG_EXT, TAG_EXT_W) else "glb", v[s:s + qlen], v[s + qlen:s + qlen + tlen], w, v[6:10], mat, h0, zdrop, bonus,
                 [int(x) for x in v[s + qlen + tlen:]], name)
        (ext if c.kind == "ext" else glb).append(c)
    return ext, glb


class Oracle:
    """ora_ksw_extend2 / ora_ksw_global2 of liboracle.so."""

    def __init__(self):
        self.lib = C.CDLL(os.path.join(common.ROOT, "oracle", "liboracle.so"))
        vp, ip = C.c_void_p, C.POINTER(C.c_int)
        self.lib.ora_ksw_extend2.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 8 + [ip] * 5
        self.lib.ora_ksw_global2.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 5 + [ip, C.POINTER(C.POINTER(C.c_uint32))]
        self.libc = C.CDLL(None)
        self.libc.free.argtypes = [C.c_void_p]

    def extend(self, c):
        """[score, qle, tle, gtle, gscore, max_off]"""
        o = [C.c_int() for _ in range(5)]
        sc = self.lib.ora_ksw_extend2(c.qlen, c.q.ctypes.data, c.tlen, c.t.ctypes.data, 5, c.mat.ctypes.data, *c.gaps, c.w, c.bonus, c.zdrop, c.h0,
                                      *[C.byref(x) for x in o])
        return [sc] + [x.value for x in o]

    def global2(self, c):
        """[score, n_cigar, words...]"""
        n, cig = C.c_int(), C.POINTER(C.c_uint32)()
        sc = self.lib.ora_ksw_global2(c.qlen, c.q.ctypes.data, c.tlen, c.t.ctypes.data, 5, c.mat.ctypes.data, *c.gaps, c.w, C.byref(n), C.byref(cig))
        out = [sc, n.value] + [int(cig[i]) for i in range(n.value)]
        self.libc.free(cig)
        return out

    def answer(self, c):
        return self.extend(c) if c.kind == "ext" else self.global2(c)


# ------------------------------------------------------------------------------------------------ seeded random cases
def rand_query(rng, n, n_frac=0.0):
    q = rng.integers(0, 4, n).astype(np.uint8)
    if n_frac > 0:
        q[rng.random(n) < n_frac] = 4
    return q


def mutate(rng, q, tlen, err, n_frac=0.0, max_gap=40):
    """A target of tlen bases: the query with substitutions (60 % of the errors), indels of 1 to 3 bases and, one error in ten, a gap of
    up to max_gap bases; cut or filled with random bases to tlen."""
    t = q.copy()
    t[t > 3] = 0
    n_ev = int(rng.binomial(len(q), err))
    for _ in range(n_ev):
        if len(t) == 0:
            break
        p = int(rng.integers(0, len(t)))
        k = rng.random()
        if k < 0.6:
            t[p] = (t[p] + 1 + rng.integers(0, 3)) & 3
        else:
            g = int(rng.integers(1, max_gap + 1)) if rng.random() < 0.25 else int(rng.integers(1, 4))
            t = np.delete(t, slice(p, p + g)) if k < 0.8 else np.insert(t, p, rng.integers(0, 4, g).astype(np.uint8))
    t = t[:tlen] if len(t) >= tlen else np.concatenate([t, rng.integers(0, 4, tlen - len(t)).astype(np.uint8)])
    if n_frac > 0:
        t[rng.random(tlen) < n_frac] = 4
    return t.astype(np.uint8)


def rand_len(rng):
    """1 .. 700, a third of the draws on the lengths where a device form changes."""
    k = rng.integers(0, 3)
    if k == 0:
        return int(rng.choice([1, 2, 63, 64, 65, 127, 128, 191, 192, 255, 256, 700]))
    return int(rng.integers(1, 701)) if k == 1 else int(rng.integers(1, 251))


def rand_case(rng, kind, qlen=None, max_n=0.05, fam="random", **fixed):
    """A case drawn as the oracle-versus-reference check drew them; `fixed` pins fields (w, h0, zdrop, bonus, gaps, ab, err, tlen)."""
    qlen = rand_len(rng) if qlen is None else qlen
    tlen = fixed.get("tlen", max(1, qlen + int(rng.integers(-40, 81))))
    err = fixed.get("err", rng.uniform(0, 0.08) if rng.random() < 0.75 else rng.uniform(0, 0.30))
    n_frac = rng.uniform(0, max_n) if rng.random() < 0.2 else 0.0
    q = rand_query(rng, qlen, n_frac)
    t = mutate(rng, q, tlen, err, n_frac)
    a, b = fixed.get("ab", MATRICES[rng.integers(0, 5)])
    gaps = fixed.get("gaps", GAPS[rng.integers(0, 5)])
    w = fixed.get("w", BANDS[rng.integers(0, 12)])
    if kind == "glb":
        return Case("glb", q, t, max(w, abs(tlen - qlen) + 3), gaps, scmat(a, b), fam=fam)
    h0 = fixed.get("h0", int(rng.integers(1, 5001)) if rng.random() < 0.5 else int(rng.integers(1, 121)))
    return Case("ext", q, t, w, gaps, scmat(a, b), h0, fixed.get("zdrop", ZDROPS[rng.integers(0, 5)]), fixed.get("bonus", BONUSES[rng.integers(0, 3)]), fam=fam)


# ------------------------------------------------------------------------------------------------ device calls
def pack(cases):
    qoff = np.concatenate([[0], np.cumsum([c.qlen for c in cases])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([c.tlen for c in cases])]).astype(np.int64)
    return (np.stack([c.mat for c in cases]), np.concatenate([c.q for c in cases]), qoff, np.concatenate([c.t for c in cases]), toff)


def device_global(ctx, cases, form, reverse=0, cpl=0):
    """[score, n_cigar, words...] per case (n_cigar -1: does not fit the form)."""
    params = [[c.qlen, c.tlen, c.w, *c.gaps, reverse, form, cpl] for c in cases]
    out, cig = ctx.kat_ksw_global(params, *pack(cases))
    return [[int(out[i, 0]), int(out[i, 1])] + [int(x) for x in cig[i, :max(0, out[i, 1])]] for i in range(len(cases))]


def device_extend(ctx, cases, cpl, reverse=0):
    """([score, qle, tle, gtle, gscore, max_off] per case, path masks)"""
    params = [[c.qlen, c.tlen, c.w, c.h0, c.zdrop, c.bonus, *c.gaps, reverse, cpl] for c in cases]
    out = ctx.kat_ksw_extend2(params, *pack(cases))
    return [[int(x) for x in out[i, :6]] for i in range(len(cases))], out[:, 6].copy()
