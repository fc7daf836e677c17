"""Paired-end libraries the read simulator cannot make (it draws FR pairs of one length with fragments ~ N(500, 50^2)), as a small
deterministic generator over the test genome, and what each library is meant to exercise, checked on the CPU path's stage records.

A fragment is a stretch of one contig, taken from either strand with equal probability.  On the fragment F of length L the mates are
    FF: F[:l1], F[L-l2:]        FR: F[:l1], rc(F[L-l2:])        RF: rc(F[:l1]), F[L-l2:]        RR: F[L-l1:], F[:l2]
which are the four classes of infer_dir (bwamem_pair.c:48) whichever strand F came from.  One mate of about a third of the pairs is made
`noisy`: substitutions so dense that no exact match reaches the minimum seed length, so the mate has no region of its own and can only
be placed by mate rescue (mem_matesw, bwamem_pair.c:137)."""
import os
import subprocess
import numpy as np
import common
from common import bw

STAGE_REGS, STAGE_PESTAT, STAGE_REGS_PE, STAGE_PAIR = 4, 7, 8, 9
FF, FR, RF, RR = 0, 1, 2, 3
_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def rc(s):
    return s.translate(_RC)[::-1]


def load_genome(fa):
    """FASTA -> list of contig sequences (bytes, upper case)."""
    ctg, cur = [], []
    with open(fa, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if cur:
                    ctg.append(b"".join(cur))
                cur = []
            else:
                cur.append(line.strip().upper())
    ctg.append(b"".join(cur))
    return ctg


def _mutate(rng, s, sub, indel, nrate, max_run=0):
    """Substitutions / one-base indels / Ns at the given rates per base; max_run > 0: no stretch of max_run unchanged bases remains."""
    a = bytearray(s)
    out = bytearray()
    run = 0
    for c in a:
        u = rng.random()
        if u < indel:
            if rng.random() < .5:
                run = 0
                continue                                        # deletion
            out.append(b"ACGT"[int(rng.integers(0, 4))])        # insertion in front of the base
            run = 0
        if rng.random() < nrate:
            out.append(ord("N")); run = 0
            continue
        if rng.random() < sub or (max_run and run >= max_run - 1):
            alt = [x for x in b"ACGT" if x != c]
            out.append(alt[int(rng.integers(0, 3))]); run = 0
            continue
        out.append(c); run += 1
    return bytes(out)


def make_library(genome, seed, n_pairs, orient=(0, 1, 0, 0), frag=(500, 50), frag_clip=(300, 700), len1=150, len2=150, forced_lens=(),
                 forced_copies=3, noisy_share=1 / 3, noisy_orient=None, clean=(.005, .0005, .0005), noisy=(.02, .0, .0), noisy_max_run=15,
                 edge_share=0., edge_within=700, flush_share=0.):
    """-> (reads1, reads2, meta): two lists of ASCII reads and, per pair, (orientation class, contig, fragment start, fragment length,
    strand of F, noisy mate or -1).
      orient         weights of the classes FF, FR, RF, RR: each pair draws its class, except that the first pairs are dealt out so that
                     a class with a weight gets round(weight * n_pairs) pairs exactly (the counts near MIN_DIR_CNT must not wobble)
      frag           mean, sd of the fragment length (normal, clipped to frag_clip and to what holds both mates)
      len1 / len2    length of mate 1 / 2: an int, or (lo, hi) drawn per read
      forced_lens    mate lengths each given to the NOISY mate of forced_copies pairs
      clean / noisy  (substitution, indel, N) rates per base of an ordinary / a noisy mate; a noisy mate keeps no run of noisy_max_run
                     unchanged bases (below the default minimum seed length of 19)
      noisy_orient   classes whose pairs may get a noisy mate (None: all)
      edge_share     share of fragments that begin within edge_within bases of a contig's start or end within them of its end, of which
      flush_share    end within 8 bases of the contig's end (a rescue window around such an anchor has its middle in the next contig)"""
    rng = np.random.default_rng(seed)
    w = np.asarray(orient, float) / sum(orient)
    cls = np.concatenate([np.full(int(round(w[d] * n_pairs)), d) for d in range(4)])[:n_pairs]
    cls = np.concatenate([cls, np.full(n_pairs - len(cls), int(np.argmax(w)))]).astype(int)
    rng.shuffle(cls)
    may = [i for i in range(n_pairs) if noisy_orient is None or cls[i] in noisy_orient]
    noisy_pairs = set(int(x) for x in rng.choice(may, int(round(noisy_share * n_pairs)), replace=False)) if may else set()
    forced = {}
    for k, p in enumerate(sorted(noisy_pairs)[:len(forced_lens) * forced_copies]):
        forced[p] = forced_lens[k % len(forced_lens)]
    clen = np.array([len(c) for c in genome], float)

    def draw_len(spec):
        return int(spec) if np.isscalar(spec) else int(rng.integers(spec[0], spec[1] + 1))
    r1, r2, meta = [], [], []
    for i in range(n_pairs):
        l1, l2 = draw_len(len1), draw_len(len2)
        nm = int(rng.integers(0, 2)) if i in noisy_pairs else -1
        if i in forced:
            if nm == 0:
                l1 = forced[i]
            else:
                l2 = forced[i]
        while True:
            L = int(round(rng.normal(frag[0], frag[1])))
            L = max(frag_clip[0], min(frag_clip[1], L), l1, l2)
            c = int(rng.choice(len(genome), p=clen / clen.sum()))
            n = len(genome[c])
            u = rng.random()
            if u < edge_share:
                d = int(rng.integers(0, 8 if rng.random() < flush_share else edge_within))
                s = d if rng.random() < .5 else n - L - d
            else:
                s = int(rng.integers(0, n - L + 1))
            if 0 <= s <= n - L and genome[c][s:s + L].count(b"N") * 4 < L:
                break
        strand = int(rng.integers(0, 2))
        F = genome[c][s:s + L]
        if strand:
            F = rc(F)
        d = cls[i]
        a, b = ((F[:l1], F[L - l2:]), (F[:l1], rc(F[L - l2:])), (rc(F[:l1]), F[L - l2:]), (F[L - l1:], F[:l2]))[d]
        mates = [a, b]
        for k in range(2):
            if k == nm:
                mates[k] = _mutate(rng, mates[k], *noisy, max_run=noisy_max_run)
            else:
                mates[k] = _mutate(rng, mates[k], *clean)
        r1.append(mates[0]); r2.append(mates[1])
        meta.append((int(d), c, s, L, strand, nm))
    return r1, r2, meta


def write_fastq(path, reads, tag="p"):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@%s%d\n%s\n+\n%s\n" % (tag.encode(), i, r, b"I" * len(r)))


# ---------------------------------------------------------------------------------------------------- the named libraries
# window: the class of mem_matesw's reference window high - low + mate length (bwamem_pair.c:153-160) for a 150-base mate, by the limits of
# the rescue kernels: up to 1024 bases the alignments are run ahead of the sequential pass, up to 4096 the window is held in LDS, beyond
# that in a slab in global memory.  failed: mem_pestat's verdict per class (FF, FR, RF, RR).  The seeds were chosen with bwa_oracle so that
# preconditions() holds; nothing here was looked up in a GPU result.
BOUNDARY_LENS = (160, 161, 249, 250, 256, 257, 124, 125)
LIBRARIES = {
    "rf":          dict(seed=301, n_pairs=500, orient=(0, 0, 1, 0), failed=(1, 1, 0, 1), window="ahead"),
    "ff_rr":       dict(seed=302, n_pairs=600, orient=(1, 0, 0, 1), failed=(0, 1, 1, 0), window="ahead"),
    "mixed4":      dict(seed=303, n_pairs=600, orient=(1, 1, 1, 1), failed=(0, 0, 0, 0), window="ahead"),
    # 520 FR, 40 FF (above MIN_DIR_RATIO = 5 % of the FR count), 14 RF (at least MIN_DIR_CNT = 10 but below the ratio), no RR; only FR pairs
    # get noisy mates, so the small classes keep their counts
    "minor_dir":   dict(seed=304, n_pairs=574, orient=(40, 520, 14, 0), noisy_orient=(FR,), failed=(0, 0, 1, 1), window="ahead"),
    "mid_insert":  dict(seed=305, n_pairs=400, frag=(1300, 200), frag_clip=(400, 2600), failed=(1, 0, 1, 1), window="lds"),
    "wide_insert": dict(seed=306, n_pairs=400, frag=(3000, 550), frag_clip=(600, 6000), failed=(1, 0, 1, 1), window="slab"),
    "ragged":      dict(seed=307, n_pairs=600, len1=(30, 300), len2=(30, 300), forced_lens=BOUNDARY_LENS, forced_copies=4,
                        failed=(1, 0, 1, 1), window="ahead"),
    "edges":       dict(seed=308, n_pairs=600, orient=(1, 1, 1, 1), edge_share=.4, flush_share=.4, failed=(0, 0, 0, 0), window="ahead"),
}
_GEN_KEYS = ("seed", "n_pairs", "orient", "frag", "frag_clip", "len1", "len2", "forced_lens", "forced_copies", "noisy_share", "noisy_orient",
             "clean", "noisy", "noisy_max_run", "edge_share", "edge_within", "flush_share")


GOLDEN_PAIRS = 300          # pairs per library in tests/golden/pelib_* (minor_dir in full: its class counts are the point)


def golden_pairs(name):
    return LIBRARIES[name]["n_pairs"] if name == "minor_dir" else GOLDEN_PAIRS


def library(genome, name, n_pairs=None):
    kw = {k: v for k, v in LIBRARIES[name].items() if k in _GEN_KEYS}
    if n_pairs is not None:
        kw["n_pairs"] = n_pairs
    return make_library(genome, **kw)


def write_library(genome, name, d, n_pairs=None):
    """-> (fq1, fq2, reads1, reads2, meta) with the two files written into directory d."""
    r1, r2, meta = library(genome, name, n_pairs)
    fq1, fq2 = os.path.join(str(d), f"{name}_1.fq"), os.path.join(str(d), f"{name}_2.fq")
    write_fastq(fq1, r1); write_fastq(fq2, r2)
    return fq1, fq2, r1, r2, meta


# ---------------------------------------------------------------------------------------------------- stage records
def split_pe(records):
    """[(tag, arr)] of a paired-end stage dump -> (PESTAT array, list of {tag: arr} per read)."""
    pestat = [a for t, a in records if t == STAGE_PESTAT]
    assert len(pestat) == 1
    return pestat[0], common.by_read([(t, a) for t, a in records if t != STAGE_PESTAT])


def oracle_pe_stages(prefix, fq1, fq2, out, flags=()):
    subprocess.check_call([common.ORACLE, "stages", *flags, prefix, fq1, fq2, out])
    return split_pe(bw.read_record_file(out))


def oracle_sam(prefix, fq1, fq2, flags=()):
    return subprocess.run([common.ORACLE, "mem", *flags, prefix, fq1, fq2], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout


def pestat_dicts(ps):
    return [dict(low=int(ps[5 * d]), high=int(ps[5 * d + 1]), failed=int(ps[5 * d + 2]),
                 avg=float(np.array([ps[5 * d + 3]], np.int64).view(np.float64)[0]), std=float(np.array([ps[5 * d + 4]], np.int64).view(np.float64)[0]))
            for d in range(4)]


def pes0_from(ps):
    """PESTAT record -> the pes0 argument of the product's entries."""
    pes0 = (bw.PeStat * 4)()
    for d, p in enumerate(pestat_dicts(ps)):
        pes0[d].low, pes0[d].high, pes0[d].failed, pes0[d].avg, pes0[d].std = p["low"], p["high"], p["failed"], p["avg"], p["std"]
    return pes0


def window_class(ps, l_ms=150):
    w = max(p["high"] - p["low"] + l_ms for p in pestat_dicts(ps) if not p["failed"])
    return "ahead" if w <= 1024 else "lds" if w <= 4096 else "slab"


def rescued_reads(reads):
    """Reads whose list mem_matesw changed."""
    return [i for i, r in enumerate(reads) if not np.array_equal(r[STAGE_REGS], r[STAGE_REGS_PE])]


def off_contig_windows(ps, reads, lens, contig_lens):
    """Rescue windows (bwamem_pair.c:153-166) whose middle lies in another contig than the anchor, so that the alignment is not attempted:
    counted over the best region of every read whose mate has no region at all -- there no orientation is skipped but the failed ones."""
    pes = pestat_dicts(ps)
    off = np.concatenate([[0], np.cumsum(contig_lens)])
    l_pac = int(off[-1])
    n = 0
    for i, rd in enumerate(reads):
        me, mate = rd[STAGE_REGS], reads[i ^ 1][STAGE_REGS]
        if int(me[0]) == 0 or int(mate[0]) != 0:
            continue
        arb, arid, l_ms = int(me[1]), int(me[5]), int(lens[i ^ 1])
        for r in range(4):
            if pes[r]["failed"]:
                continue
            is_rev, is_larger = (r >> 1) != (r & 1), not (r >> 1)
            lo, hi = pes[r]["low"], pes[r]["high"]
            if not is_rev:
                rb = arb + lo if is_larger else arb - hi
                re = (arb + hi if is_larger else arb - lo) + l_ms
            else:
                rb = (arb + lo if is_larger else arb - hi) - l_ms
                re = arb + hi if is_larger else arb - lo
            rb, re = max(rb, 0), min(re, 2 * l_pac)
            if rb >= re:
                continue
            mid = (rb + re) >> 1
            fwd = 2 * l_pac - 1 - mid if mid >= l_pac else mid
            n += int(np.searchsorted(off, fwd, side="right") - 1 != arid)
    return n


def preconditions(name, ps, reads, lens):
    """What library `name` is for, asserted on the CPU path's records (ps, reads: oracle_pe_stages; lens: length of every read)."""
    spec = LIBRARIES[name]
    failed = tuple(p["failed"] for p in pestat_dicts(ps))
    assert failed == spec["failed"], f"{name}: mem_pestat failed flags {failed}, meant {spec['failed']}"
    assert window_class(ps) == spec["window"], f"{name}: window class {window_class(ps)} ({pestat_dicts(ps)}), meant {spec['window']}"
    resc = rescued_reads(reads)
    assert len(resc) >= 30, f"{name}: mate rescue changed only {len(resc)} lists"
    have = {int(lens[i]) for i in resc}
    want = set(spec.get("forced_lens", ()))
    assert want <= have, f"{name}: no rescued mate of length {sorted(want - have)}"
