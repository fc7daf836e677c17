"""The synthetic records of the QC tests (tests/test_qc_cpu.py, tests/test_gpu_qc.py): minimal BAM records built by hand over references
whose lengths sit at 1 and around the wavefront (64), the workgroup (256), the scan tile (2048) and the windows 2^4, 2^8 and 2^14 -- a
reference of 2^29 bases is beyond a test of seconds, so window_shift 29 is covered as "one window per reference" --, one reference of
several tiles, one without any record and one that only holds a stack of records for the depths around the cap bin.  assert_families
checks on the judge's own reading (tests/qc_ref.py) that everything the tests are about is in the set, so that it cannot quietly lose one."""
import random
import struct

import numpy as np

import qc_ref as ref
from qc_ref import D, EQ, H, I, M, N, P, S, X

TILE = 2048
REF_LEN = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 16383, 16384, 16385, 5000, 300, 130]
TILES_REF, EMPTY_REF, STACK_REF = 16, 17, 18
SHIFTS = (4, 8, 14)                              # the window sizes whose boundaries the set must cross
MAPQS = (0, 3, 4, 5, 20, 29, 30, 60, 255)
TLENS = (0, -200, 1, 150, 400, 1023, 1024, 1025, 5000)


def rec(name, ref_id, pos, cigar=(), flag=0, mapq=60, next_ref=-1, next_pos=-1, tlen=0, tail=b""):
    """One record without bases: 36 bytes, the name, the CIGAR operations [(length, op)], then `tail`."""
    name = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), mapq, 0, len(cigar), flag, 0, next_ref, next_pos, tlen) + name
    body += b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar) + tail
    return struct.pack("<i", len(body)) + body


def _cigar(rng, span):
    """A CIGAR over about `span` reference bases."""
    k = rng.randrange(8)
    a = max(1, span // 3)
    if k == 0:
        return [(span, M)]
    if k == 1:
        return [(rng.randrange(1, 9), S), (a, M), (rng.randrange(1, 5), I), (a, M)]
    if k == 2:
        return [(a, M), (rng.randrange(1, 7), D), (a, EQ), (rng.randrange(1, 4), X)]
    if k == 3:
        return [(rng.randrange(1, 9), H), (a, M), (rng.randrange(1, 200), N), (a, M), (rng.randrange(1, 9), S)]
    if k == 4:
        return [(a, EQ), (rng.randrange(1, 3), P), (a, X), (rng.randrange(1, 5), H)]
    if k == 5:
        return [(a, M), (2, N), (3, D), (1, I), (a, M)]
    if k == 6:
        return [(rng.randrange(5, 40), S), (rng.randrange(1, 20), I)]                      # nothing on the reference
    return [(span, M), (3, S)]


def _flag(rng):
    f = 0
    if rng.random() < 0.8:
        f |= 0x1 | rng.choice((0x40, 0x80, 0x40, 0x80, 0, 0xc0))
        if rng.random() < 0.55:
            f |= 0x2
        if rng.random() < 0.2:
            f |= 0x8
        if rng.random() < 0.4:
            f |= 0x20
    for bit, p in ((0x4, 0.1), (0x10, 0.5), (0x100, 0.1), (0x800, 0.07), (0x400, 0.13), (0x200, 0.3)):
        if rng.random() < p:
            f |= bit
    return f


def record_set(seed=3, n_random=2600):
    rng = random.Random(seed)
    out = []
    busy = [r for r in range(len(REF_LEN)) if r not in (EMPTY_REF, STACK_REF)]
    for k in range(n_random):
        r = rng.choice(busy)
        L = REF_LEN[r]
        pos = rng.randrange(0, L)
        flag = _flag(rng)
        nxt = r if rng.random() < 0.6 else rng.choice((-1, *busy))
        out.append(rec(b"q%d" % k + b"x" * (k % 4), r, pos, _cigar(rng, rng.randrange(1, 151)), flag, rng.choice(MAPQS), nxt, rng.randrange(0, L), rng.choice(TLENS),
                       tail=bytes(rng.randrange(0, 4))))
    for r in busy:                                                   # from base 0 to exactly the end; beyond the end; the last base alone
        L = REF_LEN[r]
        out += [rec(b"whole", r, 0, [(L, M)]), rec(b"beyond", r, L - 1, [(10, M)], 0x10), rec(b"d_beyond", r, max(0, L - 3), [(2, M), (9, D), (4, M)]), rec(b"last", r, L - 1, [(1, X)])]
    out += [rec(b"tilecross", TILES_REF, TILE - 8, [(20, M)]), rec(b"tiles", TILES_REF, 100, [(2 * TILE + 50, EQ)]), rec(b"n_over_tile", TILES_REF, TILE - 3, [(2, M), (TILE, N), (2, M)])]
    out += [rec(b"nocigar", 5, 10, [], 0), rec(b"nocigar_pe", 6, 3, [], 0x1 | 0x40 | 0x2, next_ref=6, tlen=1024)]   # mapped, no CIGAR
    for bit in (0x4, 0x100, 0x200, 0x400):                           # excluded by exactly one bit of 1796; by mapq alone
        out.append(rec(b"only%x" % bit, 7, 20, [(30, M)], bit))
    out += [rec(b"mq29", 7, 50, [(30, M)], 0, mapq=29), rec(b"mq30", 7, 60, [(30, M)], 0, mapq=30)]
    for tlen in (1023, 1024, 1025, 1):                               # the insert-size bins around the cap
        out.append(rec(b"is%d" % tlen, 8, 5, [(20, M)], 0x1 | 0x2 | 0x40, next_ref=8, tlen=tlen))
    out += [rec(b"nc%d" % k, -1, -1, [], 0x4 | (0x1 | 0x80 | 0x8 if k & 1 else 0), mapq=0, tail=bytes(k)) for k in range(7)]
    out += [rec(b"nc_cig", -1, 77, [(20, M)], 0x4)]                   # no reference: its CIGAR covers nothing
    # depth 254 on [100, 105), 255 on [105, 110), 256 on [110, 115), 306 on [115, 120) of a reference nothing else touches
    out += [rec(b"st%d" % k, STACK_REF, 100, [(20, M)]) for k in range(254)] + [rec(b"st255", STACK_REF, 105, [(15, M)]), rec(b"st256", STACK_REF, 110, [(10, M)])]
    out += [rec(b"top%d" % k, STACK_REF, 115, [(5, M)]) for k in range(50)]
    rng.shuffle(out)
    return make_case(out)


def make_case(records, ref_len=REF_LEN, shift=0):
    """shift: bytes in front of the first record (the offsets do not start at 0)."""
    off = np.zeros(len(records) + 1, dtype=np.int64)
    if records:
        off[1:] = np.cumsum([len(r) for r in records])
    return dict(records=records, ref_len=list(ref_len), buf=b"\x5a" * shift + b"".join(records), off=off + shift)


def ordinary(n_bytes, seed=1):
    """At least n_bytes of ordinary records (long tails, so that few of them are many bytes)."""
    rng, out, got = random.Random(seed), [], 0
    while got < n_bytes:
        out.append(rec(b"o%d" % len(out), TILES_REF, rng.randrange(0, 4900), [(rng.randrange(30, 151), M)], 16 * rng.randrange(2), tail=bytes(rng.randrange(150, 260))))
        got += len(out[-1])
    return out


def bad_records(n_ref=len(REF_LEN)):
    """name -> (record, the rule refuses it).  The table of tests/test_gpu_markdup.py::test_kat_dup_desc_refusals: what the rule checks
    (length, block_size, name + CIGAR) is refused; l_seq is not among the fields the rule reads, so those records count as they are.  And
    the two checks that table has no use for: refID and pos."""
    good = rec(b"bad", 0, 0, [(1, M)], 0)
    good_seq = good[:20] + struct.pack("<i", 10) + good[24:] + b"\x11" * 5 + b"\x20" * 10
    good_seq = struct.pack("<i", len(good_seq) - 4) + good_seq[4:]
    patched = lambda src, at, fmt, v: (lambda b: (struct.pack_into(fmt, b, at, v), bytes(b))[1])(bytearray(src))
    raw = lambda n: struct.pack("<iiiBBHHH", n - 4, 0, 0, 1, 0, 0, 0, 0) + bytes(n - 20)
    return {"block_size below 32": (raw(20), True), "a read of 35 bytes": (raw(35), True), "block_size one too large": (patched(good, 0, "<i", len(good) - 3), True),
            "block_size one too small": (patched(good, 0, "<i", len(good) - 5), True), "bytes after the last record": (good + b"\0" * 10, True),
            "n_cigar_op beyond the record": (patched(good, 16, "<H", 60000), True), "l_read_name beyond the record": (patched(good, 12, "<B", 255), True),
            "l_seq beyond the record": (patched(good_seq, 20, "<i", 1 << 30), False), "l_seq negative": (patched(good_seq, 20, "<i", -1), False),
            "l_seq one too large": (patched(good_seq, 20, "<i", 11), False),
            "refID = n_ref": (rec(b"bad", n_ref, 0, [(1, M)]), True), "refID = 2^31 - 1": (rec(b"bad", 0x7fffffff, 0), True),
            "pos < 0 on a reference": (rec(b"bad", 0, -1, [(1, M)]), True), "pos < 0 without a reference": (rec(b"bad", -1, -5), False)}


def assert_families(case):
    recs, lens = case["records"], case["ref_len"]
    f = [ref.fields(r, len(lens)) for r in recs]
    assert 2000 <= len(recs) <= 6000
    s = ref.summary(recs, lens)
    counts = s["count"][0] + s["count"][1]
    assert all(counts) and len(set(counts)) == 32, counts                                  # every category non-zero, no two alike
    ops = {op for x in f for _, op in x["cigar"]}
    assert ops == set(range(9)), ops
    assert any(not x["cigar"] and x["ref"] >= 0 and not x["flag"] & 0x4 for x in f)        # mapped, no CIGAR
    assert s["n_no_coor"] >= 5 and any(x["ref"] < 0 and x["cigar"] for x in f)
    iv = [(x["ref"], a, b) for x in f if ref.takes_part(x, ref.resolve()) for a, b in ref.intervals(x, lens[x["ref"]])]
    assert any(a == 0 for _, a, _ in iv) and any(b == lens[r] for r, _, b in iv)
    raw_end = lambda x: x["pos"] + sum(n for n, op in x["cigar"] if op in ref.REF_OPS)
    assert any(x["ref"] >= 0 and ref.takes_part(x, ref.resolve()) and raw_end(x) > lens[x["ref"]] and ref.intervals(x, lens[x["ref"]]) for x in f)   # clipped
    assert any(a // TILE != (b - 1) // TILE for _, a, b in iv)
    for ws in SHIFTS:
        assert any(a >> ws != (b - 1) >> ws for _, a, b in iv), ws
        assert {(1 << ws) - 1, 1 << ws, (1 << ws) + 1} <= set(lens), ws
    for n in (64, 256, TILE):
        assert {n - 1, n, n + 1} <= set(lens) and 1 in lens
    assert max(lens) < 3 * TILE * 3 and any(n > 2 * TILE for n in lens)
    dep = ref.depths(recs, lens)
    flat = {d for row in dep for d in row}
    assert {254, 255, 256} <= flat and max(flat) > 300, sorted(flat)[-5:]
    assert s["refs"][EMPTY_REF]["mapped"] + s["refs"][EMPTY_REF]["placed_unmapped"] == 0 and not any(dep[EMPTY_REF])
    cov = lambda x: x["ref"] >= 0 and any(op in ref.COVER_OPS for _, op in x["cigar"])
    for bit in (0x4, 0x100, 0x200, 0x400):
        assert any(cov(x) and x["flag"] & ref.DEFAULT_EXCLUDE == bit for x in f), hex(bit)
    assert any(cov(x) and not x["flag"] & ref.DEFAULT_EXCLUDE and x["mapq"] < 30 for x in f) and any(cov(x) and x["mapq"] == 30 for x in f)
    for t in (1023, 1024, 1025):
        assert s["isize_hist"][min(t, 1024)] and any(x["tlen"] == t and x["flag"] & 0x90f == 0x3 for x in f), t
    assert s["isize_hist"][1024] > s["isize_hist"][1023] > 0
    assert sum(1 for v in s["mapq_hist"] if v) >= len(MAPQS)
    starts, o = set(), 0
    for r in recs:
        starts.add(o % 4)
        o += len(r)
    assert starts == {0, 1, 2, 3}                                    # records at every alignment
    return s
