"""The synthetic records of the BAI tests (tests/test_bai_cpu.py, tests/test_gpu_bai.py): valid minimal BAM records -- 36 bytes, a
name, a CIGAR, padding -- in coordinate order, with member lengths chosen here.  assert_families checks on the judge's output
(tests/bai_ref.py) that every family the tests are about is in the set, so that the set cannot quietly lose one."""
import random
import struct

import numpy as np

import bai_ref

BLOCK = 65280
M, I, D, N, S, H, P, EQ, X = range(9)
N_REF = 5
BASE = 1234                                      # the file offset of the first member of the records


def rec(ref, pos, cigar=(), flag=0, size=None, name=b"r\0", bin_field=0):
    """One record; its bin field is deliberately not the right one (the index must compute it)."""
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name), 0, bin_field, len(cigar), flag, 0, -1, -1, 0) + name
    body += b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar)
    if size is not None:
        assert size >= 4 + len(body)
        body += bytes(size - 4 - len(body))
    return struct.pack("<i", len(body)) + body


def ordinary(n_bytes, ref=0, pos0=1000, seed=1):
    """At least n_bytes of ordinary records in coordinate order."""
    rng, out, pos, got = random.Random(seed), [], pos0, 0
    while got < n_bytes:
        pos += rng.randrange(0, 300)
        out.append(rec(ref, pos, [(rng.randrange(30, 151), M)], size=rng.randrange(200, 420), flag=16 * rng.randrange(2)))
        got += len(out[-1])
    return out


def member_lens(total, seed):
    rng = random.Random(seed)
    return np.array([rng.randrange(100, 65537) for _ in range((total + BLOCK - 1) // BLOCK)], dtype=np.int32)


def offsets_of(lens, base=BASE):
    return [base + int(x) for x in np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))]


def make_case(records, seed=7, n_ref=N_REF):
    total = sum(map(len, records))
    lens = member_lens(total, seed)
    off = np.zeros(len(records) + 1, dtype=np.int64)
    if records:
        off[1:] = np.cumsum([len(r) for r in records])
    return dict(records=records, n_ref=n_ref, lens=lens, base=BASE, offsets=offsets_of(lens), rec_off=off, total=total, buf=b"".join(records))


def synthetic(whole_blocks):
    """whole_blocks: the last record is padded so that the stream ends on a block cut."""
    r = [rec(0, 0, [(10, M)], size=BLOCK)]                                         # ends exactly on the first cut; the next begins there
    r += [rec(0, 10, [(5, S), (3, I)]), rec(0, 11, [(4, H), (2, P)]), rec(0, 12, [(50, M)], flag=4)]   # rlen 0; 0x4 with a CIGAR
    r += [rec(0, 100, [(50, M)]), rec(0, 200, [(20000, M)]), rec(0, 300, [(50, EQ)]), rec(0, 400, [(20, X), (30, M)])]   # bin 4681, its parent 585, 4681 again: joined
    r += [rec(0, 500, [(20000, M)], size=140000), rec(0, 600, [(50, M)])]            # 140 000 bytes of the parent bin between: not joined
    r += [rec(0, 131000, [(200, M)]), rec(0, (1 << 20) - 50, [(100, M)]), rec(0, (1 << 23) - 10, [(20, D), (5, M)])]   # levels 3, 2, 1
    r += [rec(0, 1 << 24, [(10, M), (1 << 26, N), (10, M)])]                          # level 0
    r += ordinary(150000, 0, 1 << 25, seed=3)
    r += [rec(0, (1 << 29) - 100, [(100, M)])]                                       # e = 2^29 exactly
    r += [rec(2, 50000, [(30, M)]), rec(2, 50010, [], flag=4 | 1), rec(2, 70000, [(10, M)], flag=16)]   # reference 1 has none; windows 0 .. 2 of reference 2 are filled from 3
    r += [rec(3, 5, [(1, M)])]
    r += [rec(-1, -1, [], flag=4) for _ in range(3)]                               # no coordinate; reference 4 has none either
    total = sum(map(len, r))
    if whole_blocks:
        r[-1] = rec(-1, -1, [], flag=4, size=len(r[-1]) + (-total) % BLOCK)
    c = make_case(r, seed=11 if whole_blocks else 12)
    assert (c["total"] % BLOCK == 0) == whole_blocks and c["total"] > 0
    return c


def assert_families(c, want):
    """want: the judge's bytes for case c (a synthetic() one)."""
    idx = bai_ref.parse(want)
    f = [bai_ref.fields(x, c["n_ref"]) for x in c["records"]]
    u = c["rec_off"].tolist()
    assert BLOCK in u[:-1] and BLOCK in u[1:]                                        # begins / ends exactly on a cut
    assert any(b // BLOCK - a // BLOCK >= 2 and b - a == 140000 for a, b in zip(u, u[1:]))   # spans three blocks
    levels = {bai_ref.level_of(b) for R in idx["refs"] for b in R["bins"]}
    assert levels == {0, 1, 2, 3, 4, 5}, levels
    assert any(x[2] == 1 << 29 for x in f)
    cig_only = [x for x, r in zip(f, c["records"]) if struct.unpack_from("<H", r, 16)[0] and x[2] == x[1] + 1 and not x[4]]
    assert len(cig_only) >= 2                                                        # S / H / I / P only
    assert any(x[4] and struct.unpack_from("<H", r, 16)[0] and x[2] == x[1] + 1 for x, r in zip(f, c["records"]))   # 0x4 with a CIGAR
    bins0 = [x[3] for x in f if x[0] == 0]
    runs = sum(1 for k, b in enumerate(bins0) if b == 4681 and (k == 0 or bins0[k - 1] != 4681))
    assert runs == 3 and len(idx["refs"][0]["bins"][4681]) == 2                      # joined once, kept apart once
    assert len(idx["refs"][0]["bins"][585]) >= 1
    lin2 = idx["refs"][2]["lin"]
    assert min(x[1] for x in f if x[0] == 2) >> 14 == 3 and lin2[0] == lin2[1] == lin2[2] == lin2[3]   # filled at the start
    covered = set()
    for x in f:
        if x[0] == 0:
            covered.update(range(x[1] >> 14, ((x[2] - 1) >> 14) + 1))
    lin0 = idx["refs"][0]["lin"]
    assert len(lin0) == 32768 and any(w not in covered and w + 1 in covered and lin0[w] == lin0[w + 1] for w in range(1, 32767))   # and in the middle
    assert not idx["refs"][1]["bins"] and not idx["refs"][1]["lin"] and idx["refs"][0]["bins"] and idx["refs"][2]["bins"] and not idx["refs"][4]["bins"]
    assert idx["n_no_coor"] == 3
    assert idx["refs"][2]["meta"][1] == (2, 1)                                       # the unmapped read with its mate's coordinates
