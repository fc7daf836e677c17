"""BGZF on the CPU side: tests/bgzf_ref.py (the member parser the GPU tests judge with) against the host writer, and the C ABI of the
GPU deflate stage (declared, exported, mirrored).  No GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import bgzf_ref
import common
from common import bw

HDR = os.path.join(common.ROOT, "include", "bwahip.h")
NEW = ["bwahip_kat_bgzf", "bwahip_process_seqs_bgzf", "bwahip_batch_run_bgzf", "bwahip_batch_bgzf", "bwahip_stream_run_bam_dev"]


def _text(n, seed):
    rnd = random.Random(seed)
    words = [bytes(rnd.choice(b"ACGTNacgt=:\tIF#") for _ in range(rnd.randint(2, 12))) for _ in range(60)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words)
    return bytes(out[:n])


def _host_bgzf(tmp_path, data, level, threads=1):
    p = str(tmp_path / f"h{level}_{threads}.bgzf")
    fd = os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        bw.bgzf_write(fd, data, level, threads)
    finally:
        os.close(fd)
    return open(p, "rb").read()


@pytest.mark.parametrize("level", [0, 1])
def test_parser_reads_what_the_host_writer_makes(built, tmp_path, level):
    data = _text(2 * 65280 + 1234, 5)
    got = _host_bgzf(tmp_path, data, level, 3)
    ms = bgzf_ref.parse(got)
    assert [m["data"] for m in ms] == bgzf_ref.blocks_of(data) and len(ms) == 3
    assert all(m["btype"] == (0 if level == 0 else 2) for m in ms)
    if level == 0:
        assert [m["size"] for m in ms] == [65280 + 5 + 26, 65280 + 5 + 26, 1234 + 5 + 26]
    else:
        assert sum(m["deflate_len"] for m in ms) == sum(bgzf_ref.zlib_deflate_len(b, 1) for b in bgzf_ref.blocks_of(data))
    assert bgzf_ref.inflate(got + bgzf_ref.EOF_BLOCK) == data
    assert bgzf_ref.parse(bgzf_ref.EOF_BLOCK)[0]["data"] == b""


@pytest.mark.parametrize("level", [0, 1])
def test_parser_refuses_damaged_members(built, tmp_path, level):
    data = _text(70000, 6)
    good = _host_bgzf(tmp_path, data, level)
    first = bgzf_ref.parse(good)[0]["size"]
    crc_flipped = bytearray(good)
    crc_flipped[first - 8] ^= 0x01                                 # a CRC byte of the first member
    with pytest.raises(bgzf_ref.BgzfError, match="CRC32"):
        bgzf_ref.parse(bytes(crc_flipped))
    for delta in (-1, 1):                                          # BSIZE one too small / too large
        wrong = bytearray(good)
        b = int.from_bytes(wrong[16:18], "little") + delta
        wrong[16:18] = b.to_bytes(2, "little")
        with pytest.raises(bgzf_ref.BgzfError):
            bgzf_ref.parse(bytes(wrong))
    for cut in (1, 8, 9, 30, first - 27):                          # truncated: inside the trailer, the stream, down to less than a member
        with pytest.raises(bgzf_ref.BgzfError):
            bgzf_ref.parse(good[:first - cut])
    isize = bytearray(good)
    isize[first - 4] ^= 0x01
    with pytest.raises(bgzf_ref.BgzfError, match="ISIZE"):
        bgzf_ref.parse(bytes(isize))
    magic = bytearray(good)
    magic[3] = 0
    with pytest.raises(bgzf_ref.BgzfError):
        bgzf_ref.parse(bytes(magic))


def test_header_declares_and_library_exports_the_device_bgzf_entry_points(built):
    text = open(HDR).read()
    declared = set(re.findall(r"\b(bwahip_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(bw.LIB_PATH)
    for s in NEW:
        assert s in declared, f"{s} is not declared in include/bwahip.h"
        assert hasattr(lib, s), f"{s} is not exported by libbwahip.so"
    assert "bwahip_bgzf_stats_t" in text


def test_python_mirrors_exist(built):
    for m in ("kat_bgzf", "process_seqs_bgzf", "process_seqs_bgzf_array", "batch_run_bgzf", "batch_bgzf"):
        assert callable(getattr(bw.Context, m, None)), m
    assert callable(getattr(bw, "stream_run_bam_dev", None))
    assert [f[0] for f in bw.BgzfStats._fields_] == ["raw_bytes", "bgzf_bytes", "n_blocks", "n_stored", "deflate_ms"]
    L = bw.lib()
    for s in NEW:
        assert getattr(L, s).argtypes, s


def test_stats_mirror_has_the_size_of_the_c_struct(built, tmp_path):
    """sizeof and the field offsets of bwahip_bgzf_stats_t as the C compiler lays it out; bwahip_stream_t keeps its layout."""
    src = tmp_path / "sz.c"
    src.write_text(r'''
#include <stddef.h>
#include "bwahip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(bwahip_bgzf_stats_t), offsetof(bwahip_bgzf_stats_t, raw_bytes), offsetof(bwahip_bgzf_stats_t, bgzf_bytes),
           offsetof(bwahip_bgzf_stats_t, n_blocks), offsetof(bwahip_bgzf_stats_t, n_stored), offsetof(bwahip_bgzf_stats_t, deflate_ms), sizeof(bwahip_stream_t));
    return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(common.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    S = bw.BgzfStats
    assert got[:6] == [C.sizeof(S), S.raw_bytes.offset, S.bgzf_bytes.offset, S.n_blocks.offset, S.n_stored.offset, S.deflate_ms.offset]
    assert got[0] == 40 and got[6] == C.sizeof(bw.StreamStats) == 80
