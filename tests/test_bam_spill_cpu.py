"""Spilled runs of the device merger, the parts that need no device: bwahip_bam_devmerge_spill_hbm_need against hand-computed cases, the
layout of bwahip_spill_t against a compiled C probe, and the host-side store (bwa-mem-gpu_amd/csrc/spill_store.cpp) and the finish's window
plan (bwa-mem-gpu_amd/csrc/spill_plan.h), each through a stand-alone program (tests/spill_store_check.cpp, tests/spill_plan_check.cpp) built
with the address and undefined-behaviour sanitizers and run as a child process."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import common
from common import bw

INC = os.path.join(common.ROOT, "include")
CSRC = os.path.join(common.ROOT, "bwa-mem-gpu_amd", "csrc")
BLOCK = 65280
PER_BLOCK = 4 * BLOCK + 2 * 31 + 65536 + 12                    # two inputs, two outputs (input + 31), the slot, the member's length and offset


def blocks(n):
    return (n + BLOCK - 1) // BLOCK


def want_need(res, sp, longest, n_rec, n_runs, pb, wp):
    """include/bwahip.h, term by term."""
    stage = min(wp * pb * BLOCK + 2 * longest, sp)
    pieces = PER_BLOCK * (min(blocks(res + sp), pb) - min(blocks(res), pb))
    table = 16 * (n_runs + 1) * blocks(res + sp)
    work = 2 * stage + pieces + table
    return bw.bam_devmerge_hbm_need(res, n_rec, n_runs, pb) + work + work // 8


def test_spill_hbm_need_refuses_bad_arguments(built):
    good = dict(resident_raw_bytes=1000, spilled_raw_bytes=1000, longest_record=100, n_records=10, n_runs=2, piece_blocks=1, window_pieces=1)
    assert bw.bam_devmerge_spill_hbm_need(**good) > 0
    for k, bad in (("resident_raw_bytes", -1), ("spilled_raw_bytes", -1), ("longest_record", -1), ("n_records", -1), ("n_runs", -1), ("piece_blocks", 0), ("piece_blocks", 4097),
                   ("window_pieces", 0), ("window_pieces", -3), ("window_pieces", 65537)):
        assert bw.bam_devmerge_spill_hbm_need(**dict(good, **{k: bad})) == -1, (k, bad)


def test_spill_hbm_need_is_the_resident_need_plus_the_documented_terms(built):
    # 1. nothing spilled: the resident merger's need and the cut table of its blocks alone
    res, n = 10 * BLOCK, 2000
    table = 16 * 4 * 10
    assert bw.bam_devmerge_spill_hbm_need(res, 0, 400, n, 3, 4, 2) == bw.bam_devmerge_hbm_need(res, n, 3, 4) + table + table // 8
    # 2. everything spilled, windows far smaller than the spilled bytes: two windows with two straddlers each, all piece buffers, the table
    sp = 1000 * BLOCK
    stage = 8 * 16 * BLOCK + 2 * 500
    work = 2 * stage + PER_BLOCK * 16 + 16 * 8 * 1000
    assert bw.bam_devmerge_spill_hbm_need(0, sp, 500, 100000, 7, 16, 8) == bw.bam_devmerge_hbm_need(0, 100000, 7, 16) + work + work // 8
    # 3. a mix in which one window covers all spilled bytes, and the resident bytes already fill a piece: no staging beyond the bytes, no piece term
    res, sp = 40 * BLOCK + 5, 3 * BLOCK - 7
    work = 2 * sp + 0 + 16 * 3 * blocks(res + sp)
    assert blocks(res + sp) == 43
    assert bw.bam_devmerge_spill_hbm_need(res, sp, 70000, 5000, 2, 32, 2) == bw.bam_devmerge_hbm_need(res, 5000, 2, 32) + work + work // 8
    for args in ((res, 0, 400, n, 3, 4, 2), (0, 1000 * BLOCK, 500, 100000, 7, 16, 8), (res, sp, 70000, 5000, 2, 32, 2), (123456, 7654321, 333, 40000, 9, 3, 5)):
        assert bw.bam_devmerge_spill_hbm_need(*args) == want_need(*args), args


def test_spill_hbm_need_never_falls_as_an_argument_grows(built):
    base = [3 * BLOCK + 11, 20 * BLOCK - 3, 777, 9000, 5, 2, 3]
    steps = [(1, BLOCK - 1, BLOCK, 7 * BLOCK, 1 << 33), (1, BLOCK, 9 * BLOCK + 1, 1 << 34), (1, 1000, 1 << 20, 1 << 31), (1, 10 ** 6, 2 ** 31 - 9001), (1, 50, 5000),
             (1, 2, 9, 20, 100, 4094), (1, 2, 3, 10, 1000, 65533)]
    for k, incs in enumerate(steps):
        last = bw.bam_devmerge_spill_hbm_need(*base)
        for inc in incs:
            args = list(base)
            args[k] += inc
            now = bw.bam_devmerge_spill_hbm_need(*args)
            assert now >= last > 0, (k, inc)
            last = now
    for pb in range(1, 40):                                                                # and step by step where the pieces and the windows change
        for wp in range(1, 12):
            here = bw.bam_devmerge_spill_hbm_need(3 * BLOCK, 20 * BLOCK, 777, 9000, 5, pb, wp)
            assert bw.bam_devmerge_spill_hbm_need(3 * BLOCK, 20 * BLOCK, 777, 9000, 5, pb + 1, wp) >= here
            assert bw.bam_devmerge_spill_hbm_need(3 * BLOCK, 20 * BLOCK, 777, 9000, 5, pb, wp + 1) >= here
            assert bw.bam_devmerge_spill_hbm_need(3 * BLOCK + 1, 20 * BLOCK, 777, 9000, 5, pb, wp) >= here


def test_spill_struct_layout_is_the_headers(built, tmp_path):
    fields = [f for f, _ in bw.SpillStats._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bwahip.h"\nint main(void) { printf("%zu", sizeof(bwahip_spill_t));\n' +
                   "".join(f' printf(" %zu", offsetof(bwahip_spill_t, {f}));\n' for f in fields) + " return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + INC, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(bw.SpillStats)] + [getattr(bw.SpillStats, f).offset for f in fields]
    assert fields[:3] == ["host_budget", "tmp_dir", "window_pieces"] and len(fields) == 11


def test_store_round_trips_under_the_sanitizers(built, tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe, d, f = tmp_path / "spill_store_check", tmp_path / "dir", tmp_path / "file"
    d.mkdir()
    f.write_bytes(b"x")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + INC, "-I" + CSRC,
                           os.path.join(common.ROOT, "tests", "spill_store_check.cpp"), os.path.join(CSRC, "spill_store.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(d), str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert os.listdir(d) == []


def test_window_plan_holds_under_the_sanitizers(built, tmp_path):
    """tests/spill_plan_check.cpp: 1, 3 and 7 runs with every subset spilled, window_pieces 1, 2 and beyond the pieces, an empty run, a run
    inside one window, a tie block and a record over three windows, and every malformed cut table the plan refuses."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "spill_plan_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + INC, "-I" + CSRC,
                           os.path.join(common.ROOT, "tests", "spill_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
